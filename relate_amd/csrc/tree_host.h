// tree_host.h -- what the host sides of the tree modes share (compare.cpp: CompareTopology; pairwise.cpp:
// PairwiseCoalescence): the check of a tree's shape and the wording of a refusal, the tables of one tree that the
// device builds with the passes of tree_passes.h, and the trees of an .anc file as the C entry points take them.
#pragma once
#include <vector>

#include "anc_file.h"

namespace rl {

// the shape every tree of this library has (MinMatch numbers a merged cluster after its parts): binary, leaves
// 0..N-1, parent[v] > v, root 2N-2.  0, or the first node that breaks the rule + 1.
int first_bad_node(const int *parent, int N, std::vector<unsigned char> &kids);
// sets the message that names the node first_bad_node finds, behind `tree` ("rl_compare_trees: tree 3 of A",
// "<where>: tree 3"); RL_EINVAL
int refuse_tree(const char *tree, const int *parent, int N);

// One tree's tables by node label.  first / second: the children in node order; size: leaves below; lo: the left
// end of the node's interval of depth-first ranks (the first child first), for a leaf its rank.
struct TreeTables {
  int N, nodes;
  std::vector<int> first, second, size, lo;
  std::vector<unsigned char> kids;  // first_bad_node's
  explicit TreeTables(int n) : N(n), nodes(2 * n - 1), first(nodes), second(nodes), size(nodes), lo(nodes) {}
  // parent must have passed first_bad_node
  void fill(const int *parent);
};

// the parent arrays of the file's trees one after another ([trees][2N-1]) and, if asked for, their branch lengths
void flatten_anc(const AncFile &a, std::vector<int> &parents, std::vector<double> *branch_length = nullptr);

}  // namespace rl
