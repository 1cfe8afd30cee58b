// tree_host.h -- what the host sides of the tree modes share (compare.cpp: CompareTopology; pairwise.cpp:
// PairwiseCoalescence; coalrate.cpp: CoalescentRateForSection; frequency.cpp: Frequency; mutrate.cpp: AvgMutationRate;
// coaltree.cpp: CoalRateForTree; subtrees.cpp: SubTreesForSubpopulation; mutctx.cpp: MutationRateWithContext): the
// checks of a tree's shape and of its branch lengths and the wording of a refusal (check_tree: the one sequence every
// mode with dated trees goes through), the checks and the makers of the epoch boundaries, the tables of one tree
// that the device builds with the passes of tree_passes.h, and the trees of an .anc file as the C entry points take
// them.
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
// 0, or the first of bl[0..count) that is negative or not finite + 1.  count: 2N-2 (the root's is not read), or 2N-1
// for SubTreesForSubpopulation (the root's ends in the subtree root's)
int first_bad_length(const double *bl, int count);
// A tree on its way to the host's implementation, or one the device refused: RL_OK for a tree the host accepts and
// the device did not refuse; otherwise RL_EINVAL with the message behind `tree_name` -- the node first_bad_node
// finds, the first bad one of the n_lengths branch lengths (none are read if bl_or_null is null), or that the device
// refused what the host accepts.
int check_tree(const char *tree_name, const int *parent, const double *bl_or_null, int N, int n_lengths,
               bool refused_by_device, std::vector<unsigned char> &kids);

// the epoch boundaries of a call (float or double): 2 <= E <= max_epochs, ep[0] = 0, rising, finite.  `who` is the
// entry point a message starts with
template <class T>
int check_epochs(const char *who, const T *ep, int E, int max_epochs);
// The reference's boundaries in generations (CoalescentRateForSection.cpp:306-378, AvgMutationRate.cpp:382-454), in
// the element type T the mode keeps them in: the default 31, or those of `--bins lower,upper,step` (log10 years).
// *nepochs: in, the room in `out`; out, the number of boundaries
template <class T>
int make_epochs(const char *who, float years_per_gen, const char *bins_or_null, T *out, int *nepochs);

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
