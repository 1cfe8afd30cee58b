// tree_host.cpp -- see tree_host.h.
#include "tree_host.h"

#include <algorithm>
#include <cstring>

#include "common.h"

namespace rl {

int first_bad_node(const int *parent, int N, std::vector<unsigned char> &kids) {
  const int nodes = 2 * N - 1;
  kids.assign((size_t)nodes, 0);
  for (int v = 0; v < nodes - 1; v++) {
    const int p = parent[v];
    if (!(p > v && p >= N && p < nodes) || ++kids[p] > 2) return v + 1;
  }
  if (parent[nodes - 1] != -1) return nodes;
  for (int v = N; v < nodes; v++)
    if (kids[v] != 2) return v + 1;
  return 0;
}

int refuse_tree(const char *tree, const int *parent, int N) {
  std::vector<unsigned char> kids;
  const int bad = first_bad_node(parent, N, kids);
  const int v = bad - 1;
  if (bad == 0) set_error("%s was refused by the device and not by the host", tree);
  else if (v == 2 * N - 2) set_error("%s: node %d is not the root (parent %d, expected -1) or has not two children", tree, v, parent[v]);
  else if (parent[v] <= v) set_error("%s: parent %d of node %d does not have a label above its child's", tree, parent[v], v);
  else set_error("%s: node %d (parent %d) does not fit a binary tree on %d leaves", tree, v, parent[v], N);
  return RL_EINVAL;
}

void TreeTables::fill(const int *parent) {
  std::fill(first.begin(), first.end(), -1);
  for (int v = 0; v < nodes; v++) size[v] = v < N ? 1 : 0;
  for (int v = 0; v < nodes - 1; v++) {  // label order: a node is complete before its parent reads it
    const int p = parent[v];
    size[p] += size[v];
    if (first[p] == -1) first[p] = v;
    else second[p] = v;
  }
  lo[nodes - 1] = 0;
  for (int p = nodes - 1; p >= N; p--) {  // falling order: a parent hands the left ends down
    lo[first[p]] = lo[p];
    lo[second[p]] = lo[p] + size[first[p]];
  }
}

void flatten_anc(const AncFile &a, std::vector<int> &parents, std::vector<double> *branch_length) {
  const size_t nodes = (size_t)2 * a.N - 1, T = a.trees.size();
  parents.resize(T * nodes);
  if (branch_length) branch_length->resize(T * nodes);
  for (size_t t = 0; t < T; t++) {
    memcpy(&parents[t * nodes], a.trees[t].parent.data(), nodes * sizeof(int));
    if (branch_length) memcpy(&(*branch_length)[t * nodes], a.trees[t].branch_length.data(), nodes * sizeof(double));
  }
}

}  // namespace rl
