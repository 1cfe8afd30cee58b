// pairwise.cpp -- PairwiseCoalescence, host side: S(i,j) = sum over trees of w_t * v_t(i,j), v the number of leaves
// below (metric size) or the height of (metric time) the most recent common ancestor of the leaves i and j
// (include/relate_amd.h has the definitions).
//
// Per tree, as on the device (pairwise_kernels.hip): the leaves are ranked in depth-first order (first child = the
// child with the smaller label, first), every internal node m owns the boundary between the last leaf of its first
// child and the first leaf of its second, g[k] = the node that owns the boundary between the ranks k and k+1.  Labels
// rise towards the root, so MRCA(i,j) is the largest label among g[min(r_i,r_j) .. max(r_i,r_j)-1]: row i of the
// tree's matrix is a running maximum of g outwards from rank[i], one step per element, no walk in the tree.
// This file is that on one thread for any N (the CPU suite's implementation, the yardstick of the GPU tests and the
// `device < 0` path), the sum over .anc files on top of either implementation, and the C entry points.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "anc_file.h"
#include "common.h"
#include "pairwise.h"

namespace rl {

int first_bad_node(const int *parent, int N, std::vector<unsigned char> &kids);  // compare.cpp

namespace {

int refuse_tree(const char *where, long long index, const int *parent, int N) {
  std::vector<unsigned char> kids;
  const int bad = first_bad_node(parent, N, kids);
  const int v = bad - 1;
  if (bad == 0) set_error("%s: tree %lld was refused by the device and not by the host", where, index);
  else if (v == 2 * N - 2) set_error("%s: tree %lld: node %d is not the root (parent %d, expected -1) or has not two children", where, index, v, parent[v]);
  else if (parent[v] <= v) set_error("%s: tree %lld: parent %d of node %d does not have a label above its child's", where, index, parent[v], v);
  else set_error("%s: tree %lld: node %d (parent %d) does not fit a binary tree on %d leaves", where, index, v, parent[v], N);
  return RL_EINVAL;
}

// one tree's tables and its contribution to S
struct HostPairwise {
  int N, nodes;
  std::vector<int> first, second, size, lo, order, g;
  std::vector<double> height;
  std::vector<unsigned char> kids;
  explicit HostPairwise(int n) : N(n), nodes(2 * n - 1), first(nodes), second(nodes), size(nodes), lo(nodes), order(n), g(n), height(nodes) {}

  // parent must have passed first_bad_node
  void prepare(const int *parent, const double *bl) {
    std::fill(first.begin(), first.end(), -1);
    for (int v = 0; v < nodes; v++) size[v] = v < N ? 1 : 0;
    for (int v = 0; v < nodes - 1; v++) {  // label order: a node is complete before its parent reads it
      const int p = parent[v];
      size[p] += size[v];
      if (first[p] == -1) first[p] = v;
      else second[p] = v;
    }
    if (bl) {
      for (int v = 0; v < N; v++) height[v] = 0.0;
      for (int n = N; n < nodes; n++) height[n] = height[first[n]] + bl[first[n]];  // one addition per node
    }
    lo[nodes - 1] = 0;
    for (int p = nodes - 1; p >= N; p--) {  // falling order: a parent hands the left ends down
      const int a = first[p], b = second[p];
      lo[a] = lo[p];
      lo[b] = lo[p] + size[a];
      g[lo[b] - 1] = p;
    }
    for (int v = 0; v < N; v++) order[lo[v]] = v;
  }

  // S[i][j] += w * value(MRCA(i,j)) for every j != i
  template <class sum_t, class Value>
  void add_row(int i, sum_t *row, sum_t w, Value value) const {
    const int r = lo[i];
    int m = 0;
    for (int p = r; p < N - 1; p++) {
      m = std::max(m, g[p]);
      sum_t &s = row[order[p + 1]];
      s = add(s, w, value(m));
    }
    m = 0;
    for (int p = r - 1; p >= 0; p--) {
      m = std::max(m, g[p]);
      sum_t &s = row[order[p]];
      s = add(s, w, value(m));
    }
  }
  static unsigned long long add(unsigned long long s, unsigned long long w, unsigned long long v) { return s + w * v; }
  // the product is rounded, then the sum: no fused multiply-add (pairwise_kernels.hip does the same)
  static double add(double s, double w, double v) {
#pragma clang fp contract(off)
    const double p = w * v;
    return s + p;
  }
};

// the sum in the making, on the host (in the caller's matrix) or on a device
struct Pairwise {
  int N = 0, device = -1;
  bool time = false;
  void *sum_out = nullptr;
  long long W = 0;
  PairwiseDevice *dev = nullptr;
  HostPairwise *host = nullptr;
  ~Pairwise() {
    if (dev) pairwise_device_free(dev);
    delete host;
  }
  int begin(int n, bool t, int d, void *out) {
    N = n, time = t, device = d, sum_out = out;
    if (device >= 0) return pairwise_device_begin(&dev, N, time, device);
    memset(sum_out, 0, (size_t)N * N * 8);
    host = new HostPairwise(N);
    return RL_OK;
  }
  // `where` names the trees' origin in a message: the entry point, or the file
  int add(const int *parents, const double *bl, const long long *weights, int ntrees, const char *where) {
    const size_t nodes = (size_t)2 * N - 1;
    for (int t = 0; t < ntrees; t++) {
      if (weights[t] < 0) {
        set_error("%s: tree %d: weight %lld is negative", where, t, weights[t]);
        return RL_EINVAL;
      }
      W += weights[t];
    }
    if (dev) {
      int bad = -1;
      const int rc = pairwise_device_add(dev, parents, bl, weights, ntrees, &bad);
      return bad >= 0 ? refuse_tree(where, bad, parents + (size_t)bad * nodes, N) : rc;
    }
    for (int t = 0; t < ntrees; t++) {
      const int *parent = parents + t * nodes;
      if (first_bad_node(parent, N, host->kids)) return refuse_tree(where, t, parent, N);
      host->prepare(parent, time ? bl + t * nodes : nullptr);
      const HostPairwise &h = *host;
      for (int i = 0; i < N; i++) {
        if (time) h.add_row(i, static_cast<double *>(sum_out) + (size_t)i * N, (double)weights[t], [&](int m) { return h.height[m]; });
        else h.add_row(i, static_cast<unsigned long long *>(sum_out) + (size_t)i * N, (unsigned long long)weights[t], [&](int m) { return (unsigned long long)h.size[m]; });
      }
    }
    return RL_OK;
  }
  int finish(long long *total_weight) {
    *total_weight = W;
    return dev ? pairwise_device_finish(dev, sum_out) : RL_OK;
  }
};

}  // namespace
}  // namespace rl

using namespace rl;

extern "C" int rl_pairwise_trees(const int *parents, const double *branch_length, const long long *weights, int N,
                                 int ntrees, int metric, int device, void *sum_out, long long *total_weight) {
  if (!parents || !weights || !sum_out || !total_weight || N < 2 || ntrees < 0) {
    set_error("rl_pairwise_trees: bad arguments (N=%d, ntrees=%d; N >= 2, no null pointers)", N, ntrees);
    return RL_EINVAL;
  }
  if (metric != RL_PAIRWISE_SIZE && metric != RL_PAIRWISE_TIME) {
    set_error("rl_pairwise_trees: metric %d is neither RL_PAIRWISE_SIZE nor RL_PAIRWISE_TIME", metric);
    return RL_EINVAL;
  }
  if (metric == RL_PAIRWISE_TIME && !branch_length) {
    set_error("rl_pairwise_trees: metric time needs branch lengths");
    return RL_EINVAL;
  }
  Pairwise pw;
  int rc = pw.begin(N, metric == RL_PAIRWISE_TIME, device, sum_out);
  rc = rc ? rc : pw.add(parents, branch_length, weights, ntrees, "rl_pairwise_trees");
  return rc ? rc : pw.finish(total_weight);
}

extern "C" int rl_pairwise_anc(const char *const *anc_paths, int npaths, int metric, int device, void *sum_out,
                               long long *total_weight, int *N_out) {
  if (!anc_paths || npaths < 1 || !N_out || (sum_out && !total_weight)) {
    set_error("rl_pairwise_anc: bad arguments (npaths=%d; at least one file, no null pointers)", npaths);
    return RL_EINVAL;
  }
  for (int f = 0; f < npaths; f++)
    if (!anc_paths[f]) {
      set_error("rl_pairwise_anc: path %d is null", f);
      return RL_EINVAL;
    }
  if (metric != RL_PAIRWISE_SIZE && metric != RL_PAIRWISE_TIME) {
    set_error("rl_pairwise_anc: metric %d is neither RL_PAIRWISE_SIZE nor RL_PAIRWISE_TIME", metric);
    return RL_EINVAL;
  }
  unsigned n0 = 0, trees0 = 0;
  bool ages0 = false;
  int rc = read_anc_header(anc_paths[0], &n0, &trees0, &ages0);
  if (rc) return rc;
  if (n0 < 2 || n0 > (1u << 30)) {
    set_error("PairwiseCoalescence: %s: %u haplotypes: no pair to take", anc_paths[0], n0);
    return RL_EINVAL;
  }
  const int N = (int)n0;
  *N_out = N;
  if (!sum_out) return RL_OK;
  const bool time = metric == RL_PAIRWISE_TIME;
  Pairwise pw;
  if ((rc = pw.begin(N, time, device, sum_out))) return rc;
  const size_t nodes = (size_t)2 * N - 1;
  std::vector<int> parents;
  std::vector<double> bl;
  std::vector<long long> weights;
  for (int f = 0; f < npaths; f++) {  // one file in memory at a time
    AncFile A;
    if ((rc = read_anc(anc_paths[f], A))) return rc;
    if ((int)A.N != N) {
      set_error("PairwiseCoalescence: %s holds trees on %d haplotypes, %s on %u", anc_paths[0], N, anc_paths[f], A.N);
      return RL_EINVAL;
    }
    if (time && A.has_ages) {
      set_error("PairwiseCoalescence: %s has sample ages: its leaves are not at height 0, metric time does not apply (metric size does)", anc_paths[f]);
      return RL_EINVAL;
    }
    int first_snp, last_snp;
    if ((rc = anc_coverage(A, anc_paths[f], &first_snp, &last_snp))) return rc;
    const size_t T = A.trees.size();
    parents.resize(T * nodes);
    weights.resize(T);
    if (time) bl.resize(T * nodes);
    for (size_t t = 0; t < T; t++) {
      memcpy(&parents[t * nodes], A.trees[t].parent.data(), nodes * sizeof(int));
      if (time) memcpy(&bl[t * nodes], A.trees[t].branch_length.data(), nodes * sizeof(double));
      weights[t] = (t + 1 < T ? A.trees[t + 1].pos : last_snp + 1) - (long long)A.trees[t].pos;
    }
    if ((rc = pw.add(parents.data(), time ? bl.data() : nullptr, weights.data(), (int)T, anc_paths[f]))) return rc;
  }
  return pw.finish(total_weight);
}
