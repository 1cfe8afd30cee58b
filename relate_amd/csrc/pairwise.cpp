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
#include "tree_host.h"

namespace rl {

namespace {

// check_tree of tree `index` of `where`; the branch lengths are not checked: any double is added
int check_at(const char *where, long long index, const int *parent, int N, bool refused_by_device, std::vector<unsigned char> &kids) {
  return check_tree((std::string(where) + ": tree " + std::to_string(index)).c_str(), parent, nullptr, N, 0, refused_by_device, kids);
}

// one tree's tables and its contribution to S
struct HostPairwise : TreeTables {
  std::vector<int> order, g;
  std::vector<double> height;
  explicit HostPairwise(int n) : TreeTables(n), order(n), g(n), height(nodes) {}

  // parent must have passed first_bad_node
  void prepare(const int *parent, const double *bl) {
    fill(parent);
    if (bl) {
      for (int v = 0; v < N; v++) height[v] = 0.0;
      for (int n = N; n < nodes; n++) height[n] = height[first[n]] + bl[first[n]];  // one addition per node
    }
    for (int p = N; p < nodes; p++) g[lo[second[p]] - 1] = p;
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
      std::vector<unsigned char> kids;
      return bad >= 0 ? check_at(where, bad, parents + (size_t)bad * nodes, N, true, kids) : rc;
    }
    for (int t = 0; t < ntrees; t++) {
      const int *parent = parents + t * nodes;
      if (const int rc = check_at(where, t, parent, N, false, host->kids)) return rc;
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
    flatten_anc(A, parents, time ? &bl : nullptr);
    weights.resize(T);
    for (size_t t = 0; t < T; t++) weights[t] = (t + 1 < T ? A.trees[t + 1].pos : last_snp + 1) - (long long)A.trees[t].pos;
    if ((rc = pw.add(parents.data(), time ? bl.data() : nullptr, weights.data(), (int)T, anc_paths[f]))) return rc;
  }
  return pw.finish(total_weight);
}
