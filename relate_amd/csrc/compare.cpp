// compare.cpp -- CompareTopology: the clade (rooted Robinson-Foulds) distance between trees, host side.
//
// The definition (include/relate_amd.h): the clades of a tree on the leaves 0..N-1 are the leaf sets of its internal
// nodes other than the root, d(A,B) = |clades(A) \ clades(B)| + |clades(B) \ clades(A)|.  Both trees are binary, so
// each has N-2 distinct clades and d = 2 (N - 2 - common).
//
// `common` by Day's algorithm (W.H.E. Day 1985, "Optimal algorithms for comparing trees with labeled leaves"), in
// integers, no hashing:
//   - the leaves are ranked in the order a depth-first walk of A meets them: a clade of A is an interval [l, r] of
//     ranks.  Node labels rise from child to parent, so one pass over the nodes in label order sums the clade sizes
//     and one pass in falling order hands every node the left end of its interval;
//   - A's intervals go into ONE table of N entries: a first child shares l with its parent and is stored at index r,
//     a second child shares r and is stored at index l (two first children with the same r, or two second children
//     with the same l, would be the same clade; a first child stored at i and a second stored at i share only leaf i
//     and cannot both have two leaves or more);
//   - a node of B gets (size, min rank, max rank) of its leaves in one pass in label order; its clade is a clade of
//     A iff max - min + 1 == size and the table holds (min, max) at min or at max.
// This file is the plain C++ implementation (the CPU suite's, and the one used when no device is asked for), the
// comparison of two .anc files on top of either implementation, and the C entry points; the device implementation is
// compare_kernels.hip.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "anc_file.h"
#include "common.h"
#include "tree_host.h"

namespace rl {

int compare_trees_device(const int *parentsA, int treesA, const int *parentsB, int treesB, int N, int npairs,
                         const int *pairs, int device, int *out);  // compare_kernels.hip

static int refuse_side(const char *which, int index, const int *parent, int N) {
  char tree[64];
  snprintf(tree, sizeof tree, "rl_compare_trees: tree %d of %s", index, which);
  return refuse_tree(tree, parent, N);
}

// Day's algorithm for one tree A against any number of trees B
struct HostComparer : TreeTables {
  std::vector<int> table, sz, mn, mx;
  explicit HostComparer(int n) : TreeTables(n), table(n), sz(nodes), mn(nodes), mx(nodes) {}

  // ranks and the interval table of A; parent must have passed first_bad_node
  void set_reference(const int *parent) {
    fill(parent);
    std::fill(table.begin(), table.end(), -1);
    for (int p = N; p < nodes; p++) {
      const int a = first[p], b = second[p];
      if (a >= N) table[lo[a] + size[a] - 1] = lo[a];       // first child, stored at r: holds l
      if (b >= N) table[lo[b]] = lo[b] + size[b] - 1;       // second child, stored at l: holds r
    }
  }
  // leaves of A are ranked lo[leaf]
  int distance(const int *parent) {
    for (int v = 0; v < nodes; v++) {
      sz[v] = v < N ? 1 : 0;
      mn[v] = v < N ? lo[v] : N;
      mx[v] = v < N ? lo[v] : -1;
    }
    int common = 0;
    for (int v = 0; v < nodes - 1; v++) {
      if (v >= N) {
        const int l = mn[v], r = mx[v];
        if (r - l + 1 == sz[v] && (table[l] == r || table[r] == l)) common++;
      }
      const int p = parent[v];
      sz[p] += sz[v];
      mn[p] = std::min(mn[p], mn[v]);
      mx[p] = std::max(mx[p], mx[v]);
    }
    return 2 * (N - 2 - common);
  }
};

static int compare_trees_host(const int *parentsA, const int *parentsB, int N, int npairs, const int *pairs, int *out) {
  const size_t nodes = (size_t)2 * N - 1;
  HostComparer hc(N);
  int held = -1;  // the tree of A the table was built from
  for (int k = 0; k < npairs; k++) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    const int *pa = parentsA + (size_t)a * nodes, *pb = parentsB + (size_t)b * nodes;
    if (a != held) {
      if (first_bad_node(pa, N, hc.kids)) return refuse_side("A", a, pa, N);
      hc.set_reference(pa);
      held = a;
    }
    if (first_bad_node(pb, N, hc.kids)) return refuse_side("B", b, pb, N);
    out[k] = hc.distance(pb);
  }
  return RL_OK;
}

}  // namespace rl

using namespace rl;

extern "C" int rl_compare_trees(const int *parentsA, const int *parentsB, int N, int npairs, const int *pairs,
                                int device, int *out) {
  if (!parentsA || !parentsB || !pairs || !out || N < 2 || npairs < 0) {
    set_error("rl_compare_trees: bad arguments (N=%d, npairs=%d; N >= 2, no null pointers)", N, npairs);
    return RL_EINVAL;
  }
  int treesA = 0, treesB = 0;
  for (int k = 0; k < npairs; k++) {
    if (pairs[2 * k] < 0 || pairs[2 * k + 1] < 0) {
      set_error("rl_compare_trees: pair %d names a negative tree index", k);
      return RL_EINVAL;
    }
    treesA = std::max(treesA, pairs[2 * k] + 1);
    treesB = std::max(treesB, pairs[2 * k + 1] + 1);
  }
  if (npairs == 0) return RL_OK;
  if (device < 0) return compare_trees_host(parentsA, parentsB, N, npairs, pairs, out);
  const int rc = compare_trees_device(parentsA, treesA, parentsB, treesB, N, npairs, pairs, device, out);
  if (rc != RL_OK) return rc;
  for (int k = 0; k < npairs; k++)  // the kernel marks a pair whose tree it refused: -1 tree A, -2 tree B
    if (out[k] < 0) {
      const bool isA = out[k] == -1;
      const int t = pairs[2 * k + (isA ? 0 : 1)];
      return refuse_side(isA ? "A" : "B", t, (isA ? parentsA : parentsB) + (size_t)t * ((size_t)2 * N - 1), N);
    }
  return RL_OK;
}

extern "C" int rl_compare_anc(const char *ancA, const char *ancB, int device, rl_compare_summary *summary,
                              const char *per_interval_path) {
  if (!ancA || !ancB || !summary) {
    set_error("rl_compare_anc: null argument");
    return RL_EINVAL;
  }
  memset(summary, 0, sizeof *summary);
  AncFile A, B;
  int rc = read_anc(ancA, A);
  rc = rc ? rc : read_anc(ancB, B);
  if (rc) return rc;
  if (A.N != B.N) {
    set_error("CompareTopology: %s holds trees on %u haplotypes, %s on %u", ancA, A.N, ancB, B.N);
    return RL_EINVAL;
  }
  if (A.N < 2) {
    set_error("CompareTopology: %u haplotypes: nothing to compare", A.N);
    return RL_EINVAL;
  }
  const int N = (int)A.N;
  int a0, a1, b0, b1;
  if ((rc = anc_coverage(A, ancA, &a0, &a1)) || (rc = anc_coverage(B, ancB, &b0, &b1))) return rc;
  const int begin = std::max(a0, b0), end = std::min(a1, b1) + 1;  // [begin, end)
  if (begin >= end) {
    set_error("CompareTopology: the SNP ranges do not overlap: %s covers %d..%d, %s covers %d..%d", ancA, a0, a1, ancB, b0, b1);
    return RL_EINVAL;
  }
  // the merge of the two files' tree positions over [begin, end)
  struct Interval {
    int b, e, ta, tb;
  };
  std::vector<Interval> iv;
  {
    size_t ta = 0, tb = 0;
    while (ta + 1 < A.trees.size() && A.trees[ta + 1].pos <= begin) ta++;
    while (tb + 1 < B.trees.size() && B.trees[tb + 1].pos <= begin) tb++;
    int at = begin;
    while (at < end) {
      const int na = ta + 1 < A.trees.size() ? A.trees[ta + 1].pos : end;
      const int nb = tb + 1 < B.trees.size() ? B.trees[tb + 1].pos : end;
      const int next = std::min({na, nb, end});
      iv.push_back(Interval{at, next, (int)ta, (int)tb});
      if (na == next) ta++;
      if (nb == next) tb++;
      at = next;
    }
  }
  std::vector<int> pa, pb, pairs(iv.size() * 2), d(iv.size());
  flatten_anc(A, pa);
  flatten_anc(B, pb);
  for (size_t k = 0; k < iv.size(); k++) {
    pairs[2 * k] = iv[k].ta;
    pairs[2 * k + 1] = iv[k].tb;
  }
  if ((rc = rl_compare_trees(pa.data(), pb.data(), N, (int)iv.size(), pairs.data(), device, d.data()))) return rc;
  summary->N = N;
  summary->trees_a = (int)A.trees.size();
  summary->trees_b = (int)B.trees.size();
  summary->intervals = (int)iv.size();
  summary->snp_begin = begin;
  summary->snp_end = end;
  const double full = 2.0 * (N - 2), snps = (double)(end - begin);
  double weighted = 0.0;
  for (size_t k = 0; k < iv.size(); k++) {  // interval order, double
    const int len = iv[k].e - iv[k].b;
    if (N > 2) weighted += (double)len * ((double)d[k] / full);
    summary->max_distance = std::max(summary->max_distance, d[k]);
    if (d[k] == 0) summary->snps_identical += len;
  }
  summary->mean_normalised = weighted / snps;
  summary->share_identical = (double)summary->snps_identical / snps;
  if (per_interval_path) {
    FILE *fp = fopen(per_interval_path, "w");
    if (!fp) {
      set_error("cannot open %s for writing", per_interval_path);
      return RL_EIO;
    }
    for (size_t k = 0; k < iv.size(); k++) fprintf(fp, "%d %d %d %d %d\n", iv[k].b, iv[k].e, iv[k].ta, iv[k].tb, d[k]);
    const bool bad = ferror(fp) != 0;
    if (fclose(fp) != 0 || bad) {
      set_error("writing %s failed", per_interval_path);
      return RL_EIO;
    }
  }
  return RL_OK;
}
