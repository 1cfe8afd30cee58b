// subtrees_kernels.hip -- SubTreesForSubpopulation on the device: every tree of a batch pruned to the leaves of a
// subset, its unary chains contracted, its nodes renumbered and the result dated (include/relate_amd.h has the
// definition; subtrees.cpp restates the reference's Tree::GetSubTree and Tree::GetCoordinates on one host thread and
// is the authority this kernel is held to, bit for bit).
//
// The reference goes through the internal nodes in label order and, for a node with one child above a subset leaf,
// adds its branch length onto the subtree node that child converts to: one double chain per subtree node, added from
// the bottom up.  Here every chain has a thread.  subtrees_kernel, one workgroup per tree:
//   1. build_kids with its checks, then the branch-length check (all 2N-1: the root's length ends in the subtree
//      root's);
//   2. wavefront 0: number_in_subpop of the internal nodes, a rising pull scan (wave_pull) whose leaf value is
//      "is in the subset";
//   3. all threads: a node is KEPT when both children have subset leaves below them; an exclusive scan of the keep
//      flags in label order gives the new labels M + rank.  Kept nodes other than M - 1: refused;
//   4. all threads, one per node: a subset leaf or a kept node is the head of a chain -- it walks up while the
//      parent is not kept, adds the parents' double branch lengths in that order, writes convert_index of the nodes
//      it contracts and ends at a kept parent (the subtree's parent entry) or above the root (-1).  Every node lies
//      on one chain: O(N) per tree; a caterpillar with its two lowest leaves as the subset is one chain of N-2 steps
//      on one lane;
//   5. the times of Tree::GetCoordinates on the SUBTREE: build_kids and wave_max_times over the subtree's parents
//      and branch lengths, which this workgroup has just written, in the LDS that 1-4 have released.
// M = N needs no path of its own: every leaf is a head, every internal node is kept and M + rank is its own label.
// LDS: 8 bytes per internal node (kids 4, count 2, new label 2; then the subtree's kids 4 and times 4), 80 KB at
// N = 10,240; static: a flag and the scan's wavefront sums.  No scratch, no atomics on floating-point values, every
// sum a separate operation (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "subtrees.h"
#include "tree_passes.h"

namespace rl {

constexpr int kSubtreesSmallN = 2048;  // up to here a workgroup is 256 threads, above 1024
constexpr u16 kNotKept = 0xffffu;      // (a new label is at most 2 * 10,240 - 2)

// CNT[i] = subset leaves below internal node i; leaf [N]: the new label of a subset leaf, -1 for any other.  One
// wavefront calls it.
__device__ inline void wave_subset_counts(const unsigned *K, const int *__restrict__ leaf_label, int N, u16 *CNT, int lane) {
  const int ni = N - 1;
  const auto leaf = [&](int c) { return (unsigned)(leaf_label[c] >= 0); };
  const auto table = [&](int j) { return (unsigned)CNT[j]; };
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;
    unsigned s1 = 0, s2 = 0;
    if (act) {
      d1 = child_source(first_child(K, i), N, b, &s1, leaf, table);
      d2 = child_source(second_child(K, i), N, b, &s2, leaf, table);
    }
    const unsigned n = wave_pull<2>(act, d1, s1, d2, s2, [](unsigned a, unsigned c) { return a + c; });
    if (act) CNT[i] = (u16)n;
  }
}

template <int T>
__global__ void __launch_bounds__(T) subtrees_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                     const int *__restrict__ LEAF, int N, int M, int ntrees, int *SUBPAR,
                                                     double *SUBBL, float *__restrict__ SUBT, int *__restrict__ CONV,
                                                     int *__restrict__ COUNT, int *__restrict__ FLAG) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  __shared__ int wave_kept[T / 64];
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1, sub_nodes = 2 * M - 1, tid = threadIdx.x, lane = tid & 63;
  const int *par = PAR + (size_t)t * nodes;
  const double *bl = BL + (size_t)t * nodes;
  int *sub_parent = SUBPAR + (size_t)t * sub_nodes;
  double *sub_bl = SUBBL + (size_t)t * sub_nodes;
  float *sub_time = SUBT + (size_t)t * sub_nodes;
  int *conv = CONV + (size_t)t * nodes;
  int *count = COUNT + (size_t)t * nodes;
  unsigned *K = reinterpret_cast<unsigned *>(lds);           // [ni] kids
  u16 *CNT = reinterpret_cast<u16 *>(lds + (size_t)4 * ni);  // [ni] subset leaves below
  u16 *NL = CNT + ni;                                        // [ni] new label, kNotKept for a node that is not kept

  // ---- 1. the checks
  if (!checked_kids<T>(par, bl, nodes, N, K, nullptr, &bad)) {  // (the root's length ends in the subtree root's)
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }

  // ---- 2. number_in_subpop
  if ((tid >> 6) == 0) wave_subset_counts(K, LEAF, N, CNT, lane);
  __syncthreads();

  // ---- 3. keep flags and new labels: thread tid takes the nodes [a, b) of the label order
  const auto below = [&](int c) { return c < N ? (unsigned)(LEAF[c] >= 0) : (unsigned)CNT[c - N]; };
  const auto kept = [&](int i) { return below(first_child(K, i)) > 0 && below(second_child(K, i)) > 0; };
  const int chunk = (ni + T - 1) / T, a = min(tid * chunk, ni), b = min(a + chunk, ni);
  int mine = 0;
  for (int i = a; i < b; i++) mine += kept(i);
  int upto = mine;  // kept nodes of this wavefront's threads up to and including this one
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(upto, d, 64);
    if (lane >= d) upto += o;
  }
  if (lane == 63) wave_kept[tid >> 6] = upto;
  __syncthreads();
  int rank = upto - mine, total = 0;
  for (int w = 0; w < T / 64; w++) {
    if (w < (tid >> 6)) rank += wave_kept[w];
    total += wave_kept[w];
  }
  if (total != M - 1) {  // (the same verdict in every thread)
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }
  for (int i = a; i < b; i++) NL[i] = kept(i) ? (u16)(M + rank++) : kNotKept;
  __syncthreads();

  // ---- 4. one thread per node; the heads walk their chains
  for (int v = tid; v < nodes; v += T) {
    int s, c;
    if (v < N) {
      s = LEAF[v];
      c = s >= 0;
    } else {
      c = CNT[v - N];
      s = NL[v - N] == kNotKept ? -1 : (int)NL[v - N];
    }
    count[v] = c;
    if (s < 0) {
      if (v < N || c == 0) conv[v] = -1;  // (a contracted node is written by the head below it)
      continue;
    }
    conv[v] = s;
    double sum = bl[v];
    int p = par[v];
    while (p != -1 && NL[p - N] == kNotKept) {
      sum += bl[p];
      conv[p] = s;
      p = par[p];
    }
    sub_parent[s] = p == -1 ? -1 : (int)NL[p - N];
    sub_bl[s] = sum;
  }
  __syncthreads();  // the subtree's parents and branch lengths are written; K, CNT and NL are released

  // ---- 5. the subtree's times
  unsigned *K2 = reinterpret_cast<unsigned *>(lds);                  // [M-1] the subtree's kids
  float *TM = reinterpret_cast<float *>(lds + (size_t)4 * (M - 1));  // [M-1] its times
  if (!build_kids<T>(sub_parent, M, K2, nullptr, &bad)) {
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }
  __syncthreads();
  if ((tid >> 6) == 0) wave_max_times(K2, sub_bl, M, TM, lane);
  __syncthreads();
  for (int s = tid; s < sub_nodes; s += T) sub_time[s] = s < M ? 0.0f : TM[s - M];
}

int subtrees_device(const int *parents, const double *branch_length, int N, int ntrees, const int *leaf_label, int M,
                    int device, int *sub_parent, double *sub_bl, float *sub_time, int *convert_index,
                    int *number_in_subpop, int *bad_tree) {
  *bad_tree = -1;
  if (N < 2 || N > kSubtreesMaxN || M < 2 || M > N) {
    set_error("rl_subtrees_trees: trees of 2 <= N <= %d leaves and a subset of 2 <= M <= N (N=%d, M=%d)", kSubtreesMaxN, N, M);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_subtrees_trees", device)) return rc;
  const size_t nodes = (size_t)2 * N - 1, sub = (size_t)2 * M - 1, ni = (size_t)N - 1;
  const size_t B = (size_t)std::min(subtrees_batch_trees(N), std::max(ntrees, 1));
  const size_t dyn = round16((size_t)8 * ni);
  DevBuf leaf, spar, sbl, stm, conv, cnt;
  TreeBatch tb;
  int rc = tb.alloc(N, (int)B);
  rc = rc ? rc : leaf.alloc((size_t)N * 4);
  rc = rc ? rc : spar.alloc(B * sub * 4);
  rc = rc ? rc : sbl.alloc(B * sub * 8);
  rc = rc ? rc : stm.alloc(B * sub * 4);
  rc = rc ? rc : conv.alloc(B * nodes * 4);
  rc = rc ? rc : cnt.alloc(B * nodes * 4);
  if (rc) return rc;
  RL_HIP(hipMemcpy(leaf.p, leaf_label, (size_t)N * 4, hipMemcpyHostToDevice));
  for (int t0 = 0; t0 < ntrees; t0 += (int)B) {
    const int n = std::min((int)B, ntrees - t0);
    if ((rc = tb.upload(parents, branch_length, t0, n))) return rc;
    const auto go = [&](auto kernel, int threads) {
      return launch_with_lds(kernel, n, threads, dyn, nullptr, tb.par.as<int>(), tb.bl.as<double>(), leaf.as<int>(), N, M, n,
                             spar.as<int>(), sbl.as<double>(), stm.as<float>(), conv.as<int>(), cnt.as<int>(), tb.flag.as<int>());
    };
    RL_HIP(N <= kSubtreesSmallN ? go(subtrees_kernel<256>, 256) : go(subtrees_kernel<1024>, 1024));
    int bad = -1;
    if ((rc = tb.first_not_done(n, &bad))) return rc;
    if (bad >= 0) {
      *bad_tree = t0 + bad;
      return RL_EINVAL;
    }
    RL_HIP(hipMemcpy(sub_parent + (size_t)t0 * sub, spar.p, (size_t)n * sub * 4, hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(sub_bl + (size_t)t0 * sub, sbl.p, (size_t)n * sub * 8, hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(sub_time + (size_t)t0 * sub, stm.p, (size_t)n * sub * 4, hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(convert_index + (size_t)t0 * nodes, conv.p, (size_t)n * nodes * 4, hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(number_in_subpop + (size_t)t0 * nodes, cnt.p, (size_t)n * nodes * 4, hipMemcpyDeviceToHost));
  }
  return RL_OK;
}

}  // namespace rl
