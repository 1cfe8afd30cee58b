// pairwise_kernels.hip -- PairwiseCoalescence on the device: S(i,j) = sum over trees of w_t * v_t(i,j), v the size
// (leaves below) or the height of the most recent common ancestor of the leaves i and j (include/relate_amd.h has
// the definitions; pairwise.cpp is the same arithmetic on one host thread).
//
// pairwise_prepare_kernel, one workgroup per tree of a batch: the passes of tree_passes.h (kids with the validity
// checks, clade sizes, left ends of the intervals of depth-first ranks) and, for `time`, the heights by the same
// pull-by-shuffle scheme with the first child as the one dependency (one double addition per node).  It leaves in
// global memory, per tree:
//   rank[leaf]  the leaf's depth-first rank;
//   g[k]        k = 0..N-2: the MRCA of the leaves at ranks k and k+1 (internal numbering, label - N).  Every internal
//               node m owns exactly one such boundary, k = left end(m) + size(first child of m) - 1;
//   val[m]      size (u16) or height (double) of internal node m.
// A tree that fails the checks sets its flag and nothing of it is used.
//
// pairwise_accumulate_kernel: labels rise towards the root, so MRCA(i,j) is the LARGEST label among
// g[min(r_i,r_j) .. max(r_i,r_j)-1]: for a row i, the MRCA with the leaf at every other rank is a running maximum
// of g outwards from rank[i], to the right and to the left -- no tree is walked, a caterpillar costs what a balanced
// tree costs.  A workgroup owns a block of rows of S and takes the trees of the batch strictly in order; per tree it
// loads g, rank and val into LDS once, then per row
//   - scans: every thread takes a run of g, the maxima of the runs go through a prefix maximum (rightwards part) and
//     a suffix maximum (leftwards part) over the workgroup -- wave shuffles, one LDS word per wave between them --
//     and the thread rewrites its run as MRCA-at-rank into LDS;
//   - adds, column j by thread: S[i][j] += w * val[mrca_at_rank[rank[j]]], the row read and written coalesced.
// Every element of S has one owner and one fixed sequence of operations: no atomics, and the double sums come out
// the same on every run and equal to the host's.  All workgroups meet the trees in the same order, so a tree's
// arrays (12 N bytes) are read from L2.
//
// LDS of the accumulation, bytes: val 8 N (2 N for size) | g 2 N | rank 2 N | MRCA-at-rank 2 N = 14 N: 140 KB at
// N = 10,000.  Labels, ranks and sizes are 16-bit: N <= 10,240.  DESIGN.md 8d has the resource table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "pairwise.h"
#include "tree_batch.h"
#include "tree_passes.h"

namespace rl {

constexpr int kPairwiseMaxN = 10240;
constexpr int kPairwiseSmallN = 1024;  // up to here: one wavefront prepares a tree, 256 threads accumulate a row block
// a batch of trees is what fits this many bytes of tree arrays (parents, branch lengths, rank, g, val) -- or half
// of what the device has free next to S, if that is less.  One tree's accumulation moves 16 N^2 bytes (1.6 GB at
// N = 10,000), so a batch of a few trees already hides its launches and copies.
constexpr size_t kPairwiseBatchBytes = (size_t)2 << 20;

template <int T, bool TIME>
__global__ void __launch_bounds__(T) pairwise_prepare_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                             int N, int ntrees, u16 *__restrict__ RANK,
                                                             u16 *__restrict__ G, void *__restrict__ VAL,
                                                             int *__restrict__ BAD) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1;
  const int *par = PAR + (size_t)t * nodes;
  double *H = reinterpret_cast<double *>(lds);  // [ni] TIME: heights, until the sizes and left ends take the room
  u16 *U = reinterpret_cast<u16 *>(lds);        // [ni] parent, then left end
  u16 *SZ = U + ni;                             // [ni] leaves of the clade
  unsigned *K = reinterpret_cast<unsigned *>(lds + (size_t)(TIME ? 8 : 4) * ni);  // [ni] kids
  u16 *rank = RANK + (size_t)t * N, *g = G + (size_t)t * N;
  const int lane = threadIdx.x & 63;
  const bool wave0 = threadIdx.x < 64;

  if (!build_kids<T>(par, N, K, nullptr, &bad)) {  // (the branch lengths are not checked: any double is added)
    if (threadIdx.x == 0) BAD[t] = kTreeRefused;
    return;
  }
  if (TIME) {
    // height(n) = height(first child) + branch_length[first child], label order, wave 0
    if (wave0) {
      const double *bl = BL + (size_t)t * nodes;
      double *val = reinterpret_cast<double *>(VAL) + (size_t)t * N;
      const auto leaf = [](int) { return 0.0; };
      const auto table = [&](int j) { return H[j]; };
      for (int b = 0; b < ni; b += 64) {
        const int i = b + lane;
        const bool act = i < ni;
        int dep = -1;
        double base = 0.0, len = 0.0;
        if (act) {
          const int c1 = first_child(K, i);
          len = bl[c1];
          dep = child_source(c1, N, b, &base, leaf, table);
        }
        const double h = wave_pull(act, dep, base, [len](double below) { return below + len; });
        if (act) {
          H[i] = h;
          val[i] = h;
        }
      }
    }
    __syncthreads();
  }
  for (int v = N + threadIdx.x; v < nodes - 1; v += T) U[v - N] = (u16)(par[v] - N);
  __syncthreads();
  if (wave0) {
    wave_clade_sizes(K, N, SZ, lane);
    wave_left_ends(K, SZ, U, N, lane, [](int, unsigned, bool, bool) {});
  }
  __syncthreads();
  for (int v = threadIdx.x; v < N; v += T) {
    const int pi = par[v] - N;
    rank[v] = (u16)leaf_rank(K, SZ, N, v, pi, U[pi]);
  }
  for (int i = threadIdx.x; i < ni; i += T) {
    g[U[i] + first_child_leaves(K, SZ, N, i) - 1u] = (u16)i;
    if (!TIME) reinterpret_cast<u16 *>(VAL)[(size_t)t * N + i] = SZ[i];
  }
}

__device__ inline unsigned long long pairwise_add(unsigned long long s, unsigned long long w, u16 v) { return s + w * v; }
// the product is rounded, then the sum: no fused multiply-add (the host does the same, pairwise.cpp)
__device__ inline double pairwise_add(double s, double w, double v) {
#pragma clang fp contract(off)
  const double p = w * v;
  return s + p;
}

template <int T, bool TIME>
__global__ void __launch_bounds__(T) pairwise_accumulate_kernel(const u16 *__restrict__ RANK, const u16 *__restrict__ G,
                                                                const void *__restrict__ VAL,
                                                                const long long *__restrict__ W, int N, int ntrees,
                                                                int rows_per_block, void *__restrict__ S_) {
  typedef typename std::conditional<TIME, double, u16>::type val_t;
  typedef typename std::conditional<TIME, double, unsigned long long>::type sum_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ unsigned wave_right[T / 64], wave_left[T / 64];
  val_t *VAL_L = reinterpret_cast<val_t *>(lds);         // [N] size or height of internal node m (N-1 used)
  u16 *G_L = reinterpret_cast<u16 *>(VAL_L + N);         // [N] g (N-1 used)
  u16 *RANK_L = G_L + N;                                 // [N] rank of leaf j
  u16 *AT = RANK_L + N;                                  // [N] the row's MRCA with the leaf at rank q
  sum_t *S = reinterpret_cast<sum_t *>(S_);
  const int ni = N - 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * rows_per_block, row1 = min(row0 + rows_per_block, N);
  const int run = (ni + T - 1) / T, p0 = min(tid * run, ni), p1 = min(p0 + run, ni);  // this thread's run of g

  for (int t = 0; t < ntrees; t++) {
    __syncthreads();  // the tree before is done with
    for (int k = tid; k < ni; k += T) {
      G_L[k] = G[(size_t)t * N + k];
      VAL_L[k] = reinterpret_cast<const val_t *>(VAL)[(size_t)t * N + k];
    }
    for (int k = tid; k < N; k += T) RANK_L[k] = RANK[(size_t)t * N + k];
    const sum_t w = (sum_t)W[t];
    __syncthreads();
    for (int i = row0; i < row1; i++) {
      const int r = RANK_L[i];
      // right of r: AT[p + 1] = max g[r..p]; left of r: AT[p] = max g[p..r-1]
      unsigned a = 0, b = 0;  // (0 is below or equal to every label: the identity)
      for (int p = p0; p < p1; p++) {
        const unsigned x = G_L[p];
        if (p >= r) a = max(a, x);
        else b = max(b, x);
      }
      unsigned ia = a, ib = b;  // inclusive prefix / suffix maxima over the wave
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned ya = __shfl_up(ia, o, 64), yb = __shfl_down(ib, o, 64);
        if (lane >= o) ia = max(ia, ya);
        if (lane + o < 64) ib = max(ib, yb);
      }
      if (lane == 63) wave_right[wave] = ia;
      if (lane == 0) wave_left[wave] = ib;
      unsigned before = __shfl_up(ia, 1, 64), after = __shfl_down(ib, 1, 64);
      if (lane == 0) before = 0;
      if (lane == 63) after = 0;
      __syncthreads();
      for (int k = 0; k < wave; k++) before = max(before, wave_right[k]);
      for (int k = wave + 1; k < T / 64; k++) after = max(after, wave_left[k]);
      for (int p = max(p0, r); p < p1; p++) {
        before = max(before, (unsigned)G_L[p]);
        AT[p + 1] = (u16)before;
      }
      for (int p = min(p1, r) - 1; p >= p0; p--) {
        after = max(after, (unsigned)G_L[p]);
        AT[p] = (u16)after;
      }
      if (tid == 0) AT[r] = 0;  // (the diagonal: looked up, never added)
      __syncthreads();
      sum_t *row = S + (size_t)i * N;
      for (int j0 = tid; j0 < N; j0 += 4 * T) {
        sum_t s[4];
        val_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int j = j0 + u * T;
          if (j < N) {
            s[u] = row[j];
            v[u] = VAL_L[AT[RANK_L[j]]];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int j = j0 + u * T;
          if (j < N && j != i) row[j] = pairwise_add(s[u], w, v[u]);
        }
      }
      __syncthreads();  // AT and the waves' words are rewritten by the next row
    }
  }
}

struct PairwiseDevice {
  int N = 0, device = 0;
  bool time = false;
  DevBuf S, w, rank, g, val;
  TreeBatch trees;  // (branch lengths only for metric time)
};

void pairwise_device_free(PairwiseDevice *d) { delete d; }

int pairwise_device_begin(PairwiseDevice **out, int N, bool time, int device) {
  *out = nullptr;
  if (N < 2 || N > kPairwiseMaxN) {
    set_error("rl_pairwise_trees: the device takes trees of 2 <= N <= %d leaves (N=%d); device < 0 selects the host", kPairwiseMaxN, N);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_pairwise_trees", device)) return rc;
  PairwiseDevice *d = new PairwiseDevice;
  d->N = N;
  d->device = device;
  d->time = time;
  const size_t sbytes = (size_t)N * N * 8;
  int rc = d->S.alloc(sbytes);
  if (rc) {
    delete d;
    return rc;
  }
  hipError_t e = hipMemset(d->S.p, 0, sbytes);
  size_t free_b = 0, total_b = 0;
  if (e == hipSuccess) e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) {
    delete d;
    set_error("rl_pairwise_trees: %s", hipGetErrorString(e));
    return RL_EHIP;
  }
  const size_t nodes = (size_t)2 * N - 1;
  const size_t per_tree = nodes * 4 + (time ? nodes * 8 : 0) + 8 + (size_t)N * (2 + 2 + (time ? 8 : 2)) + 4;
  // (a tree of 10,240 leaves is 0.4 MB: the allocations below say so if it does not fit)
  const size_t B = (size_t)batch_trees(std::min(kPairwiseBatchBytes, free_b / 2), per_tree);
  rc = d->trees.alloc(N, (int)B, time);
  rc = rc ? rc : d->w.alloc(B * 8);
  rc = rc ? rc : d->rank.alloc(B * N * 2);
  rc = rc ? rc : d->g.alloc(B * N * 2);
  rc = rc ? rc : d->val.alloc(B * N * (time ? 8 : 2));
  if (rc) {
    delete d;
    return rc;
  }
  *out = d;
  return RL_OK;
}

// the trees in order, batch by batch; SMALL: N <= kPairwiseSmallN
template <bool TIME, bool SMALL>
static int pairwise_add_batches(PairwiseDevice *d, const int *parents, const double *branch_length,
                                const long long *weights, int ntrees, int *bad_tree) {
  const int N = d->N;
  TreeBatch &tb = d->trees;
  const size_t dyn_prepare = round16((size_t)(TIME ? 12 : 8) * (N - 1)), dyn_accumulate = round16((size_t)(TIME ? 14 : 8) * N);
  const int rows = (N + 511) / 512, blocks = (N + rows - 1) / rows;
  u16 *rank = d->rank.as<u16>(), *g = d->g.as<u16>();
  for (int t0 = 0; t0 < ntrees; t0 += tb.batch) {
    const int n = std::min(tb.batch, ntrees - t0);
    RL_HIP(hipMemcpy(d->w.p, weights + t0, (size_t)n * 8, hipMemcpyHostToDevice));
    if (const int rc = tb.upload(parents, TIME ? branch_length : nullptr, t0, n)) return rc;
    RL_HIP(launch_with_lds(pairwise_prepare_kernel<SMALL ? 64 : 256, TIME>, n, SMALL ? 64 : 256, dyn_prepare, nullptr, tb.par.as<int>(),
                           TIME ? tb.bl.as<double>() : nullptr, N, n, rank, g, d->val.p, tb.flag.as<int>()));
    // Nothing of a batch is added unless all of its trees passed: the accumulation uses rank and g as indices
    int bad = -1;
    if (const int rc = tb.first_not_done(n, &bad)) return rc;
    if (bad >= 0) {
      *bad_tree = t0 + bad;
      return RL_EINVAL;
    }
    RL_HIP(launch_with_lds(pairwise_accumulate_kernel<SMALL ? 256 : 1024, TIME>, blocks, SMALL ? 256 : 1024, dyn_accumulate, nullptr, rank,
                           g, d->val.p, d->w.as<long long>(), N, n, rows, d->S.p));
    RL_HIP(hipDeviceSynchronize());  // the next batch overwrites the arrays this one reads
  }
  return RL_OK;
}

// *bad_tree: -1, or the first tree the device refused (RL_EINVAL; the caller words the message)
int pairwise_device_add(PairwiseDevice *d, const int *parents, const double *branch_length, const long long *weights,
                        int ntrees, int *bad_tree) {
  *bad_tree = -1;
  RL_HIP(hipSetDevice(d->device));
  const bool small = d->N <= kPairwiseSmallN;
  if (d->time) return small ? pairwise_add_batches<true, true>(d, parents, branch_length, weights, ntrees, bad_tree)
                            : pairwise_add_batches<true, false>(d, parents, branch_length, weights, ntrees, bad_tree);
  return small ? pairwise_add_batches<false, true>(d, parents, branch_length, weights, ntrees, bad_tree)
               : pairwise_add_batches<false, false>(d, parents, branch_length, weights, ntrees, bad_tree);
}

int pairwise_device_finish(PairwiseDevice *d, void *sum_out) {
  RL_HIP(hipSetDevice(d->device));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(sum_out, d->S.p, (size_t)d->N * d->N * 8, hipMemcpyDeviceToHost));
  return RL_OK;
}

}  // namespace rl
