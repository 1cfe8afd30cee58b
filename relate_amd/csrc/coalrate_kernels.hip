// coalrate_kernels.hip -- CoalescentRateForSection on the device: D[e][i][j], for every epoch e and pair of leaves,
// summed over the trees in order (include/relate_amd.h has the definition; coalrate.cpp is the same arithmetic on one
// host thread).  For i < j with m = MRCA(i,j), t = t(m) and es = the epoch t falls in (E-1: past the last boundary):
//   D[es][i][j] += factor                              the count            (es < E-1)
//   D[e][j][i]  += factor * (ep[e+1] - ep[e])          the opportunity, e < es
//   D[es][j][i] += factor * (t - ep[es])                                    (es < E-1)
// all floats, the product rounded before the sum.  Every element gets at most one addition per tree, so an element with
// ONE owner that takes the trees in order carries the bits of the reference's serial loop.
//
// coalrate_prepare_kernel, one workgroup per tree of a batch: the passes of tree_passes.h (kids with the validity
// checks, float times, clade sizes, left ends).  It leaves in global memory, per tree: rank[leaf], g[k] (the internal
// node that owns the boundary between the ranks k and k+1; pairwise_kernels.hip), tm[m] the float time and es[m] the
// epoch index of internal node m.  A tree that fails the checks, or has a branch length that is negative or not
// finite, sets its flag and nothing of its batch is used.
//
// coalrate_accumulate_kernel: the shape of pairwise_accumulate_kernel.  A workgroup owns a block of rows of D (in
// every plane) and takes the trees of the batch strictly in order; per row i it makes "MRCA with the leaf at rank q"
// by the prefix / suffix running maximum of g, then, column j by thread and coalesced per plane,
//   j > i: one read-modify-write at plane es (the count of the pair (i,j));
//   j < i: es + 1 read-modify-writes at the planes 0..es (the opportunity of the pair (j,i)), eight independent loads
//          in flight at a time; factor * width[e] is the same for the whole tree and lies in LDS.
// No atomics.  LDS, bytes: tm 4 N | g 2 N | rank 2 N | MRCA-at-rank 2 N | es N = 11 N: 113 KB at N = 10,240.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <vector>

#include "coalrate.h"
#include "common.h"
#include "tree_passes.h"

namespace rl {

constexpr int kCoalrateSmallN = 1024;  // up to here: one wavefront prepares a tree, 256 threads accumulate a row block

template <int T>
__global__ void __launch_bounds__(T) coalrate_prepare_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                             const float *__restrict__ EP, int E, int N, int ntrees,
                                                             u16 *__restrict__ RANK, u16 *__restrict__ G,
                                                             float *__restrict__ TM, unsigned char *__restrict__ ES,
                                                             int *__restrict__ BAD) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  __shared__ float ep[kCoalrateMaxEpochs];
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1;
  const int *par = PAR + (size_t)t * nodes;
  const double *bl = BL + (size_t)t * nodes;
  float *H = reinterpret_cast<float *>(lds);  // [ni] times, until the sizes and left ends take the room
  u16 *U = reinterpret_cast<u16 *>(lds);      // [ni] parent, then left end
  u16 *SZ = U + ni;                           // [ni] leaves of the clade
  unsigned *K = reinterpret_cast<unsigned *>(lds + (size_t)4 * ni);  // [ni] kids
  u16 *rank = RANK + (size_t)t * N, *g = G + (size_t)t * N;
  const int lane = threadIdx.x & 63;
  const bool wave0 = threadIdx.x < 64;

  if (threadIdx.x < E) ep[threadIdx.x] = EP[threadIdx.x];
  // (checked_kids of tree_passes.h written out: through the call this kernel's scalar register count comes out different)
  if (!build_kids<T>(par, N, K, nullptr, &bad)) {
    if (threadIdx.x == 0) BAD[t] = kTreeRefused;
    return;
  }
  __syncthreads();  // (every thread has read build_kids' verdict)
  for (int v = threadIdx.x; v < nodes - 1; v += T)
    if (!(bl[v] >= 0.0 && bl[v] <= DBL_MAX)) bad = 1;  // negative, infinite or NaN: the times would not rise
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) BAD[t] = kTreeRefused;
    return;
  }
  if (wave0) {
    float *tm = TM + (size_t)t * N;
    unsigned char *es = ES + (size_t)t * N;
    wave_float_times(K, bl, N, H, lane, [&](int i, float time) {
      int e = 0;
      while (e < E - 1 && !(time < ep[e + 1])) e++;  // the first epoch with t < ep[e+1]; E-1: none
      tm[i] = time;
      es[i] = (unsigned char)e;
    });
  }
  __syncthreads();
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
  for (int i = threadIdx.x; i < ni; i += T) g[U[i] + first_child_leaves(K, SZ, N, i) - 1u] = (u16)i;
}

// the product is rounded, then the sum: no fused multiply-add (the host does the same, coalrate.cpp)
__device__ inline float coalrate_term(float factor, float hi, float lo) {
#pragma clang fp contract(off)
  const float w = hi - lo;
  return factor * w;
}

template <int T>
__global__ void __launch_bounds__(T) coalrate_accumulate_kernel(const u16 *__restrict__ RANK, const u16 *__restrict__ G,
                                                                const float *__restrict__ TM,
                                                                const unsigned char *__restrict__ ES,
                                                                const float *__restrict__ F, const float *__restrict__ EP,
                                                                int E, int N, int ntrees, int rows_per_block,
                                                                float *__restrict__ D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ unsigned wave_right[T / 64], wave_left[T / 64];
  __shared__ float EP_L[kCoalrateMaxEpochs], FW[kCoalrateMaxEpochs];  // epochs; factor * width of every plane
  float *TM_L = reinterpret_cast<float *>(lds);                       // [N] time of internal node m (N-1 used)
  u16 *G_L = reinterpret_cast<u16 *>(TM_L + N);                       // [N] g (N-1 used)
  u16 *RANK_L = G_L + N;                                              // [N] rank of leaf j
  u16 *AT = RANK_L + N;                                               // [N] the row's MRCA with the leaf at rank q
  unsigned char *ES_L = reinterpret_cast<unsigned char *>(AT + N);    // [N] epoch index of internal node m
  const int ni = N - 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * rows_per_block, row1 = min(row0 + rows_per_block, N);
  const int run = (ni + T - 1) / T, p0 = min(tid * run, ni), p1 = min(p0 + run, ni);  // this thread's run of g
  const size_t plane = (size_t)N * N;

  if (tid < E) EP_L[tid] = EP[tid];
  for (int t = 0; t < ntrees; t++) {
    __syncthreads();  // the tree before is done with
    for (int k = tid; k < ni; k += T) {
      G_L[k] = G[(size_t)t * N + k];
      TM_L[k] = TM[(size_t)t * N + k];
      ES_L[k] = ES[(size_t)t * N + k];
    }
    for (int k = tid; k < N; k += T) RANK_L[k] = RANK[(size_t)t * N + k];
    const float f = F[t];
    if (tid < E - 1) FW[tid] = coalrate_term(f, EP_L[tid + 1], EP_L[tid]);
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
      float *row = D + (size_t)i * N;
      for (int jb = tid - lane; jb < N; jb += T) {  // (jb is the wavefront's: the ballot below sees all 64 lanes)
        const int j = jb + lane;
        const bool in = j < N && j != i;
        int e = 0;
        float tm = 0.0f;
        if (in) {
          const int m = AT[RANK_L[j]];
          e = ES_L[m];
          tm = TM_L[m];
        }
        if (in && j > i && e < E - 1) {  // the count of the pair (i, j)
          float *p = row + (size_t)e * plane + j;
          *p = *p + f;
        }
        // the opportunity of the pair (j, i): planes 0 .. last
        const bool low = in && j < i;
        const int last = low ? min(e, E - 2) : -1;
        const float own = low && e < E - 1 ? coalrate_term(f, tm, EP_L[e]) : 0.0f;
        for (int q0 = 0; q0 < E - 1; q0 += 8) {
          if (!__any(q0 <= last)) break;
          float s[8];
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (q0 + u <= last) s[u] = row[(size_t)(q0 + u) * plane + j];
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (q0 + u <= last) row[(size_t)(q0 + u) * plane + j] = s[u] + (q0 + u == e ? own : FW[q0 + u]);
        }
      }
      __syncthreads();  // AT and the waves' words are rewritten by the next row
    }
  }
}

struct CoalrateDevice {
  int N = 0, E = 0, device = 0;
  DevBuf D, ep, f, rank, g, tm, es;
  TreeBatch trees;
};

void coalrate_device_free(CoalrateDevice *d) { delete d; }

int coalrate_device_begin(CoalrateDevice **out, int N, const float *epochs, int E, int device) {
  *out = nullptr;
  if (N < 2 || N > kCoalrateMaxN) {
    set_error("rl_coalrate_trees: the device takes trees of 2 <= N <= %d leaves (N=%d); device < 0 selects the host", kCoalrateMaxN, N);
    return RL_EINVAL;
  }
  if (E < 2 || E > kCoalrateMaxEpochs) {
    set_error("rl_coalrate_trees: 2 <= epochs <= %d (%d given)", kCoalrateMaxEpochs, E);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_coalrate_trees", device)) return rc;
  const size_t nodes = (size_t)2 * N - 1, dbytes = (size_t)4 * E * N * N;
  const size_t B = (size_t)coalrate_batch_trees(N);
  const size_t staging = B * (nodes * 12 + (size_t)N * 9 + 8) + 256;
  size_t free_b = 0, total_b = 0;
  RL_HIP(hipMemGetInfo(&free_b, &total_b));
  if (dbytes + staging > free_b + device_cache_held(device, 0)) {
    set_error("rl_coalrate_trees: %d epochs x %d x %d floats and a batch of trees are %zu bytes, device %d has %zu free",
              E, N, N, dbytes + staging, device, free_b);
    return RL_ENOMEM;
  }
  CoalrateDevice *d = new CoalrateDevice;
  d->N = N;
  d->E = E;
  d->device = device;
  int rc = d->D.alloc(dbytes);
  rc = rc ? rc : d->ep.alloc((size_t)E * 4);
  rc = rc ? rc : d->trees.alloc(N, (int)B);
  rc = rc ? rc : d->f.alloc(B * 4);
  rc = rc ? rc : d->rank.alloc(B * N * 2);
  rc = rc ? rc : d->g.alloc(B * N * 2);
  rc = rc ? rc : d->tm.alloc(B * N * 4);
  rc = rc ? rc : d->es.alloc(B * N);
  if (rc) {
    delete d;
    return rc;
  }
  hipError_t e = hipMemset(d->D.p, 0, dbytes);
  if (e == hipSuccess) e = hipMemcpy(d->ep.p, epochs, (size_t)E * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete d;
    set_error("rl_coalrate_trees: %s", hipGetErrorString(e));
    return RL_EHIP;
  }
  *out = d;
  return RL_OK;
}

// the trees in order, batch by batch; SMALL: N <= kCoalrateSmallN
template <bool SMALL>
static int coalrate_add_batches(CoalrateDevice *d, const int *parents, const double *branch_length, const float *factors,
                                int ntrees, int *bad_tree) {
  const int N = d->N, E = d->E;
  TreeBatch &tb = d->trees;
  const size_t dyn_prepare = round16((size_t)8 * (N - 1)), dyn_accumulate = round16((size_t)11 * N);
  const int rows = (N + 511) / 512, blocks = (N + rows - 1) / rows;
  u16 *rank = d->rank.as<u16>(), *g = d->g.as<u16>();
  for (int t0 = 0; t0 < ntrees; t0 += tb.batch) {
    const int n = std::min(tb.batch, ntrees - t0);
    RL_HIP(hipMemcpy(d->f.p, factors + t0, (size_t)n * 4, hipMemcpyHostToDevice));
    if (const int rc = tb.upload(parents, branch_length, t0, n)) return rc;
    RL_HIP(launch_with_lds(coalrate_prepare_kernel<SMALL ? 64 : 256>, n, SMALL ? 64 : 256, dyn_prepare, nullptr, tb.par.as<int>(),
                           tb.bl.as<double>(), d->ep.as<float>(), E, N, n, rank, g, d->tm.as<float>(),
                           d->es.as<unsigned char>(), tb.flag.as<int>()));
    // Nothing of a batch is added unless all of its trees passed: the accumulation uses rank, g and the epoch indices
    // as indices
    int bad = -1;
    if (const int rc = tb.first_not_done(n, &bad)) return rc;
    if (bad >= 0) {
      *bad_tree = t0 + bad;
      return RL_EINVAL;
    }
    RL_HIP(launch_with_lds(coalrate_accumulate_kernel<SMALL ? 256 : 1024>, blocks, SMALL ? 256 : 1024, dyn_accumulate, nullptr, rank,
                           g, d->tm.as<float>(), d->es.as<unsigned char>(), d->f.as<float>(), d->ep.as<float>(), E, N, n,
                           rows, d->D.as<float>()));
    RL_HIP(hipDeviceSynchronize());  // the next batch overwrites the arrays this one reads
  }
  return RL_OK;
}

int coalrate_device_add(CoalrateDevice *d, const int *parents, const double *branch_length, const float *factors,
                        int ntrees, int *bad_tree) {
  *bad_tree = -1;
  RL_HIP(hipSetDevice(d->device));
  return d->N <= kCoalrateSmallN ? coalrate_add_batches<true>(d, parents, branch_length, factors, ntrees, bad_tree)
                                 : coalrate_add_batches<false>(d, parents, branch_length, factors, ntrees, bad_tree);
}

int coalrate_device_finish(CoalrateDevice *d, float *out) {
  RL_HIP(hipSetDevice(d->device));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(out, d->D.p, (size_t)4 * d->E * d->N * d->N, hipMemcpyDeviceToHost));
  return RL_OK;
}

}  // namespace rl
