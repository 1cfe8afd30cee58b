// copying_kernels.hip -- CopyingMatrix on the device: the posterior rows a window holds in HBM, reduced into the
// targets' rows of the coancestry matrix C (include/relate_amd.h has the definition, copying.cpp the host twin).
//
// One workgroup of 256 threads per target.  Thread t owns the columns j = t, t + 256, ... of the target's row of C:
// K double accumulators in registers, loaded from C when the workgroup starts, stored when it has been through the
// target's rows -- every element of C has one owner, no atomics, and the order of the additions is the order of the
// rows.  Per posterior row p with a weight other than zero:
//   1. the row is read from HBM once, in the order it lies there ([wave][register][lane]: 256 B per wavefront and
//      load), and put down in LDS in DONOR order (a word of padding per 32: lane l's run starts at l * q + min(l, rem),
//      so the stores of a wavefront are q words apart, and q is even as often as not);
//   2. thread t takes its K columns from LDS into registers and adds them up in double, k ascending: the 256 partial
//      sums of the definition.  Halving: h = 128 and 64 by the first wavefront out of LDS, h = 32 .. 1 by lane
//      shuffles -- the same tree, x[t] += x[t + h];
//   3. lane 0 divides, c_p = Wt[p] / Z_p, everybody reads it and adds c_p * x to the accumulators, the product rounded,
//      then the sum.
// Three barriers per row.  The padding registers of the layout (register >= len_l) are never read past the last one a
// lane can own.
#include <hip/hip_runtime.h>

#include "copying.h"

namespace rl {

namespace {

constexpr int CP_THREADS = 256;

__device__ __forceinline__ int lds_slot(int j) { return j + (j >> 5); }

template <int K>
__global__ __launch_bounds__(CP_THREADS) void copying_reduce_kernel(CopyingParams p) {
#pragma clang fp contract(off)
  __shared__ float row[K * 256 + K * 8];
  __shared__ double red[CP_THREADS];
  __shared__ double c_bc;
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lo = p.row_lo[t], hi = p.row_hi[t];
  if (lo >= hi) return;
  const int N = p.N, S = p.S, q = p.lay.q, rem = p.lay.rem;
  const int need = q + (rem > 0 ? 1 : 0);  // registers a lane can own
  const int64_t stride = (int64_t)S * 64 * p.waves;
  const double *wt = p.weights + p.top_off[t];
  const float *rows = p.topology + p.slab_base[t] * stride;
  double *crow = p.C + (int64_t)t * N;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int j = tid + 256 * k;
    acc[k] = j < N ? crow[j] : 0.0;
  }
  int bad = 0;
  for (int r = lo; r < hi; r++) {
    const double w = wt[r];
    if (w == 0.0) continue;  // (the same for every thread)
    const float *src = rows + (int64_t)r * stride;
    for (int g = wq; g < p.waves * S; g += CP_THREADS / 64) {
      const int wv = g / S, i = g - wv * S;
      if (i >= need) continue;
      const int vl = wv * 64 + lane;
      const float v = src[(int64_t)g * 64 + lane];
      if (i < q + (vl < rem ? 1 : 0)) row[lds_slot(vl * q + min(vl, rem) + i)] = v;
    }
    __syncthreads();
    float x[K];
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int j = tid + 256 * k;
      x[k] = 0.f;
      if (j < N) {
        x[k] = row[lds_slot(j)];
        part += (double)x[k];
      }
    }
    red[tid] = part;
    __syncthreads();
    if (tid < 64) {
      double s = (red[tid] + red[tid + 128]) + (red[tid + 64] + red[tid + 192]);
#pragma unroll
      for (int h = 32; h >= 1; h >>= 1) s += __shfl_down(s, h);
      if (tid == 0) {
        const bool ok = s > 0.0 && s < __builtin_huge_val();
        c_bc = ok ? w / s : 0.0;
        if (!ok && !bad) bad = r + 1;
      }
    }
    __syncthreads();
    const double c = c_bc;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const double prod = c * (double)x[k];
      acc[k] = acc[k] + prod;
    }
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int j = tid + 256 * k;
    if (j < N) crow[j] = acc[k];
  }
  if (tid == 0 && bad) p.bad_row[t] = bad;
}

}  // namespace

hipError_t launch_copying(const CopyingParams &p, hipStream_t stream) {
  if (p.nloc <= 0) return hipSuccess;
  const int need = (p.N + 255) / 256;
#define RL_CP(KK)                                                                                 \
  if (need <= KK) {                                                                               \
    hipLaunchKernelGGL(copying_reduce_kernel<KK>, dim3(p.nloc), dim3(CP_THREADS), 0, stream, p);  \
    return hipGetLastError();                                                                     \
  }
  RL_CP(1) RL_CP(2) RL_CP(4) RL_CP(8) RL_CP(12) RL_CP(16) RL_CP(20) RL_CP(24) RL_CP(32) RL_CP(40)
#undef RL_CP
  return hipErrorInvalidValue;  // N > 10240: no layout either
}

}  // namespace rl
