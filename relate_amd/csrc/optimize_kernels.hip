// optimize_kernels.hip -- the per-tree pass of `--mode OptimizeParameters` over the distance matrix.
//
// AncesTreeBuilder::OptimizeParameters (anc_builder.cpp:821-973) builds a tree at EVERY SNP and, before each,
// "cancels" the SNP in the matrix GetMatrix has just filled (:869-882, :926-939): along the row of every carrier i
//     d[i][j] += log_ratio   at every NON-carrier column j      (log_ratio = (float)log(theta / ntheta) < 0)
//     min_i    = min over ALL j of the row as it then is        (the diagonal included)
//     d[i][j] -= min_i       at every column j
// and MinMatch::Initialize (tree_builder.cpp:59-146, the variant without a prior) then starts from the minimum of
// every row off its diagonal.
//
// cancel_rowmin_kernel does both in ONE pass: a workgroup per row, the row read from HBM once and -- a carrier's --
// written once; between the minimum and the subtraction the row waits in LDS (N <= 10,240 floats = 40 KB), every
// thread reading back the columns it put there itself.  A non-carrier's row is not touched by the reference: it is
// only scanned for its off-diagonal minimum.  Per element the same float operations in the same order as the host
// loop (one add, one subtract; the build has no FMA contraction and no fast-math), so the matrix is the reference's
// bit for bit; a minimum does not depend on the order it is taken in (no NaN can arise: the entries are finite).
//
// The pass runs AFTER the matrix kernel (matrix_kernels.hip) on the finished matrix, on the builder's stream,
// instead of inside that kernel's last pass the way the carrier penalty of BuildTopology is folded in
// (rl_window_matrix_rows_device_ex): the matrix kernel is the one every BuildTopology tree pays for and is kept
// as it is -- registers, LDS and code path -- for that stage; this mode pays one more read of N^2 floats and a
// write of the carriers' rows per tree; DESIGN.md 8a has what that costs per tree as measured.
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

namespace rl {

// minimum over the workgroup's 256 threads, returned to all of them (part: 4 floats of LDS)
__device__ inline float block_min_256(float v, float *part) {
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    if (o < v) v = o;
  }
  __syncthreads();  // (part may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = part[0];
  for (int w = 1; w < 4; w++)
    if (part[w] < m) m = part[w];
  return m;
}

// D: N x N floats, row-major; member: N carrier flags; out: N floats.  grid = N workgroups of 256 threads,
// dynamic LDS = N floats.
__global__ void __launch_bounds__(256) cancel_rowmin_kernel(float *__restrict__ D, int N,
                                                           const unsigned char *__restrict__ member, float log_ratio,
                                                           float *__restrict__ out) {
  extern __shared__ float held[];  // a carrier's row between its minimum and the subtraction
  __shared__ float part[4];
  const int a = blockIdx.x;
  if (a >= N) return;
  float *row = D + (size_t)a * N;
  float rm = INFINITY;  // the row's minimum off the diagonal, as the row ends up
  if (!member[a]) {
    for (int col = threadIdx.x; col < N; col += 256) {
      const float x = row[col];
      if (col != a && x < rm) rm = x;
    }
  } else {
    float mn = INFINITY;
    for (int col = threadIdx.x; col < N; col += 256) {
      float x = row[col];
      if (!member[col]) x = x + log_ratio;  // :873, :930
      held[col] = x;
      if (x < mn) mn = x;  // :875, :932 (all columns)
    }
    mn = block_min_256(mn, part);
    for (int col = threadIdx.x; col < N; col += 256) {
      const float x = held[col] - mn;  // :879, :936
      row[col] = x;
      if (col != a && x < rm) rm = x;
    }
  }
  rm = block_min_256(rm, part);
  if (threadIdx.x == 0) out[a] = rm;
}

hipError_t launch_cancel_rowmin(float *D, int N, const unsigned char *member, float log_ratio, float *rowmin,
                                hipStream_t stream) {
  hipLaunchKernelGGL(cancel_rowmin_kernel, dim3(N), dim3(256), (size_t)N * sizeof(float), stream, D, N, member,
                     log_ratio, rowmin);
  return hipGetLastError();
}

}  // namespace rl

using namespace rl;

extern "C" int rl_debug_cancel_rowmin(float *d, int N, const char *carriers, float log_ratio, float *rowmin) {
  if (!d || !carriers || !rowmin || N < 2 || N > 10240) {
    set_error("rl_debug_cancel_rowmin: bad arguments (N=%d; 2 <= N <= 10240)", N);
    return RL_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    set_error("no usable HIP device");
    return RL_ENODEVICE;
  }
  DevBuf dD, dm, dr;
  const size_t nn = (size_t)N * N;
  int rc = dD.alloc(nn * sizeof(float));
  rc = rc ? rc : dm.alloc((size_t)N);
  rc = rc ? rc : dr.alloc((size_t)N * sizeof(float));
  if (rc) return rc;
  std::vector<unsigned char> flags((size_t)N);
  for (int i = 0; i < N; i++) flags[i] = carriers[i] ? 1 : 0;
  RL_HIP(hipMemcpy(dD.p, d, nn * sizeof(float), hipMemcpyHostToDevice));
  RL_HIP(hipMemcpy(dm.p, flags.data(), (size_t)N, hipMemcpyHostToDevice));
  RL_HIP(launch_cancel_rowmin(dD.as<float>(), N, dm.as<unsigned char>(), log_ratio, dr.as<float>(), nullptr));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(d, dD.p, nn * sizeof(float), hipMemcpyDeviceToHost));
  RL_HIP(hipMemcpy(rowmin, dr.p, (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
  return RL_OK;
}
