// mutctx_kernels.hip -- MutationRateWithContext on the device: the opportunity of every epoch and category
// (include/relate_amd.h has the definition; mutctx.cpp restates the reference's loop on one host thread and is the
// authority this file is held to, bit for bit).
//
// Per batch of trees: mutrate_kernel (mutrate_kernels.hip), one workgroup per tree, leaves LEN [trees][E], the branch
// length of every tree in every epoch, and the root's float time in device memory; the root times and the flags come
// back, the lengths do not.  The batch's qualifying SNPs go up as TREE [snps] (the tree within the batch) and CNT
// [snps][96] uint32, in the .mut's order, kMutctxSnpChunk at a time.
//
// mutctx_chains_kernel, one lane per cell (e, c) of the E x 96 accumulators, cell = e * 96 + c, one wavefront per
// workgroup: the lane loads its accumulator, walks the chunk's SNPs in order with
//     acc = acc + LEN[TREE[s]][e] * (double)CNT[s][c]      (a product, then a sum: two roundings)
// and stores it.  The loads do not depend on the chain: the operands of kMutctxDepth SNPs are in registers before
// the first of their additions, which stay one chain per lane.  The 64 lanes of a wavefront read 64 consecutive words
// of a SNP's row; 96 = 64 + 32, so a wavefront covers one epoch or two and its length loads hit one address or two.
// TREE[s] is the same for all lanes.  The accumulators stay in device memory between launches.
// No LDS, no scratch, no atomics, every product and sum a separate operation (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "common.h"
#include "mutctx.h"

namespace rl {

__global__ void __launch_bounds__(64) mutctx_chains_kernel(const double *__restrict__ LEN, const int *__restrict__ TREE,
                                                           const unsigned *__restrict__ CNT, int nsnps, int E,
                                                           double *__restrict__ OPP) {
  const int cell = blockIdx.x * 64 + threadIdx.x;
  if (cell >= E * kMutctxCategories) return;
  const int e = cell / kMutctxCategories, c = cell - e * kMutctxCategories;
  const double *len = LEN + e;
  const unsigned *cnt = CNT + c;
  double acc = OPP[cell];
  int s = 0;
  for (; s + kMutctxDepth <= nsnps; s += kMutctxDepth) {
    double l[kMutctxDepth];
    unsigned k[kMutctxDepth];
#pragma unroll
    for (int i = 0; i < kMutctxDepth; i++) {
      l[i] = len[(size_t)TREE[s + i] * E];
      k[i] = cnt[(size_t)(s + i) * kMutctxCategories];
    }
#pragma unroll
    for (int i = 0; i < kMutctxDepth; i++) {
      const double term = l[i] * (double)k[i];
      acc = acc + term;
    }
  }
  for (; s < nsnps; s++) {
    const double term = len[(size_t)TREE[s] * E] * (double)cnt[(size_t)s * kMutctxCategories];
    acc = acc + term;
  }
  OPP[cell] = acc;
}

struct MutctxDevice {
  int N = 0, E = 0, device = 0;
  DevBuf ep, opp, len, root, tree, cnt;
  TreeBatch trees;
  double seconds[3] = {0.0, 0.0, 0.0};
};

int mutctx_device_begin(MutctxDevice **out, int N, const double *epochs, int E, int device) {
  *out = nullptr;
  if (N < 2 || N > kMutrateMaxN) {
    set_error("rl_mutctx_trees: trees of 2 <= N <= %d leaves (N=%d)", kMutrateMaxN, N);
    return RL_EINVAL;
  }
  if (E < 2 || E > kMutrateMaxEpochs) {
    set_error("rl_mutctx_trees: 2 <= epochs <= %d (%d given)", kMutrateMaxEpochs, E);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_mutctx_trees", device)) return rc;
  MutctxDevice *d = new MutctxDevice;
  d->N = N, d->E = E, d->device = device;
  const size_t B = (size_t)mutrate_batch_trees(N);
  int rc = d->ep.alloc((size_t)E * 8);
  rc = rc ? rc : d->opp.alloc((size_t)E * kMutctxCategories * 8);
  rc = rc ? rc : d->trees.alloc(N, (int)B);
  rc = rc ? rc : d->len.alloc(B * E * 8);
  rc = rc ? rc : d->root.alloc(B * 4);
  rc = rc ? rc : d->tree.alloc((size_t)kMutctxSnpChunk * 4);
  rc = rc ? rc : d->cnt.alloc((size_t)kMutctxSnpChunk * kMutctxCategories * 4);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(d->ep.p, epochs, (size_t)E * 8, hipMemcpyHostToDevice);
  if (!rc && e == hipSuccess) e = hipMemset(d->opp.p, 0, (size_t)E * kMutctxCategories * 8);
  if (rc || e != hipSuccess) {
    if (!rc) set_error("rl_mutctx_trees: setting up the device failed: %s", hipGetErrorString(e));
    delete d;
    return rc ? rc : RL_EHIP;
  }
  *out = d;
  return RL_OK;
}

int mutctx_device_add(MutctxDevice *d, const int *parents, const double *branch_length, int ntrees, const int *snp_tree,
                      const uint32_t *counts, long long nsnps, float *roots, int *bad_tree) {
  typedef std::chrono::steady_clock Clock;
  const auto since = [](Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); };
  *bad_tree = -1;
  TreeBatch &tb = d->trees;
  if (ntrees < 1 || ntrees > tb.batch || nsnps < 0) {
    set_error("rl_mutctx_trees: a batch of %d trees, %lld SNPs (1 <= trees <= %d)", ntrees, nsnps, tb.batch);
    return RL_EINVAL;
  }
  for (long long s = 0; s < nsnps; s++)
    if (snp_tree[s] < 0 || snp_tree[s] >= ntrees) {
      set_error("rl_mutctx_trees: SNP %lld of a batch names tree %d of %d", s, snp_tree[s], ntrees);
      return RL_EINVAL;
    }
  RL_HIP(hipSetDevice(d->device));
  const int N = d->N, E = d->E;
  Clock::time_point t0 = Clock::now();
  if (const int rc = tb.upload(parents, branch_length, 0, ntrees)) return rc;
  RL_HIP(hipMemset(d->len.p, 0, (size_t)ntrees * E * 8));
  RL_HIP(hipMemset(d->root.p, 0, (size_t)ntrees * 4));
  RL_HIP(mutrate_launch(tb.par.as<int>(), tb.bl.as<double>(), d->ep.as<double>(), E, N, ntrees, d->len.as<double>(),
                        tb.flag.as<int>(), d->root.as<float>()));
  // (the copies wait for the kernel)
  int bad = -1;
  if (const int rc = tb.first_not_done(ntrees, &bad)) return rc;
  RL_HIP(hipMemcpy(roots, d->root.p, (size_t)ntrees * 4, hipMemcpyDeviceToHost));
  d->seconds[0] += since(t0);
  if (bad >= 0) {
    *bad_tree = bad;
    return RL_EINVAL;
  }
  const int cells = E * kMutctxCategories, grid = (cells + 63) / 64;
  for (long long s0 = 0; s0 < nsnps; s0 += kMutctxSnpChunk) {
    const int n = (int)std::min<long long>(kMutctxSnpChunk, nsnps - s0);
    t0 = Clock::now();
    RL_HIP(hipMemcpy(d->tree.p, snp_tree + s0, (size_t)n * 4, hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(d->cnt.p, counts + (size_t)s0 * kMutctxCategories, (size_t)n * kMutctxCategories * 4, hipMemcpyHostToDevice));
    d->seconds[1] += since(t0);
    t0 = Clock::now();
    hipLaunchKernelGGL(mutctx_chains_kernel, dim3(grid), dim3(64), 0, nullptr, d->len.as<double>(), d->tree.as<int>(),
                       d->cnt.as<unsigned>(), n, E, d->opp.as<double>());
    RL_HIP(hipGetLastError());
    RL_HIP(hipDeviceSynchronize());  // the next chunk overwrites the arrays this one reads
    d->seconds[2] += since(t0);
  }
  return RL_OK;
}

int mutctx_device_finish(MutctxDevice *d, double *opportunity) {
  RL_HIP(hipSetDevice(d->device));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(opportunity, d->opp.p, (size_t)d->E * kMutctxCategories * 8, hipMemcpyDeviceToHost));
  return RL_OK;
}

void mutctx_device_seconds(const MutctxDevice *d, double *seconds) { std::copy(d->seconds, d->seconds + 3, seconds); }

void mutctx_device_free(MutctxDevice *d) { delete d; }

}  // namespace rl
