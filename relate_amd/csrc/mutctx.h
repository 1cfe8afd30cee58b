// mutctx.h -- MutationRateWithContext: what mutctx.cpp (host twin, files, C ABI) asks of mutctx_kernels.hip (device).
#pragma once
#include <cstddef>
#include <cstdint>

#include "mutrate.h"

namespace rl {

constexpr int kMutctxCategories = 96;  // the trinucleotide categories; a SNP's row of counts is this many uint32
// the qualifying SNPs of a batch of trees go up this many at a time (384 bytes each: 12 MB)
constexpr int kMutctxSnpChunk = 1 << 15;
// SNPs whose operands a lane of the chains kernel holds in registers at a time
constexpr int kMutctxDepth = 16;

struct MutctxDevice;  // the accumulators [E][96] on the device and the room of one batch of trees and one chunk of SNPs

// epochs [E] have passed the host's checks; N and E beyond the per-tree kernel's limits (mutrate.h) are RL_EINVAL
// before any launch.  The accumulators start at +0.
int mutctx_device_begin(MutctxDevice **out, int N, const double *epochs, int E, int device);
// one batch: ntrees <= mutrate_batch_trees(N) trees and its qualifying SNPs in the .mut's order, snp_tree[s] in
// [0, ntrees) the SNP's tree within the batch, counts [nsnps][96].  roots [ntrees]: the root's float time of every
// tree.  RL_EINVAL with *bad_tree = the first tree the device refused (no message set; nothing of the batch is added)
int mutctx_device_add(MutctxDevice *d, const int *parents, const double *branch_length, int ntrees, const int *snp_tree,
                      const uint32_t *counts, long long nsnps, float *roots, int *bad_tree);
// opportunity [E][96]
int mutctx_device_finish(MutctxDevice *d, double *opportunity);
// seconds [3] since begin, each measured with the device idle on both sides: the tree arrays up, the per-tree kernel
// and flags and roots down | the SNPs' trees and counts up | the chains kernel
void mutctx_device_seconds(const MutctxDevice *d, double *seconds);
void mutctx_device_free(MutctxDevice *d);

}  // namespace rl
