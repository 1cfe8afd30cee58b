// frequency.h -- Frequency: what frequency.cpp (host walk, files, C ABI) asks of frequency_kernels.hip (device).
#pragma once
#include <cstddef>

#include "tree_batch.h"

namespace rl {

constexpr int kFrequencyMaxN = 10240;    // 16-bit labels, ranks and intervals; the LDS layout of a tree
constexpr int kFrequencyMaxEpochs = 64;  // the boundaries, their counts and the bins of a SNP live in LDS
// a batch of trees is what fits this many bytes of tree arrays (frequency_batch_trees)
constexpr size_t kFrequencyBatchBytes = (size_t)2 << 20;

// trees per batch at N leaves: kFrequencyBatchBytes over the bytes one tree takes on the device (parents 4, branch
// lengths 8 per node; root time, flag and SNP offset 4 each), at least 1
inline int frequency_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1;
  return batch_trees(kFrequencyBatchBytes, nodes * 12 + 12);
}

// The rows of the SNPs snp_first[t] .. snp_first[t+1]-1 of every tree t, on branch snp_branch[s]: out [nsnps][2E+2]
// int32 -- the E counts of carriers, the E counts of lineages (both from the oldest boundary to 0), when_DAF_is_half,
// when_mutation_has_freq2.  A SNP whose branch is not in [0, 2N-3] and the SNPs of a tree whose flag is not
// kTreeDone keep zeros.  root_time, flags: [ntrees].  epochs [E] have passed the host's checks; N and E
// beyond the limits are RL_EINVAL before any launch.
int frequency_device(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_first,
                     const int *snp_branch, int nsnps, const float *epochs, int E, int device, int *out,
                     float *root_time, int *flags);

}  // namespace rl
