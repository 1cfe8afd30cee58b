// mutrate.h -- AvgMutationRate: what mutrate.cpp (host twin, files, C ABI) asks of mutrate_kernels.hip (device).
#pragma once
#include <cstddef>

namespace rl {

constexpr int kMutrateMaxN = 10240;    // the LDS layout of a tree: kids, then times and their sorted copy
constexpr int kMutrateMaxEpochs = 64;  // one lane of one wavefront per epoch
// a batch of trees is what fits this many bytes of tree arrays (mutrate_batch_trees)
constexpr size_t kMutrateBatchBytes = (size_t)2 << 20;

// trees per batch at N leaves: kMutrateBatchBytes over the bytes one tree takes on the device (parents 4, branch
// lengths 8 per node; a flag of 4), at least 1
inline int mutrate_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1, per_tree = nodes * 12 + 4;
  const size_t b = kMutrateBatchBytes / per_tree;
  return b < 1 ? 1 : (b > (1u << 20) ? 1 << 20 : (int)b);
}

// what the device says of a tree
enum { kMutrateTreeDone = 0, kMutrateTreeRefused = 1 };

// out [ntrees][E] doubles: the branch length of every tree in every epoch (entry E-1 is 0); the row of a tree whose
// flag is not kMutrateTreeDone keeps zeros.  flags: [ntrees].  epochs [E] have passed the host's checks; N and E
// beyond the limits are RL_EINVAL before any launch.
int mutrate_device(const int *parents, const double *branch_length, int N, int ntrees, const double *epochs, int E,
                   int device, double *out, int *flags);

}  // namespace rl
