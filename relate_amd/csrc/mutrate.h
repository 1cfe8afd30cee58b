// mutrate.h -- AvgMutationRate: what mutrate.cpp (host twin, files, C ABI) asks of mutrate_kernels.hip (device).
#pragma once
#include <cstddef>

#include "tree_batch.h"

namespace rl {

constexpr int kMutrateMaxN = 10240;    // the LDS layout of a tree: kids, then times and their sorted copy
constexpr int kMutrateMaxEpochs = 64;  // one lane of one wavefront per epoch
// a batch of trees is what fits this many bytes of tree arrays (mutrate_batch_trees)
constexpr size_t kMutrateBatchBytes = (size_t)2 << 20;

// trees per batch at N leaves: kMutrateBatchBytes over the bytes one tree takes on the device (parents 4, branch
// lengths 8 per node; a flag of 4), at least 1
inline int mutrate_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1;
  return batch_trees(kMutrateBatchBytes, nodes * 12 + 4);
}

// out [ntrees][E] doubles: the branch length of every tree in every epoch (entry E-1 is 0); the row of a tree whose
// flag is not kTreeDone keeps zeros.  flags: [ntrees].  epochs [E] have passed the host's checks; N and E
// beyond the limits are RL_EINVAL before any launch.
int mutrate_device(const int *parents, const double *branch_length, int N, int ntrees, const double *epochs, int E,
                   int device, double *out, int *flags);

// the host twin on trees [ntrees][2N-1]: out [ntrees][E]; roots (may be null) [ntrees]: the root's float time, the last
// of the sorted coordinates.  RL_EINVAL names the tree (`where`: the trees' origin; tree_id or null: what a tree is
// called).  with_device: the trees were refused by the device, so one the host accepts is refused too
int mutrate_host_rows(const int *parents, const double *bl, int N, int ntrees, const double *ep, int E, double *out,
                      float *roots, const char *where, const int *tree_id, bool refused_by_device = false);

#ifdef __HIPCC__
// the per-tree kernel on device pointers, n trees (n workgroups) on the null stream: rows [n][E] and flag [n] start at
// 0; root (may be null) [n] floats
hipError_t mutrate_launch(const int *par, const double *bl, const double *ep, int E, int N, int n, double *rows, int *flag,
                          float *root);
#endif

}  // namespace rl
