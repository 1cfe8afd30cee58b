// coaltree.h -- CoalRateForTree: what coaltree.cpp (host twin, files, C ABI) asks of coaltree_kernels.hip (device).
#pragma once
#include <cstddef>

#include "tree_batch.h"

namespace rl {

constexpr int kCoaltreeMaxN = 10240;    // the LDS layout of a tree: kids, then times and their sorted copy
constexpr int kCoaltreeMaxEpochs = 64;  // one lane of one wavefront per epoch
constexpr int kCoaltreeBlockSize = 1000;  // trees per block in CoalescenceRateForTree (CoalescentRateForSection.cpp:716)
// a batch of trees is what fits this many bytes of tree arrays (coaltree_batch_trees): 51 trees at N = 10,240, so that
// a launch of the terms kernel has a workgroup for a fifth of the CUs, and 680 at N = 1000
constexpr size_t kCoaltreeBatchBytes = (size_t)16 << 20;

// trees per batch at N leaves: kCoaltreeBatchBytes over the bytes one tree takes on the device (parents 4, branch
// lengths 8 per node; a term of 8 per internal node; first 4, count 4 and exit term 8 per epoch at the most epochs;
// factor and flag 4 each), at least 1
inline int coaltree_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1;
  return batch_trees(kCoaltreeBatchBytes, nodes * 12 + ((size_t)N - 1) * 8 + (size_t)kCoaltreeMaxEpochs * 16 + 8);
}

// (int)(ntrees / (double)block_size + 1), coal_tree::update_ancmut (coal_tree.cpp:78): the last block may stay empty
inline int coaltree_num_blocks(long long ntrees, int block_size) { return (int)((double)ntrees / (double)block_size + 1); }

struct CoaltreeDevice;  // the accumulators [num_blocks][E] on the device and the room of one batch of trees

// epochs [E] have passed the host's checks; N and E beyond the limits are RL_EINVAL before any launch.  ntrees: the
// trees of the whole sequence, which decide the number of blocks; block_size >= 1.  The accumulators start at +0.
int coaltree_device_begin(CoaltreeDevice **out, int N, const double *epochs, int E, long long ntrees, int block_size,
                          int device);
// adds the trees that follow those added before, in order, onto the accumulators of their blocks; the factors are
// finite and >= 0.  RL_EINVAL with *bad_tree = the first tree of this call the device refused (no message set; none
// of the call's trees is added then)
int coaltree_device_add(CoaltreeDevice *d, const int *parents, const double *branch_length, const float *factors,
                        int ntrees, int *bad_tree);
// num, denom: [num_blocks][E]
int coaltree_device_finish(CoaltreeDevice *d, double *num, double *denom);
void coaltree_device_free(CoaltreeDevice *d);

}  // namespace rl
