// subtrees.h -- SubTreesForSubpopulation: what subtrees.cpp (host twin, files, C ABI) asks of subtrees_kernels.hip
// (device).
#pragma once
#include <cstddef>

#include "tree_batch.h"

namespace rl {

constexpr int kSubtreesMaxN = 10240;  // the LDS layout of a tree: kids, then counts and new labels, 8 bytes a node
// a batch of trees is what fits this many bytes of tree arrays (subtrees_batch_trees): 22 trees at N = 10,240 and
// 233 at N = 1000
constexpr size_t kSubtreesBatchBytes = (size_t)16 << 20;

// trees per batch at N leaves: kSubtreesBatchBytes over the bytes one tree takes on the device at M = N (in: parents
// 4, branch lengths 8 per node; out: convert_index 4, number_in_subpop 4, the subtree's parent 4, branch length 8 and
// time 4 per node; a flag of 4), at least 1
inline int subtrees_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1;
  return batch_trees(kSubtreesBatchBytes, nodes * 36 + 4);
}

// The subtrees of ntrees trees of N leaves for the M leaves whose new labels leaf_label [N] gives (k for the k-th
// leaf of the subset in rising label order, -1 for any other leaf; the host has checked the subset).  Outputs per
// tree: sub_parent, sub_bl, sub_time [2M-1]; convert_index, number_in_subpop [2N-1].  N beyond the limits is
// RL_EINVAL before any launch.  RL_EINVAL with *bad_tree = the first tree the device refused (no message set; the
// outputs of the trees before it in its batch are not delivered)
int subtrees_device(const int *parents, const double *branch_length, int N, int ntrees, const int *leaf_label, int M,
                    int device, int *sub_parent, double *sub_bl, float *sub_time, int *convert_index,
                    int *number_in_subpop, int *bad_tree);

}  // namespace rl
