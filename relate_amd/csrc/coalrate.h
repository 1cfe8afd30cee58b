// coalrate.h -- CoalescentRateForSection: what coalrate.cpp (host, files, C ABI) asks of coalrate_kernels.hip (device).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "tree_batch.h"

namespace rl {

constexpr int kCoalrateMaxN = 10240;   // 16-bit labels and ranks, the LDS layout of the accumulation
constexpr int kCoalrateMaxEpochs = 64;  // the epochs and the per-plane terms of a tree live in LDS
// a batch of trees is what fits this many bytes of tree arrays (coalrate_batch_trees)
constexpr size_t kCoalrateBatchBytes = (size_t)2 << 20;

// trees per batch at N leaves: kCoalrateBatchBytes over the bytes one tree takes on the device (parents 4, branch
// lengths 8 per node; rank 2, g 2, time 4, epoch index 1 per leaf; factor and flag 4 each), at least 1
inline int coalrate_batch_trees(int N) {
  const size_t nodes = (size_t)2 * N - 1;
  return batch_trees(kCoalrateBatchBytes, nodes * 12 + (size_t)N * 9 + 8);
}

// ---- the .poplabels as FinalizePopulationSize and SubTreesForSubpopulation (subtrees.cpp) read it
// Sample::Read (src/sample.cpp:4-103): the group names sorted, and the group of every haplotype -- two haplotypes per
// line, one if any line's fourth column is `1`; a file that mixes the two is refused (defined in coalrate.cpp)
int read_poplabels(const char *mode, const std::string &fn, std::vector<std::string> &groups, std::vector<int> &group_of_haplotype);

struct CoalrateDevice;  // D on the device and the staging room of one batch of trees

// epochs [E] have passed the host's checks (2 <= E <= kCoalrateMaxEpochs, ep[0] = 0, rising)
int coalrate_device_begin(CoalrateDevice **out, int N, const float *epochs, int E, int device);
// adds the trees in order; RL_EINVAL with *bad_tree = the first tree the device refused (no message set)
int coalrate_device_add(CoalrateDevice *d, const int *parents, const double *branch_length, const float *factors,
                        int ntrees, int *bad_tree);
int coalrate_device_finish(CoalrateDevice *d, float *out);
void coalrate_device_free(CoalrateDevice *d);

}  // namespace rl
