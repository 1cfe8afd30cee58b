// pairwise.h -- PairwiseCoalescence: what pairwise.cpp (host, C ABI) asks of pairwise_kernels.hip (device).
#pragma once

namespace rl {

struct PairwiseDevice;  // S on the device and the staging room of one batch of trees

int pairwise_device_begin(PairwiseDevice **out, int N, bool time, int device);
// adds the trees in order; RL_EINVAL with *bad_tree = the first tree the device refused (no message set)
int pairwise_device_add(PairwiseDevice *d, const int *parents, const double *branch_length, const long long *weights,
                        int ntrees, int *bad_tree);
int pairwise_device_finish(PairwiseDevice *d, void *sum_out);
void pairwise_device_free(PairwiseDevice *d);

}  // namespace rl
