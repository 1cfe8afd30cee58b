// tree_batch.h -- what the device sides of the modes that consume a dated tree sequence share around their kernels
// (coalrate_kernels.hip, pairwise_kernels.hip, coaltree_kernels.hip, mutrate_kernels.hip, mutctx_kernels.hip,
// frequency_kernels.hip, subtrees_kernels.hip): the flag a kernel leaves for a tree, the size of a batch, and
// TreeBatch, the staging room of one batch of trees -- parent arrays, branch lengths and flags -- with the copies up,
// the clearing of the flags and the copy back.  A driver keeps what is its own: its other buffers, its second kernel,
// its output copies, its rule for a batch with a refused tree, and the hipDeviceSynchronize() that guards the reuse of
// the staging arrays by the next batch.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace rl {

// what a kernel says of a tree in the tree's flag word, cleared before the launch.  kTreeNeedsHost: the tree is
// sound, the host walks it (frequency_kernels.hip: tied node times)
enum { kTreeDone = 0, kTreeRefused = 1, kTreeNeedsHost = 2 };

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// trees per batch: what fits `bytes` at per_tree bytes of device arrays a tree, at least 1 and at most 2^20
inline int batch_trees(size_t bytes, size_t per_tree) {
  const size_t b = bytes / per_tree;
  return b < 1 ? 1 : (b > (1u << 20) ? 1 << 20 : (int)b);
}

struct TreeBatch {
  DevBuf par, bl, flag;    // [batch][2N-1] ints, [batch][2N-1] doubles (if asked for), [batch] ints
  std::vector<int> flags;  // the host's copy of flag
  size_t nodes = 0;
  int batch = 0;

  int alloc(int N, int batch_trees, bool with_lengths = true) {
    nodes = (size_t)2 * N - 1;
    batch = batch_trees;
    flags.resize((size_t)batch);
    int rc = par.alloc((size_t)batch * nodes * 4);
    if (!rc && with_lengths) rc = bl.alloc((size_t)batch * nodes * 8);
    return rc ? rc : flag.alloc((size_t)batch * 4);
  }
  // the n trees from t0 of parents (and of bl_or_null) up, their flags cleared.  A driver's other copies up go before
  // it and its other memsets behind it: a copy issued behind a memset waits for it
  int upload(const int *parents, const double *bl_or_null, size_t t0, int n) {
    RL_HIP(hipMemcpy(par.p, parents + t0 * nodes, (size_t)n * nodes * 4, hipMemcpyHostToDevice));
    if (bl_or_null) RL_HIP(hipMemcpy(bl.p, bl_or_null + t0 * nodes, (size_t)n * nodes * 8, hipMemcpyHostToDevice));
    RL_HIP(hipMemset(flag.p, 0, (size_t)n * 4));
    return RL_OK;
  }
  // the flags of the n trees back into `flags`: the copy waits for the kernel
  int download(int n) {
    RL_HIP(hipMemcpy(flags.data(), flag.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RL_OK;
  }
  // download, then *first = the first of the n trees whose flag is not kTreeDone, or -1
  int first_not_done(int n, int *first) {
    if (const int rc = download(n)) return rc;
    const auto it = std::find_if(flags.begin(), flags.begin() + n, [](int f) { return f != kTreeDone; });
    *first = it == flags.begin() + n ? -1 : (int)(it - flags.begin());
    return RL_OK;
  }
};

// One argument list for a kernel that comes in two workgroup sizes: with
//   const auto go = [&](auto kernel, int threads) { return launch_with_lds(kernel, n, threads, dyn, nullptr, args...); };
// a driver writes `N <= small ? go(k<256>, 256) : go(k<1024>, 1024)`.

}  // namespace rl
