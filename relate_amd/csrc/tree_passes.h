// tree_passes.h -- the per-tree passes the tree kernels share (compare_kernels.hip: CompareTopology; pairwise_kernels.hip:
// PairwiseCoalescence).  A tree comes as a parent array with labels rising from child to parent; its tables live in
// LDS, internal node v at index v - N (ni = N - 1 of them).
//   build_kids      all threads: kids of every internal node, with the validity checks that must precede any use of a
//                   label as an index;
//   wave_clade_sizes   one wavefront: leaves below every internal node, label order;
//   wave_left_ends     one wavefront: left end of every internal node's interval of depth-first ranks, falling order.
// The two wave passes take the internal nodes 64 at a time; a lane PULLS what it depends on -- from LDS for a node of
// another 64, by lane shuffle for a node of its own 64 once that lane is done (a ballot of the done lanes per round;
// the lane whose dependencies lie outside the 64 never waits).  A round costs a ballot and one or two shuffles, no
// LDS traffic: a caterpillar, whose every node waits for the one before it, takes N-1 such rounds per pass, O(N) in
// all -- there is no walk from a leaf to the root anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace rl {

typedef unsigned short u16;

// K: ni words, first child + 1 << 16 | second child + 1 (first = the smaller label); up (may be null): ni parent
// indices (internal numbering) of the internal nodes.  Every node v puts v+1 into its parent's word with atomicMax
// (low half: the child with the larger label), then every other child adds (v+1) << 16.  A parent label that is not
// above its child's, not internal or out of range, a root with a parent, an internal node with a half left empty:
// refused.  (Every non-root node has passed the parent test, so the N-1 internal nodes have 2N-2 children between
// them, and none with fewer than two means all with exactly two.)
// All threads of the workgroup call it; returns the same value to all.
template <int T>
__device__ bool build_kids(const int *__restrict__ par, int N, unsigned *K, u16 *up, int *bad) {
  const int nodes = 2 * N - 1, ni = N - 1;
  for (int i = threadIdx.x; i < ni; i += T) K[i] = 0u;
  if (threadIdx.x == 0) *bad = par[nodes - 1] != -1;
  __syncthreads();
  for (int v = threadIdx.x; v < nodes - 1; v += T) {
    const int p = par[v];
    if (!(p > v && p >= N && p < nodes)) {
      *bad = 1;
    } else {
      atomicMax(&K[p - N], (unsigned)(v + 1));
      if (up && v >= N) up[v - N] = (u16)(p - N);
    }
  }
  __syncthreads();
  if (*bad) return false;
  for (int v = threadIdx.x; v < nodes - 1; v += T) {
    const int p = par[v];
    if ((K[p - N] & 0xffffu) != (unsigned)(v + 1)) atomicAdd(&K[p - N], (unsigned)(v + 1) << 16);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ni; i += T) {
    const unsigned k = K[i];
    if ((k & 0xffffu) == 0u || (k >> 16) == 0u) *bad = 1;
  }
  __syncthreads();
  return *bad == 0;
}

// SZ[i] = leaves below internal node i.  One wavefront calls it (lane = its lane index).
__device__ inline void wave_clade_sizes(const unsigned *K, int N, u16 *SZ, int lane) {
  const int ni = N - 1;
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;  // lanes this one waits for
    unsigned s1 = 0, s2 = 0;
    if (act) {
      const unsigned k = K[i];
      const int c1 = (int)(k >> 16) - 1, c2 = (int)(k & 0xffffu) - 1;
      if (c1 < N) s1 = 1;
      else if (c1 - N < b) s1 = SZ[c1 - N];
      else d1 = c1 - N - b;
      if (c2 < N) s2 = 1;
      else if (c2 - N < b) s2 = SZ[c2 - N];
      else d2 = c2 - N - b;
    }
    unsigned sz = 0;
    bool done = !act;
    for (;;) {
      const unsigned long long dm = __ballot(done);
      if (dm == ~0ull) break;
      const unsigned t1 = __shfl(sz, d1 < 0 ? 0 : d1, 64), t2 = __shfl(sz, d2 < 0 ? 0 : d2, 64);
      if (!done && (d1 < 0 || ((dm >> d1) & 1)) && (d2 < 0 || ((dm >> d2) & 1))) {
        sz = (d1 < 0 ? s1 : t1) + (d2 < 0 ? s2 : t2);
        done = true;
      }
    }
    if (act) SZ[i] = (u16)sz;
  }
}

// U[i] holds the parent (internal numbering) of internal node i on entry and the left end of its interval on return:
// the first child starts where its parent does, the second after the first child's leaves.  One wavefront calls it;
// each lane calls visit(i, left end, is a second child, is the root) for its node once U[i] is written.
template <class F>
__device__ inline void wave_left_ends(const unsigned *K, const u16 *SZ, u16 *U, int N, int lane, F visit) {
  const int ni = N - 1;
  for (int b = ((ni - 1) / 64) * 64; b >= 0; b -= 64) {
    const int i = b + lane;
    const bool act = i < ni, root = i == ni - 1;
    int dep = -1;
    unsigned base = 0, off = 0;
    bool second = false;
    if (act && !root) {
      const int pi = U[i];
      const int c1 = (int)(K[pi] >> 16) - 1;  // the parent's first child
      second = c1 != i + N;
      if (second) off = c1 < N ? 1u : (unsigned)SZ[c1 - N];
      if (pi >= b + 64) base = U[pi];  // (its left end by now: written 64 or more labels ago)
      else dep = pi - b;
    }
    unsigned lo = 0;
    bool done = !act || root;
    for (;;) {
      const unsigned long long dm = __ballot(done);
      if (dm == ~0ull) break;
      const unsigned t = __shfl(lo, dep < 0 ? 0 : dep, 64);
      if (!done && (dep < 0 || ((dm >> dep) & 1))) {
        lo = (dep < 0 ? base : t) + off;
        done = true;
      }
    }
    if (act) {
      U[i] = (u16)lo;
      visit(i, lo, second, root);
    }
  }
}

}  // namespace rl
