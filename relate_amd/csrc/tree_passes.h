// tree_passes.h -- the per-tree passes the tree kernels share (compare_kernels.hip: CompareTopology; pairwise_kernels.hip:
// PairwiseCoalescence; coalrate_kernels.hip: CoalescentRateForSection; frequency_kernels.hip: Frequency;
// mutrate_kernels.hip: AvgMutationRate and MutationRateWithContext; coaltree_kernels.hip: CoalRateForTree;
// subtrees_kernels.hip: SubTreesForSubpopulation).  A tree comes as a parent array with labels rising from child to
// parent; its tables live in LDS, internal node v at index v - N (ni = N - 1 of them).  What the drivers around the
// kernels share -- the staging of a batch, the flag of a tree -- is in tree_batch.h.
//   build_kids      all threads: kids of every internal node, with the validity checks that must precede any use of a
//                   label as an index;
//   checked_kids    all threads: build_kids and the check of the branch lengths, the prologue of every kernel that
//                   takes a dated tree;
//   wave_pull       one wavefront: the scan every pass below and in the kernels is an instance of;
//   wave_clade_sizes   one wavefront: leaves below every internal node, label order;
//   wave_float_times   one wavefront: the float time of every internal node, rounded at every node, label order;
//   wave_left_ends     one wavefront: left end of every internal node's interval of depth-first ranks, falling order;
//   wave_max_times     one wavefront: the float time of every internal node as Tree::GetCoordinates has it;
//   sorted_max_times   all threads: the checks, wave_max_times and the in-place sort of those times.
// The wave passes take the internal nodes 64 at a time; a lane PULLS what it depends on -- from LDS for a node of
// another 64, by lane shuffle for a node of its own 64 once that lane is done.  A round costs a ballot and a shuffle
// per dependency and value word, no LDS traffic: a caterpillar, whose every node waits for the one before it, takes
// N-1 such rounds per pass, O(N) in all -- there is no walk from a leaf to the root anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

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

// The checked prologue of a kernel that takes a dated tree: build_kids, then the first n_lengths branch lengths
// (2N-2: the root's is not read; 2N-1 in subtrees_kernels.hip) -- one that is negative, infinite or NaN is refused: the
// times would not rise.  All threads of the workgroup call it; returns the same value to all, after a barrier.  The
// kernel writes its flag for a refused tree.
template <int T>
__device__ bool checked_kids(const int *__restrict__ par, const double *__restrict__ bl, int n_lengths, int N, unsigned *K,
                             u16 *up, int *bad) {
  if (!build_kids<T>(par, N, K, up, bad)) return false;
  __syncthreads();  // (every thread has read build_kids' verdict)
  for (int v = threadIdx.x; v < n_lengths; v += T)
    if (!(bl[v] >= 0.0 && bl[v] <= DBL_MAX)) *bad = 1;
  __syncthreads();
  return *bad == 0;
}

inline __device__ int first_child(const unsigned *K, int pi) { return (int)(K[pi] >> 16) - 1; }
inline __device__ int second_child(const unsigned *K, int pi) { return (int)(K[pi] & 0xffffu) - 1; }
// leaves below the first child of internal node pi
inline __device__ unsigned first_child_leaves(const unsigned *K, const u16 *SZ, int N, int pi) {
  const int c1 = first_child(K, pi);
  return c1 < N ? 1u : (unsigned)SZ[c1 - N];
}
// depth-first rank of leaf v, a child of internal node pi whose left end is lo: the first child starts where its
// parent does, the second after the first child's leaves
inline __device__ unsigned leaf_rank(const unsigned *K, const u16 *SZ, int N, int v, int pi, unsigned lo) {
  return lo + (first_child(K, pi) != v ? first_child_leaves(K, SZ, N, pi) : 0u);
}

// (size, min rank << 16 | max rank) of a clade: the value CompareTopology pulls, shuffled member by member
struct SizeSpan {
  unsigned sz, mm;
};
template <class V>
inline __device__ V wave_shfl(V v, int lane) { return __shfl(v, lane, 64); }
inline __device__ SizeSpan wave_shfl(SizeSpan v, int lane) { return SizeSpan{__shfl(v.sz, lane, 64), __shfl(v.mm, lane, 64)}; }

// The pull scan over 64 consecutive items, one per lane of the calling wavefront (all 64 lanes call it).  A lane with
// `pending` set has DEPS (1 or 2) dependencies: d < 0 -- the value is known already and given; d >= 0 -- it is the
// value of lane d of this 64.  Returns combine(value of dependency 1[, of dependency 2]) to a pending lane, V() to
// any other.  Per round: a ballot of the done lanes, a shuffle of every dependency's value, and the lanes whose
// dependencies are all done finish.
// Termination: in a rising pass (children before parents) every dependency is a LOWER lane, in a falling pass
// (parents before children) a HIGHER one -- the callers' labels rise from child to parent, which build_kids has
// checked.  So the lowest (highest) lane not done has no dependency that is not done: every round retires at least
// one lane, 64 rounds at the most, and no lane reads a value before the ballot has shown it final.
template <int DEPS, class V, class F>
inline __device__ V wave_pull(bool pending, int d1, V known1, int d2, V known2, F combine) {
  static_assert(DEPS == 1 || DEPS == 2, "one or two dependencies");
  V val = V();
  bool done = !pending;
  for (;;) {
    const unsigned long long dm = __ballot(done);
    if (dm == ~0ull) break;
    const V t1 = wave_shfl(val, d1 < 0 ? 0 : d1);
    const V t2 = DEPS == 2 ? wave_shfl(val, d2 < 0 ? 0 : d2) : known2;
    if (!done && (d1 < 0 || ((dm >> d1) & 1)) && (DEPS == 1 || d2 < 0 || ((dm >> d2) & 1))) {
      val = combine(d1 < 0 ? known1 : t1, DEPS == 1 || d2 < 0 ? known2 : t2);
      done = true;
    }
  }
  return val;
}
template <class V, class F>
inline __device__ V wave_pull(bool pending, int d, V known, F combine) {
  return wave_pull<1>(pending, d, known, -1, V(), [&](V a, V) { return combine(a); });
}

// Where a rising pass over the 64 items from b finds child c: -1 with *known = leaf(c) or table(c - N) (a leaf; a
// node of an earlier 64, in LDS by now), or the lane of this 64 that will have it.
template <class V, class L, class T>
inline __device__ int child_source(int c, int N, int b, V *known, L leaf, T table) {
  if (c < N) *known = leaf(c);
  else if (c - N < b) *known = table(c - N);
  else return c - N - b;
  return -1;
}

// SZ[i] = leaves below internal node i.  One wavefront calls it (lane = its lane index).
__device__ inline void wave_clade_sizes(const unsigned *K, int N, u16 *SZ, int lane) {
  const int ni = N - 1;
  const auto leaf = [](int) { return 1u; };
  const auto table = [&](int j) { return (unsigned)SZ[j]; };
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;  // lanes this one waits for
    unsigned s1 = 0, s2 = 0;
    if (act) {
      d1 = child_source(first_child(K, i), N, b, &s1, leaf, table);
      d2 = child_source(second_child(K, i), N, b, &s2, leaf, table);
    }
    const unsigned sz = wave_pull<2>(act, d1, s1, d2, s2, [](unsigned a, unsigned c) { return a + c; });
    if (act) SZ[i] = (u16)sz;
  }
}

// TM[i] = time of internal node i as the reference's coalescence-rate recursion has it: a float, rounded at every
// node, t(m) = (float)((double)t(c) + bl[c]) with c the first child of m and t(leaf) = 0.  One wavefront calls it;
// each lane calls visit(i, t) for its node once TM[i] is written.
template <class F>
__device__ inline void wave_float_times(const unsigned *K, const double *__restrict__ bl, int N, float *TM, int lane, F visit) {
  const int ni = N - 1;
  const auto leaf = [](int) { return 0.0f; };
  const auto table = [&](int j) { return TM[j]; };
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int dep = -1;
    float base = 0.0f;
    double len = 0.0;
    if (act) {
      const int c1 = first_child(K, i);
      len = bl[c1];
      dep = child_source(c1, N, b, &base, leaf, table);
    }
    const float t = wave_pull(act, dep, base, [len](float below) { return (float)((double)below + len); });
    if (act) {
      TM[i] = t;
      visit(i, t);
    }
  }
}

// TM[i] = time of internal node i as the reference's Tree::GetCoordinates has it (src/anc.cpp:525-537): a float,
// rounded at every node, t(m) = (float)max((double)t(c2) + bl[c2], (double)t(c1) + bl[c1]) over both children and
// t(leaf) = 0.  One wavefront calls it.
__device__ inline void wave_max_times(const unsigned *K, const double *__restrict__ bl, int N, float *TM, int lane) {
  const int ni = N - 1;
  const auto leaf = [](int) { return 0.0f; };
  const auto table = [&](int j) { return TM[j]; };
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;
    float t1 = 0.0f, t2 = 0.0f;
    double len1 = 0.0, len2 = 0.0;
    if (act) {
      const int c1 = first_child(K, i), c2 = second_child(K, i);
      len1 = bl[c1];
      len2 = bl[c2];
      d1 = child_source(c1, N, b, &t1, leaf, table);
      d2 = child_source(c2, N, b, &t2, leaf, table);
    }
    const float t = wave_pull<2>(act, d1, t1, d2, t2, [len1, len2](float a, float c) {
      return (float)fmax((double)c + len2, (double)a + len1);
    });
    if (act) TM[i] = t;
  }
}

// The prologue of the kernels that consume a tree as its sorted node times (mutrate_kernels.hip: AvgMutationRate;
// coaltree_kernels.hip: CoalRateForTree).  All threads of the workgroup call it; K and S are ni words of LDS each.
//   1. build_kids with its checks, then the branch-length check (negative, infinite or NaN: the times would not rise);
//   2. wavefront 0 takes the times of Tree::GetCoordinates (wave_max_times);
//   3. the N-1 internal times sorted ascending IN PLACE: a bitonic network whose comparators all point the same way
//      (the first step of a merge of width k pairs i with i ^ (k-1), the others i with i ^ j), so the slots from N-1
//      to the next power of two stand for +infinity without existing -- a comparator that reaches one is skipped.
//      Only values move: no labels, no ranks.
// Returns false to all threads for a refused tree; otherwise it ends at the __syncthreads() after the sort, with S
// the sorted times: interval k, (S[k-1], S[k]] with S[-1] = 0, carries N - k lineages.
template <int T>
__device__ bool sorted_max_times(const int *__restrict__ par, const double *__restrict__ bl, int N, unsigned *K,
                                 float *S, int *bad) {
  const int nodes = 2 * N - 1, ni = N - 1, tid = threadIdx.x;
  int P = 1;
  while (P < ni) P <<= 1;
  if (!checked_kids<T>(par, bl, nodes - 1, N, K, nullptr, bad)) return false;
  if ((tid >> 6) == 0) wave_max_times(K, bl, N, S, tid & 63);
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int flip = j == (k >> 1) ? k - 1 : j;
      for (int i = tid; i < P; i += T) {
        const int l = i ^ flip;
        if (l > i && l < ni) {  // (l >= ni: +infinity, in its place already)
          const float a = S[i], b = S[l];
          if (a > b) {
            S[i] = b;
            S[l] = a;
          }
        }
      }
      __syncthreads();
    }
  return true;
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
      second = first_child(K, pi) != i + N;
      if (second) off = first_child_leaves(K, SZ, N, pi);
      if (pi >= b + 64) base = U[pi];  // (its left end by now: written 64 or more labels ago)
      else dep = pi - b;
    }
    const unsigned lo = wave_pull(act && !root, dep, base, [off](unsigned a) { return a + off; });  // the root: 0
    if (act) {
      U[i] = (u16)lo;
      visit(i, lo, second, root);
    }
  }
}

}  // namespace rl
