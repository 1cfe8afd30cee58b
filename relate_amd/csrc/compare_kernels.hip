// compare_kernels.hip -- CompareTopology on the device: the clade (rooted Robinson-Foulds) distance of pairs of trees.
//
// clade_distance_kernel: one workgroup per pair (tree a of batch A, tree b of batch B), Day's algorithm as in the host
// implementation (compare.cpp has the definition and why one table of N entries is enough), in integers, all tables
// of the pair in LDS.  Trees come as parent arrays with labels rising from child to parent; the kernel checks that
// itself (and that the tree is binary) before it uses a label as an index, and answers -1 (tree A) or -2 (tree B)
// for the pair instead of a distance when it does not hold.
//
// Steps of a pair (T threads; "wave 0" steps run on the first wavefront while the others wait at the barrier; steps
// 1 to 3 are the passes of tree_passes.h, which PairwiseCoalescence runs as well):
//   1. kids of A, all threads: every node v puts v+1 into its parent's word with atomicMax (low half: the child with
//      the larger label, the SECOND child), then every other child adds (v+1) << 16 (high half: the FIRST child).  A
//      parent label that is not above its child's, not internal or out of range, a root with a parent, an internal
//      node with a half left empty: refused.  (Every non-root node has passed the parent test, so the N-1 internal
//      nodes have 2N-2 children between them, and none with fewer than two means all with exactly two.)
//   2. sizes of A's clades, wave 0, internal nodes in label order 64 at a time: a lane PULLS the sizes of its two
//      children -- 1 for a leaf, from LDS for a node of an earlier 64, by lane shuffle for a node of its own 64 once
//      that lane is done (a ballot of the done lanes per round; the lowest lane not done never waits, since children
//      have smaller labels).  A round costs a ballot and two shuffles, no LDS traffic: a caterpillar, whose every
//      node waits for the one before it, takes N-1 such rounds per pass, O(N) in all -- there is no walk from a leaf
//      to the root anywhere.
//   3. left ends of A's intervals, wave 0, falling label order, the same scheme with the parent as the one dependency
//      (the first child starts where its parent does, the second after the first child's leaves); the lane writes its
//      table entry as it goes.  The slot that held a node's parent index until then holds its left end afterwards.
//   4. ranks of the leaves, all threads.
//   5. kids of B (step 1 again, in the words A's kids had), then (size, min rank, max rank) of B's clades, wave 0, as
//      in step 2 with min and max packed in one word, each lane testing its own node against the table when it is done.
//   6. d = 2 (N - 2 - common).
//
// LDS, bytes, ni = N-1: kids 4 ni | A: sizes 2 ni, parent / left end 2 ni; B: min << 16 | max 4 ni (the same 4 ni) |
// B sizes 2 ni | ranks 2 N | table 2 N = 14 N - 10: 140 KB at N = 10,000 of the 160 KB a CU has, one pair per CU;
// labels and ranks fit 16 bits up to N = 10,240 (kMaxN), sizes too.  DESIGN.md 8b has the resource table.
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "tree_passes.h"

namespace rl {

constexpr int kCompareMaxN = 10240;
constexpr int kCompareSmallN = 1024;  // up to here one wavefront per pair

template <int T>
__global__ void __launch_bounds__(T) clade_distance_kernel(const int *__restrict__ PA, const int *__restrict__ PB, int N,
                                                           int npairs, const int *__restrict__ pairs,
                                                           int *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  const int pair = blockIdx.x;
  if (pair >= npairs) return;
  const int nodes = 2 * N - 1, ni = N - 1;
  const int *pa = PA + (size_t)pairs[2 * pair] * nodes;
  const int *pb = PB + (size_t)pairs[2 * pair + 1] * nodes;
  unsigned *K = reinterpret_cast<unsigned *>(lds);  // [ni] kids: first child + 1 << 16 | second child + 1
  unsigned *MM = K + ni;                            // [ni] B: min rank << 16 | max rank        } the same
  u16 *SZA = reinterpret_cast<u16 *>(MM);           // [ni] A: leaves of the clade              } 4 ni
  u16 *UA = SZA + ni;                               // [ni] A: parent, then left end            } bytes
  u16 *SZB = UA + ni;                               // [ni] B: leaves of the clade
  u16 *RANK = SZB + ni;                             // [N]  rank of a leaf in A's depth-first order
  u16 *TAB = RANK + N;                              // [N]  A's intervals: at r the l of a first child, at l the r of a second
  const int lane = threadIdx.x & 63;
  const bool wave0 = threadIdx.x < 64;

  // ---- 1
  for (int i = threadIdx.x; i < N; i += T) TAB[i] = 0xffff;
  if (!build_kids<T>(pa, N, K, UA, &bad)) {
    if (threadIdx.x == 0) out[pair] = -1;
    return;
  }
  // ---- 2, 3
  if (wave0) {
    wave_clade_sizes(K, N, SZA, lane);
    wave_left_ends(K, SZA, UA, N, lane, [&](int i, unsigned lo, bool second, bool root) {
      if (!root) {
        const unsigned r = lo + SZA[i] - 1u;
        if (second) TAB[lo] = (u16)r;
        else TAB[r] = (u16)lo;
      }
    });
  }
  __syncthreads();
  // ---- 4
  for (int v = threadIdx.x; v < N; v += T) {
    const int pi = pa[v] - N;
    const int c1 = (int)(K[pi] >> 16) - 1;
    RANK[v] = (u16)(UA[pi] + (c1 != v ? (c1 < N ? 1u : (unsigned)SZA[c1 - N]) : 0u));
  }
  __syncthreads();
  // ---- 5
  if (!build_kids<T>(pb, N, K, nullptr, &bad)) {
    if (threadIdx.x == 0) out[pair] = -2;
    return;
  }
  if (!wave0) return;
  int common = 0;
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;
    unsigned s1 = 0, s2 = 0, m1 = 0, m2 = 0;  // size and min << 16 | max of the children that are known already
    if (act) {
      const unsigned k = K[i];
      const int c1 = (int)(k >> 16) - 1, c2 = (int)(k & 0xffffu) - 1;
      if (c1 < N) {
        s1 = 1;
        m1 = (unsigned)RANK[c1] * 0x10001u;
      } else if (c1 - N < b) {
        s1 = SZB[c1 - N];
        m1 = MM[c1 - N];
      } else {
        d1 = c1 - N - b;
      }
      if (c2 < N) {
        s2 = 1;
        m2 = (unsigned)RANK[c2] * 0x10001u;
      } else if (c2 - N < b) {
        s2 = SZB[c2 - N];
        m2 = MM[c2 - N];
      } else {
        d2 = c2 - N - b;
      }
    }
    unsigned sz = 0, mm = 0;
    bool done = !act;
    for (;;) {
      const unsigned long long dm = __ballot(done);
      if (dm == ~0ull) break;
      const int l1 = d1 < 0 ? 0 : d1, l2 = d2 < 0 ? 0 : d2;
      const unsigned t1 = __shfl(sz, l1, 64), t2 = __shfl(sz, l2, 64);
      const unsigned u1 = __shfl(mm, l1, 64), u2 = __shfl(mm, l2, 64);
      if (!done && (d1 < 0 || ((dm >> d1) & 1)) && (d2 < 0 || ((dm >> d2) & 1))) {
        const unsigned a = d1 < 0 ? m1 : u1, c = d2 < 0 ? m2 : u2;
        sz = (d1 < 0 ? s1 : t1) + (d2 < 0 ? s2 : t2);
        mm = (min(a >> 16, c >> 16) << 16) | max(a & 0xffffu, c & 0xffffu);
        done = true;
      }
    }
    if (act) {
      SZB[i] = (u16)sz;
      MM[i] = mm;
      const unsigned l = mm >> 16, r = mm & 0xffffu;
      if (i != ni - 1 && r - l + 1u == sz && (TAB[l] == r || TAB[r] == l)) common++;
    }
  }
  // ---- 6
  for (int o = 32; o > 0; o >>= 1) common += __shfl_xor(common, o, 64);
  if (lane == 0) out[pair] = 2 * (N - 2 - common);
}

static size_t compare_lds_bytes(int N) { return ((size_t)14 * N + 15) & ~(size_t)15; }

template <int T>
static hipError_t launch_clade_distance(const int *PA, const int *PB, int N, int npairs, const int *pairs, int *out,
                                        hipStream_t stream) {
  const size_t dyn = compare_lds_bytes(N);
  const void *fn = reinterpret_cast<const void *>(&clade_distance_kernel<T>);
  if (dyn > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(clade_distance_kernel<T>, dim3(npairs), dim3(T), dyn, stream, PA, PB, N, npairs, pairs, out);
  return hipGetLastError();
}

int compare_trees_device(const int *parentsA, int treesA, const int *parentsB, int treesB, int N, int npairs,
                         const int *pairs, int device, int *out) {
  if (N < 2 || N > kCompareMaxN) {
    set_error("rl_compare_trees: the device compares trees of 2 <= N <= %d leaves (N=%d); device < 0 selects the host", kCompareMaxN, N);
    return RL_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    set_error("no usable HIP device");
    return RL_ENODEVICE;
  }
  if (device >= ndev) {
    set_error("rl_compare_trees: device %d of %d", device, ndev);
    return RL_ENODEVICE;
  }
  RL_HIP(hipSetDevice(device));
  const size_t nodes = (size_t)2 * N - 1;
  DevBuf dA, dB, dP, dO;
  int rc = dA.alloc((size_t)treesA * nodes * sizeof(int));
  rc = rc ? rc : dB.alloc((size_t)treesB * nodes * sizeof(int));
  rc = rc ? rc : dP.alloc((size_t)npairs * 2 * sizeof(int));
  rc = rc ? rc : dO.alloc((size_t)npairs * sizeof(int));
  if (rc) return rc;
  RL_HIP(hipMemcpy(dA.p, parentsA, (size_t)treesA * nodes * sizeof(int), hipMemcpyHostToDevice));
  RL_HIP(hipMemcpy(dB.p, parentsB, (size_t)treesB * nodes * sizeof(int), hipMemcpyHostToDevice));
  RL_HIP(hipMemcpy(dP.p, pairs, (size_t)npairs * 2 * sizeof(int), hipMemcpyHostToDevice));
  if (N <= kCompareSmallN) RL_HIP(launch_clade_distance<64>(dA.as<int>(), dB.as<int>(), N, npairs, dP.as<int>(), dO.as<int>(), nullptr));
  else RL_HIP(launch_clade_distance<256>(dA.as<int>(), dB.as<int>(), N, npairs, dP.as<int>(), dO.as<int>(), nullptr));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(out, dO.p, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost));
  return RL_OK;
}

}  // namespace rl
