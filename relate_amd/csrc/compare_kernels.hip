// compare_kernels.hip -- CompareTopology on the device: the clade (rooted Robinson-Foulds) distance of pairs of trees.
//
// clade_distance_kernel: one workgroup per pair (tree a of batch A, tree b of batch B), Day's algorithm as in the host
// implementation (compare.cpp has the definition and why one table of N entries is enough), in integers, all tables
// of the pair in LDS.  Trees come as parent arrays with labels rising from child to parent; the kernel checks that
// itself (and that the tree is binary) before it uses a label as an index, and answers -1 (tree A) or -2 (tree B)
// for the pair instead of a distance when it does not hold.
//
// Steps of a pair (T threads; "wave 0" steps run on the first wavefront while the others wait at the barrier).  Steps 1
// to 3 are the passes of tree_passes.h, which documents the kids words and the pull scan (wave_pull) and which
// PairwiseCoalescence runs as well:
//   1. kids of A, all threads (build_kids);
//   2. sizes of A's clades, wave 0 (wave_clade_sizes);
//   3. left ends of A's intervals, wave 0 (wave_left_ends); the lane writes its table entry as it goes;
//   4. ranks of the leaves, all threads;
//   5. kids of B (in the words A's kids had), then (size, min rank << 16 | max rank) of B's clades, wave 0, the pull
//      scan of step 2 on a SizeSpan, each lane testing its own node against the table when it is done;
//   6. d = 2 (N - 2 - common).
//
// LDS, bytes, ni = N-1: kids 4 ni | A: sizes 2 ni, parent / left end 2 ni; B: min << 16 | max 4 ni (the same 4 ni) |
// B sizes 2 ni | ranks 2 N | table 2 N = 14 N - 10: 140 KB at N = 10,000 of the 160 KB a CU has, one pair per CU;
// labels and ranks fit 16 bits up to N = 10,240 (kMaxN), sizes too.  DESIGN.md 8c has the resource table.
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
    RANK[v] = (u16)leaf_rank(K, SZA, N, v, pi, UA[pi]);
  }
  __syncthreads();
  // ---- 5
  if (!build_kids<T>(pb, N, K, nullptr, &bad)) {
    if (threadIdx.x == 0) out[pair] = -2;
    return;
  }
  if (!wave0) return;
  int common = 0;
  const auto leaf = [&](int c) { return SizeSpan{1u, (unsigned)RANK[c] * 0x10001u}; };
  const auto table = [&](int j) { return SizeSpan{SZB[j], MM[j]}; };
  for (int b = 0; b < ni; b += 64) {
    const int i = b + lane;
    const bool act = i < ni;
    int d1 = -1, d2 = -1;
    SizeSpan k1{0u, 0u}, k2{0u, 0u};  // the children that are known already
    if (act) {
      d1 = child_source(first_child(K, i), N, b, &k1, leaf, table);
      d2 = child_source(second_child(K, i), N, b, &k2, leaf, table);
    }
    const SizeSpan s = wave_pull<2>(act, d1, k1, d2, k2, [](SizeSpan a, SizeSpan c) {
      const unsigned lo = min(a.mm >> 16, c.mm >> 16), hi = max(a.mm & 0xffffu, c.mm & 0xffffu);
      return SizeSpan{a.sz + c.sz, (lo << 16) | hi};
    });
    if (act) {
      SZB[i] = (u16)s.sz;
      MM[i] = s.mm;
      const unsigned l = s.mm >> 16, r = s.mm & 0xffffu;
      if (i != ni - 1 && r - l + 1u == s.sz && (TAB[l] == r || TAB[r] == l)) common++;
    }
  }
  // ---- 6
  for (int o = 32; o > 0; o >>= 1) common += __shfl_xor(common, o, 64);
  if (lane == 0) out[pair] = 2 * (N - 2 - common);
}

static size_t compare_lds_bytes(int N) { return ((size_t)14 * N + 15) & ~(size_t)15; }

int compare_trees_device(const int *parentsA, int treesA, const int *parentsB, int treesB, int N, int npairs,
                         const int *pairs, int device, int *out) {
  if (N < 2 || N > kCompareMaxN) {
    set_error("rl_compare_trees: the device compares trees of 2 <= N <= %d leaves (N=%d); device < 0 selects the host", kCompareMaxN, N);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_compare_trees", device)) return rc;
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
  const size_t dyn = compare_lds_bytes(N);
  if (N <= kCompareSmallN) RL_HIP(launch_with_lds(clade_distance_kernel<64>, npairs, 64, dyn, nullptr, dA.as<int>(), dB.as<int>(), N, npairs, dP.as<int>(), dO.as<int>()));
  else RL_HIP(launch_with_lds(clade_distance_kernel<256>, npairs, 256, dyn, nullptr, dA.as<int>(), dB.as<int>(), N, npairs, dP.as<int>(), dO.as<int>()));
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(out, dO.p, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost));
  return RL_OK;
}

}  // namespace rl
