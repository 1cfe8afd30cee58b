// frequency_kernels.hip -- Frequency on the device: for every SNP that maps to one branch b of its tree, the number of
// lineages and of carriers of the derived allele at every epoch boundary (include/relate_amd.h has the definition;
// frequency.cpp is the reference's walk on one host thread and the authority for trees with tied times).
//
// frequency_kernel, one workgroup per tree of a batch:
//   1. the passes of tree_passes.h: kids with the validity checks, then wavefront 0 takes the clade sizes and the
//      left ends of the depth-first intervals while wavefront 1 takes the times of Tree::GetCoordinates (the maximum
//      over both children, rounded to float at every node);
//   2. the descending order of the N-1 internal times: a bitonic sort of the 16-bit labels, padded to a power of two
//      P, by the key (time, label) read through the label -- O(P log^2 P) compare-exchanges, none quadratic.  Two
//      neighbours with equal times, or a time <= 0, set the tree's flag to "needs the host" and the tree's rows stay
//      unwritten: the closed form below is established for tie-free trees only;
//   3. from the order: rank[u] of every internal node, and above[e] = |{u : t(u) > ep[e]}| by binary search;
//   4. per SNP of the tree: the internal nodes of the subtree S of b are those whose interval lies inside b's; the
//      threads stride over the N-1 nodes, add 1 to the bin (E + 1 of them) of the node's epoch index |{e : ep[e] <
//      t(u)}| -- found by binary search of rank[u] in above[] -- and set the node's bit in a bitmap over ranks.
//      Integer atomics only: one value whatever the order.  Then, per boundary e, written from the oldest to 0,
//        lineages = 0 if t(root) < ep[e], else 1 + above[e]
//        carriers = 0 if t(root) < ep[e] or t(parent(b)) <= ep[e] (rank[parent] >= above[e]), else 1 + the bins past e
//      and, with DAF the leaves below b and h = (DAF + 1) / 2: when_DAF_is_half = 2 + the rank of the (h-1)-th set bit
//      of the bitmap (a popcount scan over one wavefront), -1 if h <= 1; when_mutation_has_freq2 = 2 + rank[b], -1
//      for a leaf.
// No scratch, no floating-point accumulation.
//
// LDS per workgroup, bytes, ni = N - 1 and P the power of two at or above ni (2 P <= 4 ni):
//   kids 4 ni, after the passes the sorted labels 2 P | times 4 ni, after the sort the ranks 2 ni | parents, then left
//   ends 2 ni | clade sizes 2 ni | bitmap 4 ceil(ni / 32)         = 12.125 ni: 124.2 KB at N = 10,240, 12.1 KB at
//   N = 1000, of a CU's 160 KB; static: boundaries, above[], bins, flags, under 1 KB.  One workgroup per CU above
//   N = 6,750, two above N = 4,500.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <vector>

#include "common.h"
#include "frequency.h"
#include "tree_passes.h"

namespace rl {

constexpr int kFrequencySmallN = 2048;  // up to here a workgroup is 256 threads, above 1024

// label a sorts before label b: the larger time first, the padding (0xffff) last
__device__ inline bool frequency_before(const float *TM, unsigned a, unsigned b) {
  if (a == 0xffffu || b == 0xffffu) return a != 0xffffu && b == 0xffffu;
  const float ta = TM[a], tb = TM[b];
  return ta > tb || (ta == tb && a > b);
}

template <int T>
__global__ void __launch_bounds__(T) frequency_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                      const float *__restrict__ EP, int E, int N, int ntrees,
                                                      const int *__restrict__ SNP_FIRST,
                                                      const int *__restrict__ SNP_BRANCH, int *__restrict__ OUT,
                                                      float *__restrict__ ROOT, int *__restrict__ FLAG) {
  static_assert(T >= 128, "wavefront 1 has work of its own");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad, tied;
  __shared__ float ep[kFrequencyMaxEpochs];
  __shared__ int above[kFrequencyMaxEpochs];               // internal nodes with t > ep[e]
  __shared__ unsigned char root_below[kFrequencyMaxEpochs];  // t(root) < ep[e]
  __shared__ int bins[kFrequencyMaxEpochs + 1];
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int P = 1;
  while (P < ni) P <<= 1;
  const int words = (ni + 31) / 32;
  const int *par = PAR + (size_t)t * nodes;
  const double *bl = BL + (size_t)t * nodes;
  unsigned *K = reinterpret_cast<unsigned *>(lds);                     // [ni] kids
  u16 *IDX = reinterpret_cast<u16 *>(lds);                             // [P] labels by falling time, once K is done with
  float *TM = reinterpret_cast<float *>(lds + (size_t)4 * ni);         // [ni] times
  u16 *RANK = reinterpret_cast<u16 *>(lds + (size_t)4 * ni);           // [ni] ranks, once TM is done with
  u16 *U = reinterpret_cast<u16 *>(lds + (size_t)8 * ni);              // [ni] parent, then left end
  u16 *SZ = U + ni;                                                    // [ni] leaves of the clade
  unsigned *BM = reinterpret_cast<unsigned *>(lds + (((size_t)12 * ni + 3) & ~(size_t)3));  // [words] ranks of S

  if (tid < E) ep[tid] = EP[tid];
  if (tid == 0) tied = 0;
  if (!checked_kids<T>(par, bl, nodes - 1, N, K, U, &bad)) {
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }
  if (wave == 0) {
    wave_clade_sizes(K, N, SZ, lane);
    wave_left_ends(K, SZ, U, N, lane, [](int, unsigned, bool, bool) {});
  } else if (wave == 1) {
    wave_max_times(K, bl, N, TM, lane);
  }
  __syncthreads();  // K is done with

  for (int i = tid; i < P; i += T) IDX[i] = (u16)(i < ni ? i : 0xffff);
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += T) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned a = IDX[i], b = IDX[l];
          const bool falling = (i & k) == 0;  // this stretch ends up in the order of frequency_before
          if (falling ? frequency_before(TM, b, a) : frequency_before(TM, a, b)) {
            IDX[i] = (u16)b;
            IDX[l] = (u16)a;
          }
        }
      }
      __syncthreads();
    }
  for (int r = tid; r < ni; r += T) {
    const float x = TM[IDX[r]];
    if (!(x > 0.0f) || (r + 1 < ni && x == TM[IDX[r + 1]])) tied = 1;
  }
  const float root_time = TM[ni - 1];
  if (tid < E) {
    const float e = ep[tid];
    int lo = 0, hi = ni;  // the first rank whose time is not above e
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (TM[IDX[mid]] > e) lo = mid + 1;
      else hi = mid;
    }
    above[tid] = lo;
    root_below[tid] = root_time < e;
  }
  if (tid == 0) ROOT[t] = root_time;
  __syncthreads();  // TM is done with
  if (tied) {
    if (tid == 0) FLAG[t] = kTreeNeedsHost;
    return;
  }
  for (int r = tid; r < ni; r += T) RANK[IDX[r]] = (u16)r;
  __syncthreads();

  const int width = 2 * E + 2;
  for (int s = SNP_FIRST[t]; s < SNP_FIRST[t + 1]; s++) {
    const int b = SNP_BRANCH[s];
    if (b < 0 || b >= nodes - 1) continue;  // no row (the same for every thread)
    const bool inner = b >= N;
    const int parent_rank = RANK[par[b] - N];  // (build_kids has checked the parent)
    const unsigned lo = inner ? U[b - N] : 0u, hi = inner ? lo + SZ[b - N] : 0u;
    const int daf = inner ? SZ[b - N] : 1, h = (daf + 1) / 2;
    for (int i = tid; i <= E; i += T) bins[i] = 0;
    for (int i = tid; i < words; i += T) BM[i] = 0u;
    __syncthreads();
    if (inner)
      for (int i = tid; i < ni; i += T) {
        const unsigned l = U[i];
        if (l >= lo && l + SZ[i] <= hi) {
          const int r = RANK[i];
          int x = 0, y = E;  // the boundaries below t(u): those with above[e] > rank
          while (x < y) {
            const int mid = (x + y) >> 1;
            if (above[mid] > r) x = mid + 1;
            else y = mid;
          }
          atomicAdd(&bins[x], 1);
          atomicOr(&BM[r >> 5], 1u << (r & 31));
        }
      }
    __syncthreads();
    int *row = OUT + (size_t)s * width;
    if (tid < E) {
      const int e = tid;
      int inside = 0;  // nodes of S above the boundary
      for (int i = e + 1; i <= E; i++) inside += bins[i];
      row[E - 1 - e] = root_below[e] || parent_rank >= above[e] ? 0 : 1 + inside;
      row[E + E - 1 - e] = root_below[e] ? 0 : 1 + above[e];
    } else if (wave == 1) {
      if (lane == 0) row[2 * E + 1] = inner ? 2 + (int)RANK[b - N] : -1;
      if (h <= 1) {
        if (lane == 0) row[2 * E] = -1;
      } else {
        // the (h-1)-th set bit: a lane takes `chunk` words, the wavefront scans the popcounts, one lane walks its words
        const int chunk = (words + 63) / 64, w0 = min(lane * chunk, words), w1 = min(w0 + chunk, words);
        int mine = 0;
        for (int w = w0; w < w1; w++) mine += __popc(BM[w]);
        int upto = mine;
        for (int o = 1; o < 64; o <<= 1) {
          const int y = __shfl_up(upto, o, 64);
          if (lane >= o) upto += y;
        }
        int left = h - 1 - (upto - mine);  // still to count when this lane's words begin
        if (left >= 1 && left <= mine)
          for (int w = w0; w < w1; w++) {
            unsigned bits = BM[w];
            const int c = __popc(bits);
            if (left > c) {
              left -= c;
              continue;
            }
            for (; left > 1; left--) bits &= bits - 1u;
            row[2 * E] = 2 + w * 32 + (__ffs(bits) - 1);
            break;
          }
      }
    }
    __syncthreads();  // the bins and the bitmap are rewritten by the next SNP
  }
}

int frequency_device(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_first,
                     const int *snp_branch, int nsnps, const float *epochs, int E, int device, int *out,
                     float *root_time, int *flags) {
  if (N < 2 || N > kFrequencyMaxN) {
    set_error("rl_frequency_trees: the device takes trees of 2 <= N <= %d leaves (N=%d); device < 0 selects the host", kFrequencyMaxN, N);
    return RL_EINVAL;
  }
  if (E < 2 || E > kFrequencyMaxEpochs) {
    set_error("rl_frequency_trees: 2 <= epochs <= %d (%d given)", kFrequencyMaxEpochs, E);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_frequency_trees", device)) return rc;
  const size_t ni = (size_t)N - 1, width = (size_t)2 * E + 2;
  const int B = frequency_batch_trees(N);
  const size_t dyn = round16(((12 * ni + 3) & ~(size_t)3) + 4 * ((ni + 31) / 32));
  size_t most = 0;  // SNPs of one batch
  for (int t0 = 0; t0 < ntrees; t0 += B) most = std::max(most, (size_t)(snp_first[std::min(ntrees, t0 + B)] - snp_first[t0]));
  DevBuf ep, first, branch, rows, root;
  TreeBatch tb;
  int rc = ep.alloc((size_t)E * 4);
  rc = rc ? rc : tb.alloc(N, B);
  rc = rc ? rc : first.alloc(((size_t)B + 1) * 4);
  rc = rc ? rc : branch.alloc(most * 4);
  rc = rc ? rc : rows.alloc(most * width * 4);
  rc = rc ? rc : root.alloc((size_t)B * 4);
  if (rc) return rc;
  RL_HIP(hipMemcpy(ep.p, epochs, (size_t)E * 4, hipMemcpyHostToDevice));
  std::vector<int> rebased((size_t)B + 1);
  for (int t0 = 0; t0 < ntrees; t0 += B) {
    const int n = std::min(B, ntrees - t0), s0 = snp_first[t0], ns = snp_first[t0 + n] - s0;
    for (int k = 0; k <= n; k++) rebased[k] = snp_first[t0 + k] - s0;
    RL_HIP(hipMemcpy(first.p, rebased.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    if (ns) RL_HIP(hipMemcpy(branch.p, snp_branch + s0, (size_t)ns * 4, hipMemcpyHostToDevice));
    if ((rc = tb.upload(parents, branch_length, t0, n))) return rc;
    if (ns) RL_HIP(hipMemset(rows.p, 0, (size_t)ns * width * 4));
    RL_HIP(hipMemset(root.p, 0, (size_t)n * 4));
    const auto go = [&](auto kernel, int threads) {
      return launch_with_lds(kernel, n, threads, dyn, nullptr, tb.par.as<int>(), tb.bl.as<double>(), ep.as<float>(), E, N, n,
                             first.as<int>(), branch.as<int>(), rows.as<int>(), root.as<float>(), tb.flag.as<int>());
    };
    RL_HIP(N <= kFrequencySmallN ? go(frequency_kernel<256>, 256) : go(frequency_kernel<1024>, 1024));
    // (the copies wait for the kernel)
    if (ns) RL_HIP(hipMemcpy(out + (size_t)s0 * width, rows.p, (size_t)ns * width * 4, hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(root_time + t0, root.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if ((rc = tb.download(n))) return rc;
    std::copy(tb.flags.begin(), tb.flags.begin() + n, flags + t0);
  }
  return RL_OK;
}

}  // namespace rl
