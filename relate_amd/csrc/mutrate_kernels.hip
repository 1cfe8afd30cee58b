// mutrate_kernels.hip -- AvgMutationRate on the device: the branch length of every tree in every epoch
// (include/relate_amd.h has the definition; mutrate.cpp restates the reference's serial walk on one host thread and is
// the authority this kernel is held to, bit for bit).
//
// mutrate_kernel, one workgroup per tree of a batch:
//   1. the passes of tree_passes.h: kids with the validity checks, the branch-length sanity check, then wavefront 0
//      takes the times of Tree::GetCoordinates (wave_max_times);
//   2. the N-1 internal times sorted ascending IN PLACE by a bitonic network that moves values only: no labels, no
//      ranks (1 and 2 are sorted_max_times of tree_passes.h, which coaltree_kernels.hip begins with too);
//   3. one lane of wavefront 0 per epoch e.  With S the sorted times and S[-1] = 0, interval k is (S[k-1], S[k]] and
//      carries N - k lineages; an empty interval adds +0.  The lane finds by binary search the first k1 with S[k1] >
//      ep[e] and the first k2 with S[k2] >= ep[e+1], forms the term of interval k1 -- assigned as a double product
//      when the serial walk's cursor enters the epoch inside it, added as a float product when the cursor is there
//      already --, adds the float products of the intervals k1+1 .. k2-1 one by one in order, and the double exit
//      term of interval k2.  Where the cursor is when an interval starts exactly on ep[e] is the one thing that is
//      not local: the walk leaves the cursor at e-1 if it arrived on that boundary from below epoch e-1 (`lag`).
//      lag[j] depends on lag[j-1] only where two neighbouring boundaries are neighbouring node times, so the lanes
//      classify their boundary (no / yes / as the one before) and two ballots resolve the chain.
// No scratch, no atomics on doubles, every product and sum a separate operation (-ffp-contract=off).
//
// LDS per workgroup: kids 4 ni | times 4 ni, ni = N - 1: 80 KB at N = 10,240, 7.8 KB at N = 1000, of a CU's 160 KB;
// static: the boundaries and a flag, about 520 bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "mutrate.h"
#include "tree_passes.h"

namespace rl {

constexpr int kMutrateSmallN = 2048;  // up to here a workgroup is 256 threads, above 1024

template <int T>
__global__ void __launch_bounds__(T) mutrate_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                    const double *__restrict__ EP, int E, int N, int ntrees,
                                                    double *__restrict__ OUT, int *__restrict__ FLAG,
                                                    float *__restrict__ ROOT) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  __shared__ double ep[kMutrateMaxEpochs];
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int *par = PAR + (size_t)t * nodes;
  const double *bl = BL + (size_t)t * nodes;
  unsigned *K = reinterpret_cast<unsigned *>(lds);              // [ni] kids
  float *S = reinterpret_cast<float *>(lds + (size_t)4 * ni);   // [ni] times, sorted ascending after step 2

  if (tid < E) ep[tid] = EP[tid];
  if (!sorted_max_times<T>(par, bl, N, K, S, &bad)) {  // steps 1 and 2
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }
  // (MutationRateWithContext clamps a SNP's age_end to the root's time: the last of the sorted float times)
  if (ROOT && tid == 0) ROOT[t] = S[ni - 1];
  if (wave != 0 || lane >= E) return;

  // ---- one lane per epoch
  const int e = lane;
  const double L = ep[e];
  int p = 0;
  {
    int hi = ni;  // the first index whose time is not below L
    while (p < hi) {
      const int mid = (p + hi) >> 1;
      if ((double)S[mid] < L) p = mid + 1;
      else hi = mid;
    }
  }
  const int p_next = __shfl_down(p, 1, 64);  // (of boundary e + 1; every lane below E is here)
  // does the walk reach boundary e with its cursor still at e - 1?  0: no; 1: yes; 2: as at boundary e - 1
  int code = 0;
  if (e >= 1 && p < ni && (double)S[p] == L) {
    const float a = p ? S[p - 1] : 0.0f;  // the node time before L
    int f = 0, hi = e;                    // the last boundary at or below a (a < L: f < e)
    while (f + 1 < hi) {
      const int mid = (f + hi) >> 1;
      if (ep[mid] <= (double)a) f = mid;
      else hi = mid;
    }
    code = f < e - 1 ? 1 : ((double)a == ep[e - 1] && e - 1 >= 1 ? 2 : 0);
  }
  const unsigned long long yes = __ballot(code == 1), same = __ballot(code == 2);
  unsigned long long lag = 0;
  for (int j = 1; j < E; j++) lag |= (((yes >> j) | ((same >> j) & (lag >> (j - 1)))) & 1ull) << j;

  double acc = 0.0;
  if (e < E - 1) {
    const double H = ep[e + 1];
    int k1 = p, hi = ni;  // the first index whose time is above L
    while (k1 < hi) {
      const int mid = (k1 + hi) >> 1;
      if ((double)S[mid] <= L) k1 = mid + 1;
      else hi = mid;
    }
    const int k2 = p_next;
    if (k1 < ni) {
      const float a = k1 ? S[k1 - 1] : 0.0f, b = S[k1];
      const int n = N - k1;
      bool open = true;  // the cursor is still in this epoch after interval k1
      if ((double)a < L || ((lag >> e) & 1)) {  // the cursor enters the epoch inside interval k1
        if (H < (double)b) {
          acc = (double)n * (H - L);
          open = false;
        } else {
          acc = (double)n * ((double)b - L);  // (b == H: what follows adds +0)
        }
      } else if ((double)b < H) {
        acc += (double)((float)n * (b - a));
      } else {
        acc += (double)n * (H - (double)a);
        open = false;
      }
      if (open) {
        float prev = b;
        for (int k = k1 + 1; k < k2; k++) {
          const float x = S[k];
          acc += (double)((float)(N - k) * (x - prev));
          prev = x;
        }
        if (k2 > k1 && k2 < ni) acc += (double)(N - k2) * (H - (double)prev);
      }
    }
  }
  OUT[(size_t)t * E + e] = acc;
}

hipError_t mutrate_launch(const int *par, const double *bl, const double *ep, int E, int N, int n, double *rows, int *flag,
                          float *root) {
  const size_t dyn = round16(8 * ((size_t)N - 1));
  const auto go = [&](auto kernel, int threads) {
    return launch_with_lds(kernel, n, threads, dyn, nullptr, par, bl, ep, E, N, n, rows, flag, root);
  };
  return N <= kMutrateSmallN ? go(mutrate_kernel<256>, 256) : go(mutrate_kernel<1024>, 1024);
}

int mutrate_device(const int *parents, const double *branch_length, int N, int ntrees, const double *epochs, int E,
                   int device, double *out, int *flags) {
  if (N < 2 || N > kMutrateMaxN) {
    set_error("rl_mutrate_trees: trees of 2 <= N <= %d leaves (N=%d)", kMutrateMaxN, N);
    return RL_EINVAL;
  }
  if (E < 2 || E > kMutrateMaxEpochs) {
    set_error("rl_mutrate_trees: 2 <= epochs <= %d (%d given)", kMutrateMaxEpochs, E);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_mutrate_trees", device)) return rc;
  const int B = mutrate_batch_trees(N);
  DevBuf ep, rows;
  TreeBatch tb;
  int rc = ep.alloc((size_t)E * 8);
  rc = rc ? rc : tb.alloc(N, B);
  rc = rc ? rc : rows.alloc((size_t)B * E * 8);
  if (rc) return rc;
  RL_HIP(hipMemcpy(ep.p, epochs, (size_t)E * 8, hipMemcpyHostToDevice));
  for (int t0 = 0; t0 < ntrees; t0 += B) {
    const int n = std::min(B, ntrees - t0);
    if ((rc = tb.upload(parents, branch_length, t0, n))) return rc;
    RL_HIP(hipMemset(rows.p, 0, (size_t)n * E * 8));  // (after the copies: a copy behind a memset waits for it)
    RL_HIP(mutrate_launch(tb.par.as<int>(), tb.bl.as<double>(), ep.as<double>(), E, N, n, rows.as<double>(), tb.flag.as<int>(), nullptr));
    // (the copies wait for the kernel)
    RL_HIP(hipMemcpy(out + (size_t)t0 * E, rows.p, (size_t)n * E * 8, hipMemcpyDeviceToHost));
    if ((rc = tb.download(n))) return rc;
    std::copy(tb.flags.begin(), tb.flags.begin() + n, flags + t0);
  }
  return RL_OK;
}

}  // namespace rl
