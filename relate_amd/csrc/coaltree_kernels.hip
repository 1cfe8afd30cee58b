// coaltree_kernels.hip -- CoalRateForTree on the device: the coalescence counts and the pair opportunity of every
// block of trees in every epoch (include/relate_amd.h has the definition; coaltree.cpp restates the reference's
// coal_tree::populate on one host thread and is the authority these kernels are held to, bit for bit).
//
// The reference walks the 2N-1 sorted node times of a tree with an epoch cursor and adds every term straight onto the
// accumulators of the current block of trees: one serial double chain per (block, epoch) through all the block's
// trees.  Here the terms are formed in parallel and only the additions are serial.  With S the sorted times of the
// internal nodes, S[-1] = 0 and ep the boundaries:
//   node k lies in epoch j, ep[j] < S[k] <= ep[j+1] (a node at time 0 in epoch 0; one above ep[E-1] in none), and adds
//     term(N - k, S[k] - max(S[k-1], ep[j])) to denom[j] and bases/1e9 to num[j];
//   epoch j gets an exit term once a node time exceeds ep[j+1]: with k* the first such node,
//     term(N - k*, ep[j+1] - max(S[k*-1], ep[j])), added after the epoch's node terms;
//   term(n, w) = bases * n * (n-1) / 2.0 * w / 1e9, every operation in double and left to right.
// Tied times give w = 0 and a term of +0 whatever the walk's lineage count is there; every term is >= +0, so an
// absent one is stored as +0.0 and added without changing a bit.
//
// coaltree_terms_kernel, one workgroup per tree of a batch: sorted_max_times of tree_passes.h (the checks, the times
//   of Tree::GetCoordinates, the in-place sort), then ALL threads: thread k finds j(k) by binary search over the
//   boundaries in LDS and writes the node term T[k]; the first E threads find by binary search over S the first node
//   and the node count of their epoch and form the exit term X[j].  LDS as in mutrate_kernels.hip: 8 bytes per
//   internal node, 80 KB at N = 10,240; static: the boundaries and a flag.
// coaltree_chains_kernel, one workgroup per block of trees that the batch touches; one wavefront of it holds the
//   chains, lane j those of epoch j: it loads num[j] and denom[j] of the block, goes through the batch's trees of
//   that block in tree order -- bases/1e9 cnt[j] times onto num, the cnt[j] node terms one by one and then X[j] onto
//   denom -- and stores both.  A tree's terms go through LDS (8 bytes per internal node): all four wavefronts bring
//   them in, coalesced, then every lane of the first reads its own range.  The accumulators stay in device memory
//   between launches, so batches need not align with blocks.
// T, first, cnt and X never leave the device.  No scratch, no atomics on doubles, every product, sum and quotient a
// separate operation (-ffp-contract=off; the double division is IEEE's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "coaltree.h"
#include "common.h"
#include "tree_passes.h"

namespace rl {

constexpr int kCoaltreeSmallN = 2048;  // up to here a workgroup is 256 threads, above 1024

// coal_tree.cpp:166, :174: `bases * n * (n-1)/2.0 * width/1e9`
__device__ inline double pair_term(double bases, int n, double width) {
  return bases * (double)n * (double)(n - 1) / 2.0 * width / 1e9;
}

// how many of the sorted times are at or below x
__device__ inline int times_up_to(const float *S, int ni, double x) {
  int lo = 0, hi = ni;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)S[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <int T>
__global__ void __launch_bounds__(T) coaltree_terms_kernel(const int *__restrict__ PAR, const double *__restrict__ BL,
                                                           const float *__restrict__ F, const double *__restrict__ EP,
                                                           int E, int N, int ntrees, double *__restrict__ TERM,
                                                           int *__restrict__ FIRST, int *__restrict__ CNT,
                                                           double *__restrict__ EXIT, int *__restrict__ FLAG) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int bad;
  __shared__ double ep[kCoaltreeMaxEpochs];
  const int t = blockIdx.x;
  if (t >= ntrees) return;
  const int nodes = 2 * N - 1, ni = N - 1, tid = threadIdx.x;
  const int *par = PAR + (size_t)t * nodes;
  const double *bl = BL + (size_t)t * nodes;
  unsigned *K = reinterpret_cast<unsigned *>(lds);             // [ni] kids
  float *S = reinterpret_cast<float *>(lds + (size_t)4 * ni);  // [ni] times, sorted ascending by the prologue

  if (tid < E) ep[tid] = EP[tid];
  if (!sorted_max_times<T>(par, bl, N, K, S, &bad)) {
    if (tid == 0) FLAG[t] = kTreeRefused;
    return;
  }
  const double bases = (double)F[t];

  // ---- one thread per internal node
  for (int k = tid; k < ni; k += T) {
    const double s = (double)S[k], prev = k ? (double)S[k - 1] : 0.0;
    int lo = 1, hi = E;  // the first boundary from 1 on that is not below s: s lies in the epoch before it
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ep[mid] < s) lo = mid + 1;
      else hi = mid;
    }
    double term = 0.0;  // (above the last boundary: in no epoch, never read)
    if (lo < E) {
      const double from = ep[lo - 1], lower = prev > from ? prev : from;
      term = pair_term(bases, N - k, s - lower);
    }
    TERM[(size_t)t * ni + k] = term;
  }
  if (tid >= E) return;

  // ---- one thread per epoch
  const int j = tid;
  const int a = j ? times_up_to(S, ni, ep[j]) : 0;  // (a node at time 0 lies in epoch 0)
  int b = a;
  double x = 0.0;
  if (j + 1 < E) {
    b = times_up_to(S, ni, ep[j + 1]);
    if (b < ni) {  // node b is the first above ep[j+1]: the walk leaves epoch j in front of it
      const double prev = b ? (double)S[b - 1] : 0.0, from = ep[j], lower = prev > from ? prev : from;
      x = pair_term(bases, N - b, ep[j + 1] - lower);
    }
  }
  FIRST[(size_t)t * E + j] = a;
  CNT[(size_t)t * E + j] = b - a;
  EXIT[(size_t)t * E + j] = x;
}

// trees g0 .. g0 + ntrees - 1 of the sequence are the batch; workgroup i takes block g0 / block_size + i.  Wavefront 0
// holds the chains, lane j those of epoch j.  The lanes' ranges of node terms lie one behind the other in T (first[j+1]
// = first[j] + cnt[j]), so the workgroup's four wavefronts bring the terms inside the boundaries into LDS with
// coalesced loads, tree by tree, and every lane of wavefront 0 walks its range there: a load instruction whose 64
// lanes want 64 different cache lines costs a multiple of one LDS read.
constexpr int kChainsThreads = 256;
__global__ void __launch_bounds__(kChainsThreads)
    coaltree_chains_kernel(const double *__restrict__ TERM, const int *__restrict__ FIRST, const int *__restrict__ CNT,
                           const double *__restrict__ EXIT, const float *__restrict__ F, int E, int ni, int ntrees,
                           long long g0, int block_size, double *__restrict__ NUM, double *__restrict__ DEN) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double *tl = reinterpret_cast<double *>(lds);  // [ni] the node terms of the tree at hand
  const int tid = threadIdx.x, j = tid < E ? tid : E - 1;
  const bool own = tid < E;  // (the other threads only carry terms into LDS)
  const long long block = g0 / block_size + blockIdx.x;
  const long long lo = block * block_size - g0, hi = lo + block_size;
  const int ta = lo > 0 ? (int)lo : 0, tb = hi < ntrees ? (int)hi : ntrees;
  double nu = NUM[block * E + j], de = DEN[block * E + j];
  for (int t = ta; t < tb; t++) {
    const int used = FIRST[(size_t)t * E + E - 1];  // the nodes at or below the last boundary (cnt[E-1] = 0)
    const double *from = TERM + (size_t)t * ni;
    __syncthreads();  // (the tree before has been read)
#pragma unroll 4
    for (int i = tid; i < used; i += kChainsThreads) tl[i] = from[i];
    __syncthreads();
    if (tid >= 64) continue;
    const double q = (double)F[t] / 1e9;
    const int c = own ? CNT[(size_t)t * E + j] : 0;
    const double *term = tl + FIRST[(size_t)t * E + j];
    int i = 0;
    for (; i + 4 <= c; i += 4) {  // (four reads in flight; the additions stay one chain each)
      const double t0 = term[i], t1 = term[i + 1], t2 = term[i + 2], t3 = term[i + 3];
      nu += q;
      de += t0;
      nu += q;
      de += t1;
      nu += q;
      de += t2;
      nu += q;
      de += t3;
    }
    for (; i < c; i++) {
      nu += q;
      de += term[i];
    }
    de += EXIT[(size_t)t * E + j];
  }
  if (own) {
    NUM[block * E + j] = nu;
    DEN[block * E + j] = de;
  }
}

struct CoaltreeDevice {
  int N = 0, E = 0, device = 0, num_blocks = 0, block_size = 0;
  long long total = 0, added = 0;  // trees announced, trees added
  DevBuf ep, num, den, f, term, first, cnt, exit;
  TreeBatch trees;
};

int coaltree_device_begin(CoaltreeDevice **out, int N, const double *epochs, int E, long long ntrees, int block_size,
                          int device) {
  *out = nullptr;
  if (N < 2 || N > kCoaltreeMaxN) {
    set_error("rl_coaltree_trees: trees of 2 <= N <= %d leaves (N=%d)", kCoaltreeMaxN, N);
    return RL_EINVAL;
  }
  if (E < 2 || E > kCoaltreeMaxEpochs) {
    set_error("rl_coaltree_trees: 2 <= epochs <= %d (%d given)", kCoaltreeMaxEpochs, E);
    return RL_EINVAL;
  }
  if (const int rc = select_device("rl_coaltree_trees", device)) return rc;
  const size_t ni = (size_t)N - 1, B = (size_t)coaltree_batch_trees(N);
  CoaltreeDevice *d = new CoaltreeDevice;
  d->N = N, d->E = E, d->device = device, d->block_size = block_size, d->total = ntrees;
  d->num_blocks = coaltree_num_blocks(ntrees, block_size);
  const size_t acc = (size_t)d->num_blocks * E * 8;
  int rc = d->ep.alloc((size_t)E * 8);
  rc = rc ? rc : d->num.alloc(acc);
  rc = rc ? rc : d->den.alloc(acc);
  rc = rc ? rc : d->trees.alloc(N, (int)B);
  rc = rc ? rc : d->f.alloc(B * 4);
  rc = rc ? rc : d->term.alloc(B * ni * 8);
  rc = rc ? rc : d->first.alloc(B * E * 4);
  rc = rc ? rc : d->cnt.alloc(B * E * 4);
  rc = rc ? rc : d->exit.alloc(B * E * 8);
  if (rc) {
    delete d;
    return rc;
  }
  hipError_t e = hipMemset(d->num.p, 0, acc);
  if (e == hipSuccess) e = hipMemset(d->den.p, 0, acc);
  if (e == hipSuccess) e = hipMemcpy(d->ep.p, epochs, (size_t)E * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete d;
    set_error("rl_coaltree_trees: %s", hipGetErrorString(e));
    return RL_EHIP;
  }
  *out = d;
  return RL_OK;
}

int coaltree_device_add(CoaltreeDevice *d, const int *parents, const double *branch_length, const float *factors,
                        int ntrees, int *bad_tree) {
  *bad_tree = -1;
  if (d->added + ntrees > d->total) {  // (the chains index the accumulators by the tree's number)
    set_error("rl_coaltree_trees: %lld trees added to a sequence announced as %lld", d->added + ntrees, d->total);
    return RL_EINVAL;
  }
  RL_HIP(hipSetDevice(d->device));
  const int N = d->N, E = d->E, ni = N - 1, bs = d->block_size;
  const size_t dyn = round16((size_t)8 * ni);
  TreeBatch &tb = d->trees;
  for (int t0 = 0; t0 < ntrees; t0 += tb.batch) {
    const int n = std::min(tb.batch, ntrees - t0);
    RL_HIP(hipMemcpy(d->f.p, factors + t0, (size_t)n * 4, hipMemcpyHostToDevice));
    if (const int rc = tb.upload(parents, branch_length, t0, n)) return rc;
    const auto go = [&](auto kernel, int threads) {
      return launch_with_lds(kernel, n, threads, dyn, nullptr, tb.par.as<int>(), tb.bl.as<double>(), d->f.as<float>(),
                             d->ep.as<double>(), E, N, n, d->term.as<double>(), d->first.as<int>(), d->cnt.as<int>(),
                             d->exit.as<double>(), tb.flag.as<int>());
    };
    RL_HIP(N <= kCoaltreeSmallN ? go(coaltree_terms_kernel<256>, 256) : go(coaltree_terms_kernel<1024>, 1024));
    // Nothing of a batch is added unless all of its trees passed: the chains use first and cnt as indices, and a
    // refused tree leaves none
    int bad = -1;
    if (const int rc = tb.first_not_done(n, &bad)) return rc;
    if (bad >= 0) {
      *bad_tree = t0 + bad;
      return RL_EINVAL;
    }
    const long long g0 = d->added, first_block = g0 / bs, last_block = (g0 + n - 1) / bs;
    RL_HIP(launch_with_lds(coaltree_chains_kernel, (int)(last_block - first_block + 1), kChainsThreads, dyn, nullptr, d->term.as<double>(),
                           d->first.as<int>(), d->cnt.as<int>(), d->exit.as<double>(), d->f.as<float>(), E, ni, n, g0, bs,
                           d->num.as<double>(), d->den.as<double>()));
    RL_HIP(hipDeviceSynchronize());  // the next batch overwrites the arrays this one reads
    d->added += n;
  }
  return RL_OK;
}

int coaltree_device_finish(CoaltreeDevice *d, double *num, double *denom) {
  RL_HIP(hipSetDevice(d->device));
  RL_HIP(hipDeviceSynchronize());
  const size_t acc = (size_t)d->num_blocks * d->E * 8;
  RL_HIP(hipMemcpy(num, d->num.p, acc, hipMemcpyDeviceToHost));
  RL_HIP(hipMemcpy(denom, d->den.p, acc, hipMemcpyDeviceToHost));
  return RL_OK;
}

void coaltree_device_free(CoaltreeDevice *d) { delete d; }

}  // namespace rl
