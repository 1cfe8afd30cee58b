// minmatch_build.h -- MinMatch::QuickBuild on the GPU: one workgroup builds one tree, matrices in HBM.  Device code: the
// workers of minmatch_worker.hip instantiate it; the per-tree kernels of minmatch_builder.hip use its reductions.
// Reference: src/tree_builder.cpp (MinMatch, sample_ages empty): :59-146 / :1647-1735 (Initialize),
// :296-598 / :1844-2070 (Coalesce), :1061-1303 / :2358-2644 (QuickBuild).  The host builder
// (minmatch.cpp) states the algorithm and why a merge splits into a parallel part and an ordered part with
// identical results; this file is the same split on one workgroup:
//   * the N-1 merges of a tree are sequential and each walks down two columns of a 100 MB matrix -- a new
//     line per cluster: on a host dozens of open sections are bound by DRAM (DESIGN_NOTES.md 5), in HBM one
//     workgroup per tree leaves the other 255 CUs to the trees of the other sections;
//   * the parts that are order-free (distance updates, row-minimum rescans, candidate tests, reductions) run
//     on all 512 threads; the random draws -- one per feasible pair, in the reference's order -- and the
//     candidate bookkeeping run on wave 0 over lists the parallel parts leave in order;
//   * std::mt19937 (seed 1 per build) and libstdc++'s generate_canonical<double, 53> are restated below.
// The symmetric fallback (no mutually closest pair left, :255-293 / :968-1058) is here too: "the first cluster in
// scan order that reaches the minimum" is a lexicographic (value, position) reduction.  The state both builders
// carry from tree to tree (min_values_CF and the stale candidate indices, minmatch.h) is copied in before and
// out after every build, so host and device builders can alternate on a section.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "minmatch_params.h"

namespace rl {
namespace {

struct Rng {  // std::mt19937
  uint32_t mt[624];
  int idx;
};

__host__ __device__ inline void rng_seed(Rng &r, uint32_t seed) {
  r.mt[0] = seed;
  for (int i = 1; i < 624; i++) r.mt[i] = 1812433253u * (r.mt[i - 1] ^ (r.mt[i - 1] >> 30)) + (uint32_t)i;
  r.idx = 624;
}
__host__ __device__ inline uint32_t rng_next(Rng &r) {
  if (r.idx >= 624) {
    for (int i = 0; i < 624; i++) {
      const uint32_t y = (r.mt[i] & 0x80000000u) | (r.mt[(i + 1) % 624] & 0x7fffffffu);
      r.mt[i] = r.mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    r.idx = 0;
  }
  uint32_t y = r.mt[r.idx++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
// The state renewal of rng_next by one wavefront: word i takes the old words i, i+1 and word i+397 -- old for
// i < 227, already renewed (word i-227) behind that; 64 consecutive words per round, every lane reads before any
// lane writes, and a round never needs a word of its own round (227 > 64).  The last word takes the new word 0.
// (The lanes exchange words through LDS between rounds: to the compiler one thread's next-round loads are
// provably other words than its store and may move above it -- the fences pin the rounds.)
__device__ __noinline__ void rng_renew_wave(Rng &r, int lane) {
  for (int base = 0; base < 623; base += 64) {
    const int i = base + lane;
    uint32_t v = 0;
    if (i < 623) {
      const uint32_t y = (r.mt[i] & 0x80000000u) | (r.mt[i + 1] & 0x7fffffffu);
      v = r.mt[i < 227 ? i + 397 : i - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (i < 623) r.mt[i] = v;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    const uint32_t y = (r.mt[623] & 0x80000000u) | (r.mt[0] & 0x7fffffffu);
    r.mt[623] = r.mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// std::uniform_real_distribution<double>(0,1)(rng) of libstdc++: generate_canonical<double, 53> = two draws,
// sum = g1 + g2 * 2^32 in double, / 2^64, a result of 1 replaced by nextafter(1, 0)
__host__ __device__ inline double rng_unif(Rng &r) {
  const double g1 = (double)rng_next(r);
  const double g2 = (double)rng_next(r);
  const double sum = g1 + g2 * 4294967296.0;
  double ret = sum / 18446744073709551616.0;
  if (ret >= 1.0) ret = 0.99999999999999988897769753748434595763683319091796875;
  return ret;
}

struct Best {
  float dist, dist2;
  int lin1, lin2;
};

constexpr int MM_ROWS_MAX = 2;       // rows of rebuilt clusters a pass of a merge scans at most (build_tree: ROWS; 3: 119 ms per N = 5000 tree, 2: 110, 4: 134)
struct Shared {
  unsigned praw[MM_PARAM_WORDS];  // the tree's parameters as the worker read them from the queue
  unsigned ticket;
  int sym_slot;
  long long tacc[16], tmark;
  int cnt_rescan_only;  // (statistics, RELATE_AMD_TIMING) rebuilt clusters of the merge whose candidate does not touch i or j
  Rng rng;
  Best best, best_sym;
  int use_sym;
  int n, ipos;
  int count;
  int nupd, npairs;
  int wave_i[MM_WAVES];
  float wave_f[MM_WAVES];
  int wave_i2[MM_WAVES];
  int wave_i3[MM_WAVES];
  float wave_f2[MM_WAVES];
  float lex_d[MM_WAVES], lex_d2[MM_WAVES];
  int lex_p[MM_WAVES], lex_k[MM_WAVES];
  double lex_d2d[MM_WAVES];  // (the AGES build: the draw is a double)
  int a_lw;                  // ... and the last age level its clock has reached, for all waves
  int rowcount[MM_WAVES];
  float sym_dist;
  float red_f[MM_ROWS_MAX][MM_WAVES];
  int red_a[MM_ROWS_MAX][MM_WAVES], red_b[MM_ROWS_MAX][MM_WAVES];
  // the live list lives in the threads' registers (position t + 512 q in slot q of thread t): when a cluster leaves,
  // the positions behind it move up by one -- a lane takes its neighbour's, the last lane of a wave the first of the
  // next wave's from here
  short edge[MM_WAVES][MM_Q_GLOB];
  // rebuilt clusters of the merge, any order: position | cluster << 14 | rescan << 28; their new d(k, j), which is not
  // in memory until the end of the merge; their row minimum (+ threshold), as it was and then as the rescan leaves it
  unsigned upd[MM_UPD_LDS];
  float updv[MM_UPD_LDS];
  float updmv[MM_UPD_LDS];
  // feasible pairs of the merge, [0]: as found, [1]: in the reference's order
  unsigned pk[2][MM_PAIRS_LDS];   // key: position of the later cluster << 16 | position of the earlier one
  unsigned pxy[2][MM_PAIRS_LDS];  // later cluster << 16 | earlier cluster
  float psym[2][MM_PAIRS_LDS];    // symmetric distance of the pair (0 if the prior makes it a certain pair)
};

// The per-cluster state of a build and where each field lives (L_LDS / L_GLOBAL / L_HOT above).  HOT fields: read or
// written for every cluster of every merge from LDS or on the ordered part's path; COLD fields: read with the rows of
// a merge (row minima), by a few threads (sizes, min_values_CF of a pair) or from registers (the live list: `ci` is its
// mirror in memory, kept for the symmetric fallback and the AGES walk).
template <int LAY>
struct State {
  static constexpr bool hot_lds = LAY != L_GLOBAL, cold_lds = LAY == L_LDS, warm_lds = LAY == L_LDS || LAY == L_WARM;
  typedef typename std::conditional<hot_lds, short, int>::type hidx_t;
  typedef typename std::conditional<cold_lds, short, int>::type cidx_t;
  template <typename T>
  using hot = typename std::conditional<hot_lds, T *, MM_GLOBAL_PTR(T)>::type;  // (LDS: inferred)
  template <typename T>
  using warm = typename std::conditional<warm_lds, T *, MM_GLOBAL_PTR(T)>::type;
  template <typename T>
  using cold = typename std::conditional<cold_lds, T *, MM_GLOBAL_PTR(T)>::type;
  hot<float> mcd, mcd2;      // candidate (dist, dist2)
  hot<hidx_t> lin1, lin2;    // candidate pair (stale indices are part of the carried state)
  hot<unsigned char> flag;   // rebuilt in this merge
  warm<float> mv, mvcf;      // min_values, min_values_CF
  cold<cidx_t> ci;           // the live clusters in order (mirror of the threads' registers)
  cold<cidx_t> csz;          // cluster sizes (floats in the reference: exact integers)
  // the AGES build: the candidate's draw as a double and its age level, the cluster's own age level
  hot<double> d2d;
  hot<hidx_t> lv;
  cold<cidx_t> alv;
};
// Bytes of dynamic LDS per cluster as build_tree carves the fields up: the host asks for them (lds_state_bytes)
constexpr size_t MM_LDS_PER_CLUSTER_LDS = 8 + 3 * 4 + 6 * 2 + 1;  // 33: d2d; mv, mvcf, mcd; lin1, lin2, ci, csz, lv, alv; flag
constexpr size_t MM_LDS_PER_CLUSTER_HOT = 2 * 4 + 2 * 2 + 1;      // 13: mcd, mcd2; lin1, lin2; flag
constexpr size_t MM_LDS_PER_CLUSTER_WARM = 4 * 4 + 2 * 2 + 1;     // 21: L_HOT's and mv, mvcf

// Wave reductions on the DPP crossbar (quad swaps, half-row and row mirrors, the two row broadcasts: the total
// lands in lane 63 and is read back to all lanes) -- a __shfl_xor butterfly is six dependent LDS round trips per value,
// and a merge has a dozen reductions on its critical path.  Lanes a step does not write keep their own value.
template <int CTRL, int RM>
__device__ inline float dpp_keep_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, RM, 0xf, false));
}
template <int CTRL, int RM>
__device__ inline int dpp_keep_i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, RM, 0xf, false);
}
#define MM_DPP_STEPS(X) X(0xB1, 0xf) X(0x4E, 0xf) X(0x141, 0xf) X(0x140, 0xf) X(0x142, 0xa) X(0x143, 0xc)
__device__ inline float wave_min_f(float v) {
#define MM_STEP(C, R) v = fminf(v, dpp_keep_f<C, R>(v));
  MM_DPP_STEPS(MM_STEP)
#undef MM_STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ inline int wave_min_i(int v) {
#define MM_STEP(C, R) v = min(v, dpp_keep_i<C, R>(v));
  MM_DPP_STEPS(MM_STEP)
#undef MM_STEP
  return __builtin_amdgcn_readlane(v, 63);
}
// exclusive prefix of v over the threads in order; *total = sum
__device__ inline int block_scan(int v, int *total, int *buf) {
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if ((int)(threadIdx.x & 63) >= o) x += y;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 63) buf[threadIdx.x >> 6] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MM_WAVES; w++) {
    if (w < (int)(threadIdx.x >> 6)) base += buf[w];
    tot += buf[w];
  }
  *total = tot;
  return base + x - v;
}
// lexicographic minimum of (d1, d2, pos)
__device__ inline bool lex_less(float a1, float a2, int ap, float b1, float b2, int bp) {
  return a1 < b1 || (a1 == b1 && (a2 < b2 || (a2 == b2 && ap < bp)));
}
__device__ inline void wave_lex_min(float &d1, float &d2, int &pos) {
#define MM_STEP(C, R)                                                          \
  {                                                                            \
    const float o1 = dpp_keep_f<C, R>(d1), o2 = dpp_keep_f<C, R>(d2);          \
    const int op = dpp_keep_i<C, R>(pos);                                      \
    if (lex_less(o1, o2, op, d1, d2, pos)) {                                   \
      d1 = o1;                                                                 \
      d2 = o2;                                                                 \
      pos = op;                                                                \
    }                                                                          \
  }
  MM_DPP_STEPS(MM_STEP)
#undef MM_STEP
  d1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d1), 63));
  d2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d2), 63));
  pos = __builtin_amdgcn_readlane(pos, 63);
}
__device__ inline void block_lex_min(float &d1, float &d2, int &pos, float *b1, float *b2, int *bp) {
  wave_lex_min(d1, d2, pos);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    b1[threadIdx.x >> 6] = d1;
    b2[threadIdx.x >> 6] = d2;
    bp[threadIdx.x >> 6] = pos;
  }
  __syncthreads();
  d1 = b1[0];
  d2 = b2[0];
  pos = bp[0];
#pragma unroll
  for (int w = 1; w < MM_WAVES; w++)
    if (lex_less(b1[w], b2[w], bp[w], d1, d2, pos)) {
      d1 = b1[w];
      d2 = b2[w];
      pos = bp[w];
    }
}
// three independent minima with one exchange
__device__ inline void block_min3(float &f, int &a, int &b, float *bf, int *ba, int *bb) {
  f = wave_min_f(f);
  a = wave_min_i(a);
  b = wave_min_i(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    bf[threadIdx.x >> 6] = f;
    ba[threadIdx.x >> 6] = a;
    bb[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  f = bf[0];
  a = ba[0];
  b = bb[0];
#pragma unroll
  for (int w = 1; w < MM_WAVES; w++) {
    f = fminf(f, bf[w]);
    a = min(a, ba[w]);
    b = min(b, bb[w]);
  }
}

// ---- the AGES build (`--sample_ages`; tree_builder.cpp:3-22, :149-252, :601-965 and their twins with a prior)
// A candidate (dist, dist2, dist3, replace): dist3 -- the older of the pair's two sample ages -- is one of the distinct
// sample ages and is kept as its index in their sorted table (comparisons of ages = comparisons of indices);
// `replace` is not stored: after the refresh every merge begins with (:618) it equals "dist3 is beyond the clock" for
// every candidate there is, and that is how it is set when one is made (:216, :234).  lw = the largest index whose
// age the clock has reached.
constexpr int MM_AGE_EMPTY = 0x7fff;  // (more than any level: N <= 10240; fits the shorts of the state in LDS)
struct AgeCand {
  float d;
  double d2;
  int lv, l1, l2;
};
// operator> of tree_builder.cpp:7-22 (a = the holder): with a.replace and a.dist3 >= b.dist3 the first block returns
// for a.dist3 > b.dist3 and otherwise tests what the second block tests again
__device__ inline bool ages_gt(const AgeCand &a, float bd, double bd2, int blv, int lw) {
  const bool a_replace = a.lv != MM_AGE_EMPTY && a.lv > lw;
  return (a_replace && a.lv > blv) || a.d > bd || (a.d == bd && a.d2 > bd2);
}
// "may b take a's place": the test in front of every assignment to a candidate slot (:209-218) and to the running
// best (:230-237)
__device__ inline bool ages_takes(const AgeCand &a, float bd, double bd2, int blv, int lw) {
  return (a.d == INFINITY || blv <= lw) && ages_gt(a, bd, bd2, blv, lw);
}
// lexicographic minimum of (d1, d2, pos) over the wave, in every lane
__device__ inline void wave_lex_min_d(float &d1, double &d2, int &pos) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float o1 = __shfl_xor(d1, o, 64);
    const double o2 = __shfl_xor(d2, o, 64);
    const int op = __shfl_xor(pos, o, 64);
    if (o1 < d1 || (o1 == d1 && (o2 < d2 || (o2 == d2 && op < pos)))) {
      d1 = o1;
      d2 = o2;
      pos = op;
    }
  }
}
// one expected coalescence of k lineages (:1155, :1226): 2 / (k (k - 1)) * Ne, every operation rounded by itself
__device__ inline double ages_step(int k, int Ne) {
  return __dmul_rn(__ddiv_rn(2.0, __dmul_rn((double)k, (double)k - 1.0)), (double)Ne);
}

// (32-bit element offsets from a scalar base -- N <= 10240: one address register per load instead of two)
#define MM(a, b) p.M[mm_index((unsigned)(a), (unsigned)(b), (unsigned)N)]
#define MM2(a, b) (((MM_GLOBAL_PTR(const f32x2))(p.M + mm_index((unsigned)(a), (unsigned)(b), (unsigned)N)))[0])  // (d(a,b), d(b,a))
// (one half of a pair only: d(a,b) -- the first filter of a test runs on it, the few survivors fetch d(b,a))
#define MM1(a, b) (((MM_GLOBAL_PTR(const float))(p.M + mm_index((unsigned)(a), (unsigned)(b), (unsigned)N)))[0])
#define MMY(a, b) (((MM_GLOBAL_PTR(const float))(p.M + mm_index((unsigned)(a), (unsigned)(b), (unsigned)N)))[1])
#define SS(a, b) symm[(unsigned)(a) * (unsigned)N + (unsigned)(b)]

// One workgroup per tree: workgroup b builds the tree of params[b].
//
// A merge (i into j) on the workgroup, thread t holding the clusters at positions t, t + 512, ... of the live list IN
// ITS REGISTERS for the whole build (a_k; the positions behind a cluster that leaves move up by one lane):
//   A. every thread: the four entries (k,j), (k,i), (i,k), (j,k) of both matrices for its clusters k (all loads of a
//      pass issued at once, with the clusters' row minima, which stay in registers to the end of the merge), the
//      size-weighted updates written back; which clusters rebuild their
//      candidates (row minimum on a changed entry, or candidate touching i or j: appended to a list in LDS, their
//      candidates reset); partial minima of the merged cluster's row (both matrices) and the best candidate among
//      the clusters that keep theirs, (dist, dist2, position)-lexicographic -- one exchange for all of it;
//   B. the rows of the rebuilt clusters, ROWS at a time, d(k,l) per thread and position (one half of a pair: 4 of an
//      element's 16 bytes): first the row-minimum rescans (the reference's scan with early exit = "the old minimum if
//      it occurs before any smaller entry, else the row's minimum": three reductions, finished by one wave per row),
//      then, on the values still in registers, the row half of the candidate test of every pair the rebuilt cluster
//      is part of; the few survivors fetch the other half, d(l,k), themselves and append the feasible pairs, keyed by
//      (position of the later cluster, position of the earlier one), to a list in LDS;
//   C. the merged cluster's own pairs from its row as A left it (d(j,k) read back, in flight since the start of B; the
//      survivors fetch d(k,j)), keyed behind all others;
//   D. the pairs sorted by key (rank = number of smaller keys) -- the order in which the reference meets them --
//      and ONE lane draws the random numbers and updates the candidates in that order, then settles the running
//      best: per cluster the candidate it holds at its turn of the reference's loop, smallest (dist, dist2),
//      earliest position among exact ties;
//   E. the merged-away cluster leaves the list.
// Three dependent memory round trips and eight workgroup barriers per merge; everything else is LDS.
//
// AGES (`--sample_ages`): the same merge with the candidates' third key and the coalescence clock.  What is a
// reduction above -- the running best over the clusters in order -- is order-dependent there (a candidate beyond the
// clock takes an EMPTY place only, one within the clock displaces it whatever its distance), so wave 0 walks the
// live list once per merge, the pairs applied at their clusters' turns: exact, and slower (data sets with ancient
// samples are small).  Its per-cluster state lives in one place: LDS up to N = 4100 (L_LDS), global memory above.
template <int LAY, int MAXQ, bool AGES, int ROWS>
__device__ __forceinline__ void build_tree(const MMParamsDev &p, Shared &sh, unsigned char *dyn) {
  typedef typename State<LAY>::hidx_t hidx_t;
  typedef typename State<LAY>::cidx_t cidx_t;
  static_assert(ROWS <= MM_ROWS_MAX && ROWS <= MM_WAVES, "a wave finishes a row's rescan");
  static_assert((LAY != L_HOT && LAY != L_WARM) || !AGES, "the AGES build keeps all of its state in one place");
  const int N = p.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float INF = INFINITY;
  const float threshold = p.threshold, threshold_CF = p.threshold_CF;
  State<LAY> st;  // (what this carve-up takes per cluster is what the host asks for: MM_LDS_PER_CLUSTER_*)
  if constexpr (LAY == L_LDS && AGES) {  // 33 bytes per cluster (the float draw of the plain build has no place here)
    st.d2d = reinterpret_cast<double *>(dyn);
    float *f = reinterpret_cast<float *>(st.d2d + N);
    st.mv = f;
    st.mvcf = f + N;
    st.mcd = f + 2 * (size_t)N;
    st.mcd2 = nullptr;
    short *s = reinterpret_cast<short *>(f + 3 * (size_t)N);
    st.lin1 = s;
    st.lin2 = s + N;
    st.ci = s + 2 * (size_t)N;
    st.csz = s + 3 * (size_t)N;
    st.lv = s + 4 * (size_t)N;
    st.alv = s + 5 * (size_t)N;
    st.flag = reinterpret_cast<unsigned char *>(s + 6 * (size_t)N);
  } else if constexpr (LAY == L_LDS) {
    float *f = reinterpret_cast<float *>(dyn);
    st.mv = f;
    st.mvcf = f + N;
    st.mcd = f + 2 * (size_t)N;
    st.mcd2 = f + 3 * (size_t)N;
    short *s = reinterpret_cast<short *>(f + 4 * (size_t)N);
    st.lin1 = s;
    st.lin2 = s + N;
    st.ci = s + 2 * (size_t)N;
    st.csz = s + 3 * (size_t)N;
    st.flag = reinterpret_cast<unsigned char *>(s + 4 * (size_t)N);
  } else if constexpr (LAY == L_HOT || LAY == L_WARM) {  // 13 / 21 bytes per cluster in LDS
    float *f = reinterpret_cast<float *>(dyn);
    st.mcd = f;
    st.mcd2 = f + N;
    if constexpr (LAY == L_WARM) {
      st.mv = f + 2 * (size_t)N;
      st.mvcf = f + 3 * (size_t)N;
      f += 2 * (size_t)N;
    } else {
      st.mv = p.min_values;
      st.mvcf = p.min_values_CF;
    }
    short *s = reinterpret_cast<short *>(f + 2 * (size_t)N);
    st.lin1 = s;
    st.lin2 = s + N;
    st.flag = reinterpret_cast<unsigned char *>(s + 2 * (size_t)N);
    st.ci = p.cluster_index;
    st.csz = p.cluster_size;
  } else {
    st.d2d = p.mc_dist2d;
    st.lv = p.mc_lvl;
    st.alv = p.age_lvl;
    st.mv = p.min_values;
    st.mvcf = p.min_values_CF;
    st.mcd = p.mc_dist;
    st.mcd2 = p.mc_dist2;
    st.lin1 = p.mc_lin1;
    st.lin2 = p.mc_lin2;
    st.ci = p.cluster_index;
    st.csz = p.cluster_size;
    st.flag = p.kflag;
  }
  // (timing: thread 0 only, accumulators in LDS -- twelve 64-bit counters per thread would cost the kernel its registers)
  if (tid == 0) {
    for (int x = 0; x < 16; x++) sh.tacc[x] = 0;
    sh.cnt_rescan_only = 0;
    sh.tmark = wall_clock64();
  }
  const long long tstart = wall_clock64(), cstart = clock64();
#define LAP(x)                           \
  if (p.timers && tid == 0) {            \
    const long long tn = wall_clock64(); \
    sh.tacc[x] += tn - sh.tmark;         \
    sh.tmark = tn;                       \
  }                                      \
  if (p.trace && tid == 0) {             \
    p.trace[0] = (unsigned)sh.n;         \
    p.trace[1] = (unsigned)(x);          \
  }

  // The tree leaves the workgroup -- built (0) or handed to the host (1: no room for the symmetric matrix, 2: more
  // tied candidates than the lists hold): thread 0, at a point all threads have reached.  The symmetric matrix goes
  // back to the pool; status, the tree and the carried state reach memory BEFORE the host hears of them in pinned
  // memory -- the builder's host thread takes its tree while the other workgroups still build theirs, no
  // end-of-kernel write-back in between.
  auto leave = [&](int code) {
    if (tid == 0) {
      *p.status = code;
      __threadfence_system();
      if (sh.sym_slot >= 0) __hip_atomic_store(&p.sym_locks[sh.sym_slot], 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      *p.host_done = code;
      __threadfence_system();
    }
  };
  MM_GLOBAL_PTR(float) symm = nullptr;  // the symmetric matrix of the fallback, once one is taken from the pool
  if (tid == 0) sh.sym_slot = -1;

  // ---- QuickBuild set-up (:1061-1100)
  // (L_HOT: the list's mirror in memory is written when the symmetric fallback first needs it)
  constexpr bool CI_ALWAYS = LAY != L_HOT && LAY != L_WARM;
  for (int c = tid; c < N; c += MM_BLOCK) {
    if constexpr (CI_ALWAYS) st.ci[c] = (cidx_t)c;
    st.csz[c] = (cidx_t)1;
    st.mcd[c] = INF;
    st.flag[c] = 0;
    if constexpr (AGES) {
      st.d2d[c] = (double)INF;
      st.lv[c] = (hidx_t)MM_AGE_EMPTY;
      st.alv[c] = (cidx_t)p.age_lvl0[c];
    } else {
      st.mcd2[c] = INF;
    }
    if constexpr (LAY != L_GLOBAL) {  // the state carried from tree to tree comes in (pinned host memory)
      st.lin1[c] = (hidx_t)p.io_lin[c];
      st.lin2[c] = (hidx_t)p.io_lin[(size_t)N + c];
      // (L_HOT: min_values_CF as carried over is in the device array already -- the weave reads it there)
      if constexpr (LAY != L_HOT) st.mvcf[c] = p.io_mvcf[c];
    }
  }
  // the live list: position t + MM_BLOCK q in slot q of thread t, for the whole build
  int a_k[MAXQ];
#pragma unroll
  for (int q = 0; q < MAXQ; q++) a_k[q] = q * MM_BLOCK + tid < N ? q * MM_BLOCK + tid : -1;
  if (tid == 0) {
    rng_seed(sh.rng, 1u);
    sh.best.dist = INF;
    sh.best.dist2 = INF;
    sh.best.lin1 = -1;
    sh.best.lin2 = -1;
    sh.best_sym = sh.best;
    sh.use_sym = 0;
    sh.n = N;
    sh.nupd = 0;
    sh.npairs = 0;
  }
  __syncthreads();

  // ---- Initialize (:59-146 / :1647-1735): row minima (+ threshold); the minima themselves come from the penalty / prior passes
  for (int a = tid; a < N; a += MM_BLOCK) {
    st.mv[a] = p.rowmin_D[a] + threshold;
    if (p.has_prior) {
      const float old = st.mvcf[a], mc_ = p.rowmin_CF[a];  // old: carried over from the previous build (:2399-2400)
      st.mvcf[a] = (old > mc_ ? mc_ : old) + threshold_CF;
    }
  }
  __syncthreads();
  LAP(0);
  // One wave runs every ordered part in step -- the values are the same in all 64 lanes (LDS reads of one address),
  // lane 0 does the writes; the lanes matter when the generator's state is renewed (624 words, 64 at a time).
  // Per pair the LDS reads -- two words of the generator, both clusters' candidates, the next pair's record -- are
  // independent and go out together: one LDS latency per pair.
  // The draws come 64 at a time: lane l tempers words ridx + 2l, ridx + 2l + 1 of the state and forms the
  // (l + 1)-th uniform float from now -- std::uniform_real_distribution<double>(0,1) of libstdc++ (rng_unif),
  // narrowed to float (tree_builder.hpp:60) --; a pair then takes its number with one readlane instead of two LDS
  // reads and thirty dependent instructions on the ordered path.  (624 is even: a draw never straddles a renewal.)
  // (the AGES build keeps the draw as the double it is: Candidate::dist2, tree_builder.hpp:26, assigned from the
  //  distribution directly, :205)
  typedef typename std::conditional<AGES, double, float>::type rnd_t;
  int ridx = 624;       // (wave 0: position in the generator's state)
  rnd_t rnd_lane = 0;   // lane l: draw number l of the batch
  int rnd_have = 0, rnd_at = 0;
  auto next_rnd = [&]() -> rnd_t {
    if (rnd_at >= rnd_have) {
      if (ridx >= 624) {
        rng_renew_wave(sh.rng, lane);
        ridx = 0;
      }
      rnd_have = min(64, (624 - ridx) / 2);
      const int i0 = lane < rnd_have ? ridx + 2 * lane : 0;
      uint32_t y1 = sh.rng.mt[i0], y2 = sh.rng.mt[i0 + 1];
      y1 ^= y1 >> 11;
      y2 ^= y2 >> 11;
      y1 ^= (y1 << 7) & 0x9d2c5680u;
      y2 ^= (y2 << 7) & 0x9d2c5680u;
      y1 ^= (y1 << 15) & 0xefc60000u;
      y2 ^= (y2 << 15) & 0xefc60000u;
      y1 ^= y1 >> 18;
      y2 ^= y2 >> 18;
      const double sum = (double)y1 + (double)y2 * 4294967296.0;
      double ret = sum / 18446744073709551616.0;
      if (ret >= 1.0) ret = 0.99999999999999988897769753748434595763683319091796875;
      rnd_lane = (rnd_t)ret;
      ridx += 2 * rnd_have;
      rnd_at = 0;
    }
    const int at = __builtin_amdgcn_readfirstlane(rnd_at);
    rnd_at++;
    if constexpr (AGES) {
      const long long bits = __double_as_longlong(rnd_lane);
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(bits & 0xffffffffll), at);
      const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), at);
      return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    } else {
      return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rnd_lane), at));
    }
  };
  // ---- AGES: the clock (wave 0 keeps it; tree_builder.cpp:1123-1155 / :2407-2440) and the candidate slots
  int a_level = 0, a_lins = 0, a_lw = -1;  // sampling level reached, lineages alive there, last level within the clock
  double a_age = 0.0;
  auto clock_reaches = [&]() {  // a_lw follows a_age
    while (a_lw + 1 < p.n_levels && p.unique_ages[a_lw + 1] <= a_age) a_lw++;
  };
  if constexpr (AGES) {
    a_lins = p.ages_count[0];
    // the clock starts one expected coalescence in without a prior (:1155), at the youngest samples with one (:2440)
    a_age = p.has_prior ? p.unique_ages[0] : __dadd_rn(p.unique_ages[0], ages_step(a_lins, p.Ne));
    clock_reaches();
    if (tid == 0) sh.a_lw = a_lw;
  }
  auto slot_of = [&](int c) -> AgeCand {
    return AgeCand{st.mcd[c], st.d2d[c], (int)st.lv[c], (int)st.lin1[c], (int)st.lin2[c]};
  };
  // MinMatch's `cand` offered to both of its clusters (:205-218 and every block like it); xs / ys: what x and y hold
  // afterwards
  auto apply_ages = [&](int x, int y, float sym, AgeCand &xs, AgeCand &ys) {
    const double rnd = (double)next_rnd();
    xs = slot_of(x);
    ys = slot_of(y);
    const int clv = max((int)st.alv[x], (int)st.alv[y]);
    const AgeCand c{sym, rnd, clv, x, y};
    const bool tx = ages_takes(xs, sym, rnd, clv, a_lw), ty = ages_takes(ys, sym, rnd, clv, a_lw);
    if (tx) xs = c;
    if (ty) ys = c;
    if (lane == 0) {
      if (tx) {
        st.lin1[x] = (hidx_t)x;
        st.lin2[x] = (hidx_t)y;
        st.mcd[x] = sym;
        st.d2d[x] = rnd;
        st.lv[x] = (hidx_t)clv;
      }
      if (ty) {
        st.lin1[y] = (hidx_t)x;
        st.lin2[y] = (hidx_t)y;
        st.mcd[y] = sym;
        st.d2d[y] = rnd;
        st.lv[y] = (hidx_t)clv;
      }
    }
  };
  // the running best of Initialize / Coalesce (:230-237): wave 0's registers
  AgeCand abest{INF, (double)INF, MM_AGE_EMPTY, -1, -1};
  auto best_takes = [&](const AgeCand &mcand) {
    if (ages_takes(abest, mcand.d, mcand.d2, mcand.lv, a_lw)) abest = mcand;
  };
  // one feasible pair in the reference's order: one draw, both clusters' best candidate (:1704-1716); -> the draw
  auto apply = [&](int x, int y, float sym) -> float {
    const float rnd = next_rnd();
    const float ad = st.mcd[x], ad2 = st.mcd2[x], bdd = st.mcd[y], bdd2 = st.mcd2[y];
    if (lane == 0) {
      if (ad > sym || (ad == sym && ad2 > rnd)) {
        st.lin1[x] = (hidx_t)x;
        st.lin2[x] = (hidx_t)y;
        st.mcd[x] = sym;
        st.mcd2[x] = rnd;
      }
      if (bdd > sym || (bdd == sym && bdd2 > rnd)) {
        st.lin1[y] = (hidx_t)x;
        st.lin2[y] = (hidx_t)y;
        st.mcd[y] = sym;
        st.mcd2[y] = rnd;
      }
    }
    return rnd;
  };
  // mutually close pairs in (a, b) order (:1690-1722): weave_kernel has found them; MM_BLOCK rows at a time they
  // are staged in LDS in order and wave 0 draws
  auto draw_staged = [&](int count) {  // wave 0: the staged pairs sh.pxy[0] / sh.psym[0] in order (:1704-1722)
    if constexpr (AGES) {  // (:205-237)
      for (int e = 0; e < count; e++) {
        const unsigned xy = sh.pxy[0][e];
        AgeCand xs, ys;
        apply_ages((int)(xy >> 16), (int)(xy & 0xffffu), sh.psym[0][e], xs, ys);
        best_takes(ys);
      }
      if (lane == 0) {
        sh.best.dist = abest.d;
        sh.best.lin1 = abest.l1;
        sh.best.lin2 = abest.l2;
      }
      return;
    }
    Best bb = sh.best;
    for (int e = 0; e < count; e++) {
      const unsigned xy = sh.pxy[0][e];
      const float sym = sh.psym[0][e];
      const int aa = (int)(xy >> 16), b = (int)(xy & 0xffffu);
      // (b's candidate after this pair: what apply() is about to leave there)
      const float od = st.mcd[b], od2 = st.mcd2[b];
      const float rnd = apply(aa, b, sym);
      const bool took = od > sym || (od == sym && od2 > rnd);
      const float md = took ? sym : od, md2 = took ? rnd : od2;
      if (bb.dist > md || (bb.dist == md && bb.dist2 > md2)) {
        bb.lin1 = aa;
        bb.lin2 = b;
        bb.dist = sym;
        bb.dist2 = md2;
      }
    }
    if (lane == 0) sh.best = bb;
  };
  for (int a0 = 0; a0 < N; a0 += MM_BLOCK) {
    const int a = a0 + tid;
    const int c = a < N ? p.hit_cnt[a] : 0;
    int total;
    const int off = block_scan(c, &total, sh.wave_i);
    if (__syncthreads_or(c > MM_HITS)) {
      // a row of this stretch has more partners than the pair scan keeps (flat matrices): its rows are scanned here,
      // one by one, MM_BLOCK columns at a time
      for (int ar = a0; ar < min(N, a0 + MM_BLOCK); ar++) {
        const float mva = st.mv[ar];
        for (int b0 = ar + 1; b0 < N; b0 += MM_BLOCK) {
          const int b = b0 + tid;
          f32x4 e = {0.f, 0.f, 0.f, 0.f};
          bool hit = false;
          if (b < N) {
            e = MM(ar, b);
            hit = mva >= e.x && st.mv[b] >= e.y;
          }
          int cnt;
          const int at = block_scan(hit ? 1 : 0, &cnt, sh.wave_i);
          if (hit) {
            float sym = e.y + e.x;
            if constexpr (AGES) {  // (:1792-1797: the pairs the prior agrees with are kept, the others voided)
              if (p.has_prior && !(e.z <= st.mvcf[ar] && e.w <= st.mvcf[b])) sym = INF;
            } else {
              if (p.has_prior && e.z <= st.mvcf[ar] && e.w <= st.mvcf[b]) sym = 0.0f;
            }
            sh.pxy[0][at] = ((unsigned)ar << 16) | (unsigned)b;
            sh.psym[0][at] = sym;
          }
          __syncthreads();
          if (wave == 0) draw_staged(cnt);
          __syncthreads();
        }
      }
      continue;
    }
    // whole rows, as many as the staging area holds (all of them, usually), pass by pass
    for (int base = 0; base < total;) {
      if (tid == 0) sh.count = total;
      __syncthreads();
      const bool mine = c > 0 && off >= base && off + c <= base + MM_PAIRS_LDS;
      if (mine) {
        for (int e = 0; e < c; e++) {
          sh.pxy[0][off - base + e] = ((unsigned)a << 16) | p.hit_b[(size_t)a * MM_HITS + e];
          sh.psym[0][off - base + e] = p.hit_sym[(size_t)a * MM_HITS + e];
        }
      } else if (c > 0 && off >= base) {
        atomicMin(&sh.count, off);  // the first row that has to wait
      }
      __syncthreads();
      const int next = sh.count;
      if (wave == 0) draw_staged(next - base);
      __syncthreads();
      base = next;
    }
  }
  LAP(1);

  // ---- the merges
  // A tree the lists cannot hold is handed to the host (bail >= 0: the code).  ONE way out of the function, through
  // wave-uniform branches the compiler can see are uniform (readfirstlane): the workgroup goes on to its next tree
  // behind this call, and an exit the compiler takes for divergent -- it hangs on values read from LDS -- is laid
  // out as a loop in which a wave passes the caller's barriers once per group of lanes.
  int bail = -1;
  for (int num_nodes = N; num_nodes < 2 * N - 1; num_nodes++) {
    const int n = sh.n;
    if (sh.best.dist == INF && !sh.use_sym) {
      // no mutually closest pair: from here on the symmetric matrix picks the pair when there is none
      // (initialize_sym, tree_builder.cpp:255-293): s(a,l) = d(a,l) + d(l,a) over the live clusters, row minima
      // with the first cluster that reaches them, the smallest of those (first row, first cluster)
      if (tid == 0) {  // a matrix of the device's pool
        int got = -1;
        for (int sl = 0; sl < p.sym_slots && got < 0; sl++) {
          int expected = 0;
          if (__hip_atomic_compare_exchange_strong(&p.sym_locks[sl], &expected, 1, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT))
            got = sl;
        }
        sh.sym_slot = got;
      }
      __syncthreads();
      const int slot = __builtin_amdgcn_readfirstlane(sh.sym_slot);
      if (slot < 0) {  // (none free, or no pool)
        bail = 1;
        break;
      }
      symm = p.SYM + (size_t)slot * N * N;
      if constexpr (!CI_ALWAYS) {  // the live list as it stands in the registers: from here on it is kept in memory too
#pragma unroll
        for (int q = 0; q < MAXQ; q++)
          if (a_k[q] >= 0) st.ci[q * MM_BLOCK + tid] = (cidx_t)a_k[q];
        __syncthreads();
      }
      float bs = INF;
      int bs_pos = n;
      for (int ia = wave; ia < n; ia += MM_WAVES) {
        const int a = st.ci[ia];
        float mv = INF;
        int mp = n;
        for (int il = lane; il < n; il += 64) {
          const int l = st.ci[il];
          if (l == a) continue;
          const f32x2 e = MM2(a, l);
          const float v = e.x + e.y;
          SS(a, l) = v;
          if (v < mv) {  // (ascending per lane: the first one stays)
            mv = v;
            mp = il;
          }
        }
        {
          float zero = 0.0f;
          wave_lex_min(mv, zero, mp);  // (value, position)
        }
        if (lane == 0) {
          p.min_values_sym[a] = mv;
          p.mcs_dist[a] = mv;
          if (mv < INF) {
            p.mcs_lin1[a] = a;
            p.mcs_lin2[a] = st.ci[mp];
          }
          if (mv < bs) {  // (rows ascending per wave)
            bs = mv;
            bs_pos = ia;
          }
        }
      }
      float bs2 = 0.0f;
      block_lex_min(bs, bs2, bs_pos, sh.wave_f, sh.wave_f2, sh.wave_i);
      if (tid == 0) {
        sh.use_sym = 1;
        sh.best_sym.dist = bs;
        if (bs_pos < n && bs < INF) {
          sh.best_sym.lin1 = p.mcs_lin1[st.ci[bs_pos]];
          sh.best_sym.lin2 = p.mcs_lin2[st.ci[bs_pos]];
        }
      }
      __syncthreads();
    }
    const bool by_sym = sh.best.dist == INF;
    const int i = by_sym ? sh.best_sym.lin1 : sh.best.lin1, j = by_sym ? sh.best_sym.lin2 : sh.best.lin2;
    const float csi = (float)st.csz[i], csj = (float)st.csz[j];
    const float added = csi + csj;
    if (tid == 0) {  // (:2437-2460 happens on the host, from this log: no loads on the merge's path)
      p.merge_i[num_nodes - N] = i;
      p.merge_j[num_nodes - N] = j;
    }

    // -- A: this thread's clusters
    // (a / added for the size-weighted means: `added` is one integer <= 10240 for the whole merge, so the quotient
    //  comes from a double product with its reciprocal -- the exact quotient of a 24-bit by a 14-bit number is at
    //  least 2^-39 (relative) off every rounding boundary of float unless it is a float itself, the product is
    //  within 2^-51: the same float as the division's.  Quotients in the subnormal range take the division.)
    const double rc_added = 1.0 / (double)added;
    auto over_added = [&](float a) -> float {
      const float q = (float)((double)a * rc_added);
      return fabsf(q) >= 1e-30f || a == 0.0f ? q : a / added;
    };
    // (the live list shrinks from N to 2: the register slots past it are skipped by wave-uniform branches, not by
    //  predication -- half of all slots over a build)
    const int nq = (n + MM_BLOCK - 1) / MM_BLOCK;
    float mvreg[MAXQ];  // the row minima (+ threshold) of this thread's clusters as the merge finds them
    float mv_cf = INF, mvj = INF, bd = INF, bd2 = INF;
    double bd2d = (double)INF;  // (AGES)
    const int lw_all = AGES ? sh.a_lw : 0;
    int bpos = n, bk = -1;
#ifndef MM_QC20
#define MM_QC20 4
#endif
    // clusters per pass (ten at once cost more in spilled registers than the second round trip)
#ifndef MM_QC10
#define MM_QC10 5
#endif
    constexpr int QC = MAXQ == MM_Q_GLOB ? MM_QC20 : MAXQ % 5 == 0 ? (ROWS == 1 ? 5 : MM_QC10) : 4;
#pragma unroll
    for (int q0 = 0; q0 < MAXQ; q0 += QC) {
      if (q0 * MM_BLOCK >= n) break;
      // every load of the pass from memory first: the two rows and the clusters' row minima; what lives in LDS is read
      // cluster by cluster under their latency (state in global memory: asked for with the rows)
      f32x4 ei[QC], ej[QC];
#pragma unroll
      for (int qq = 0; qq < QC; qq++) {
        const int k = a_k[q0 + qq];
        if (k < 0 || k == j || k == i) continue;
        ei[qq] = MM(i, k);
        ej[qq] = MM(j, k);
      }
      // the candidate's fields from LDS: all of the pass at once while the registers allow (256 per lane: 2 ms of a
      // tree under load), at the cluster's turn in the 128-register kernels
      constexpr bool JIT = State<LAY>::hot_lds && (ROWS == 1 || QC > 5);
      float s_d1[JIT ? 1 : QC], s_d2[JIT ? 1 : QC];
      int s_l1[JIT ? 1 : QC], s_l2[JIT ? 1 : QC];
      double s_d2d[AGES && !JIT ? QC : 1];
      int s_lv[AGES && !JIT ? QC : 1];
#pragma unroll
      for (int qq = 0; qq < QC; qq++) {
        const unsigned k = a_k[q0 + qq] >= 0 ? (unsigned)a_k[q0 + qq] : 0u;
        mvreg[q0 + qq] = st.mv[k];
        if constexpr (!JIT) {
          s_l1[qq] = st.lin1[k];
          s_l2[qq] = st.lin2[k];
          s_d1[qq] = st.mcd[k];
          if constexpr (!AGES) s_d2[qq] = st.mcd2[k];
          if constexpr (AGES) {
            s_d2d[qq] = st.d2d[k];
            s_lv[qq] = st.lv[k];
          }
        }
      }
#pragma unroll
      for (int qq = 0; qq < QC; qq++) {
        const int q = q0 + qq;
        const int ik = q * MM_BLOCK + tid;
        const int k = a_k[q];
        if (k < 0) continue;
        if (k == j || k == i) {
          if (k == i) sh.ipos = ik;
          continue;
        }
        float ncjk = 0.0f, nckj = 0.0f;
        if (p.has_prior) {
          const float ckj = ej[qq].w, cki = ei[qq].w, cik = ei[qq].z, cjk = ej[qq].z;
          ncjk = cjk;
          nckj = ckj;
          if (cik != cjk) ncjk = over_added(csi * cik + csj * cjk);
          if (cki != ckj) nckj = over_added(csi * cki + csj * ckj);
          if (mv_cf > ncjk) mv_cf = ncjk;
        }
        const float dkj = ej[qq].y, dki = ei[qq].y, dik = ei[qq].x, djk = ej[qq].x;
        float njk = djk, nkj = dkj;
        if (dik != djk) njk = over_added(csi * dik + csj * djk);
        if (dki != dkj) nkj = over_added(csi * dki + csj * dkj);
        // (written whether changed or not: the same bits where the reference leaves the entry alone)
        MM(j, k) = f32x4{njk, nkj, ncjk, nckj};
        MM(k, j) = f32x4{nkj, njk, nckj, ncjk};
        if (njk < mvj) mvj = njk;
        bool rescan = false;
        const float mvk = mvreg[q];
        if (dkj != dki) {
          rescan = (double)fabsf(mvk - threshold - dkj) < 1e-4 || (double)fabsf(mvk - threshold - dki) < 1e-4;
        }
        const int sq = JIT ? 0 : qq;
        if constexpr (JIT) {
          s_l1[0] = st.lin1[k];
          s_l2[0] = st.lin2[k];
          s_d1[0] = st.mcd[k];
          if constexpr (!AGES) s_d2[0] = st.mcd2[k];
          if constexpr (AGES) {
            s_d2d[0] = st.d2d[k];
            s_lv[0] = st.lv[k];
          }
        }
        const int l1 = s_l1[sq], l2 = s_l2[sq];
        const bool touches = l1 == j || l2 == j || l1 == i || l2 == i;
        if (p.timers && rescan && !touches) atomicAdd(&sh.cnt_rescan_only, 1);
        // (AGES with a prior: a candidate that touches i or j alone does not send k through the rebuilding branch
        //  when none of its four distances moved -- :2131 against :653 --, the candidate is renamed instead, :2342)
        bool rebuilds = rescan || touches;
        if constexpr (AGES) rebuilds = rescan || (touches && (!p.has_prior || dkj != dki || djk != dik));
        if (rebuilds) {  // k rebuilds its candidates (:1893-1911)
          st.flag[k] = 1;
          st.mcd[k] = INF;
          if constexpr (AGES) {
            st.d2d[k] = (double)INF;
            st.lv[k] = (hidx_t)MM_AGE_EMPTY;
          } else {
            st.mcd2[k] = INF;
          }
          const int slot = atomicAdd(&sh.nupd, 1);
          const unsigned rec = (unsigned)ik | ((unsigned)k << 14) | (rescan ? 1u << 28 : 0u);
          if (slot < MM_UPD_LDS) {
            sh.upd[slot] = rec;
            sh.updv[slot] = nkj;
            sh.updmv[slot] = mvk;
          } else if (AGES || slot < MM_UPD_MAX) {  // (the tail of a long list: the row minimum stays in memory)
            p.upd_g[slot - MM_UPD_LDS] = rec;
            p.updv_g[slot - MM_UPD_LDS] = nkj;
          }
        } else if constexpr (AGES) {
          if (l1 == i) st.lin1[k] = (hidx_t)j;
          if (l2 == i) st.lin2[k] = (hidx_t)j;
          // k keeps its candidate.  The running best (:230-237) takes the first candidate WITHIN the clock with a
          // finite distance from whatever it holds, from then on nothing but a smaller one of that kind, and a slot
          // leaves that kind only for a smaller one of it: if one of the clusters that keep theirs holds such a
          // candidate, the best of the merge is the smallest (dist, dist2) among them all -- a reduction.  If none
          // does, wave 0 walks the list (below).
          const float d1 = s_d1[sq];
          const double d2 = s_d2d[sq];
          if (s_lv[sq] <= lw_all && d1 < INF && (bd > d1 || (bd == d1 && bd2d > d2))) {
            bd = d1;
            bd2d = d2;
            bpos = ik;
            bk = k;
          }
        } else {  // k keeps its candidate: what the reference's running best sees at k's turn
          const float d1 = s_d1[sq], d2 = s_d2[sq];
          if (bd > d1 || (bd == d1 && bd2 > d2)) {  // (ascending positions per thread: the first one wins)
            bd = d1;
            bd2 = d2;
            bpos = ik;
            bk = k;
          }
        }
      }
    }
    mvj = wave_min_f(mvj);
    mv_cf = wave_min_f(mv_cf);
    const int bpos_mine = bpos;
    if constexpr (AGES) wave_lex_min_d(bd, bd2d, bpos);
    else wave_lex_min(bd, bd2, bpos);
    if (bpos < n && bpos_mine == bpos) sh.lex_k[wave] = bk;  // (one lane: positions are unique)
    if (lane == 0) {
      sh.wave_f[wave] = mvj;
      sh.wave_f2[wave] = mv_cf;
      sh.lex_d[wave] = bd;
      sh.lex_d2[wave] = bd2;
      if constexpr (AGES) sh.lex_d2d[wave] = bd2d;
      sh.lex_p[wave] = bpos;
    }
    __syncthreads();
    LAP(2);
    float min_value_j = sh.wave_f[0], mvcf_j = sh.wave_f2[0];
#pragma unroll
    for (int w = 1; w < MM_WAVES; w++) {
      min_value_j = fminf(min_value_j, sh.wave_f[w]);
      mvcf_j = fminf(mvcf_j, sh.wave_f2[w]);
    }
    min_value_j += threshold;
    mvcf_j += threshold_CF;
    const int nupd = __builtin_amdgcn_readfirstlane(sh.nupd);
    if (!AGES && nupd > MM_UPD_MAX) {  // (degenerate matrices: this tree is the host's)
      bail = 2;
      break;
    }
    // (a list longer than MM_UPD_LDS has its tail in global memory; there the row minimum is read where it lives)
    auto upd_at = [&](int u) -> unsigned { return u < MM_UPD_LDS ? sh.upd[u] : p.upd_g[u - MM_UPD_LDS]; };
    auto updv_at = [&](int u) -> float { return u < MM_UPD_LDS ? sh.updv[u] : p.updv_g[u - MM_UPD_LDS]; };
    auto updmv_at = [&](int u, int k) -> float { return u < MM_UPD_LDS ? sh.updmv[u] : st.mv[k]; };
    auto rec_pos = [](unsigned e) -> int { return (int)(e & 0x3fffu); };
    auto rec_k = [](unsigned e) -> int { return (int)((e >> 14) & 0x3fffu); };
    auto rec_rescan = [](unsigned e) -> bool { return (e >> 28) != 0; };
    if (p.timers && tid == 0) {
      sh.tacc[12] += nupd * 100;
      sh.tacc[13] += sh.cnt_rescan_only * 100;
      sh.tacc[14] += nupd == 0 ? 100 : 0;
      sh.tacc[15] += sh.cnt_rescan_only > 0 ? 100 : 0;
      sh.cnt_rescan_only = 0;
    }

    // -- B: rows of the rebuilt clusters: (d(k,l), d(l,k)) along row k of M, ROWS rows per pass.  The row-minimum
    // rescans (:1875-1890) come first -- the reference's scan with early exit = "the old minimum if it occurs before
    // any smaller entry, else the row's minimum", three reductions finished by one wave per row --, then the
    // candidate tests of every pair a rebuilt cluster is part of (:1893-1911 for the clusters before it, :1913-2018
    // for the ones behind it), on the same registers when the merge has no more than ROWS rebuilt clusters.
    float cj[MAXQ];  // row j of M as this thread wrote it in A, d(j,k): asked for now, used in C
#pragma unroll
    for (int q = 0; q < MAXQ; q++) {
      if (q >= nq) break;
      const int k = a_k[q];
      cj[q] = (k >= 0 && k != i && k != j) ? MM1(j, k) : INF;
    }
    float v[ROWS][MAXQ];  // d(k, l) along the rows of the rebuilt clusters k
    auto load_rows = [&](const int (&ks)[ROWS]) {
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (ks[r] < 0) continue;
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
          if (q >= nq) break;
          v[r][q] = a_k[q] >= 0 ? MM1(ks[r], a_k[q]) : INF;
        }
      }
    };
    // rescans of the rows ks[r] >= 0 (entries us[r] of the list) held in v; patch[r]: the row's new entry at column j
    // (not in memory yet).  The new minimum goes to memory and, for the tests, to the list.
    auto rescan_rows = [&](const int (&ks)[ROWS], const int (&us)[ROWS], const float (&patch)[ROWS]) {
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const int k = ks[r];
        if (k < 0) continue;
        const float old = updmv_at(us[r], k) - threshold;
        float fm = INF;
        int pos_old = n, pos_less = n;
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
          if (q >= nq) break;
          const int l = a_k[q];
          if (l < 0 || l == i || l == k) continue;
          const float x = l == j ? patch[r] : v[r][q];
          fm = fminf(fm, x);
          if (x == old) pos_old = min(pos_old, q * MM_BLOCK + tid);
          if (x < old) pos_less = min(pos_less, q * MM_BLOCK + tid);
        }
        fm = wave_min_f(fm);
        pos_old = wave_min_i(pos_old);
        pos_less = wave_min_i(pos_less);
        if (lane == 0) {
          sh.red_f[r][wave] = fm;
          sh.red_a[r][wave] = pos_old;
          sh.red_b[r][wave] = pos_less;
        }
      }
      __syncthreads();
      int myk = -1, myu = 0;  // one wave finishes one row
#pragma unroll
      for (int r = 0; r < ROWS; r++)
        if (wave == r) {
          myk = ks[r];
          myu = us[r];
        }
      if (myk >= 0) {
        float fm = lane < MM_WAVES ? sh.red_f[wave][lane] : INF;
        int pos_old = lane < MM_WAVES ? sh.red_a[wave][lane] : n;
        int pos_less = lane < MM_WAVES ? sh.red_b[wave][lane] : n;
        fm = wave_min_f(fm);
        pos_old = wave_min_i(pos_old);
        pos_less = wave_min_i(pos_less);
        const float old = updmv_at(myu, myk) - threshold;
        if (lane == 0) {
          const float nv = ((pos_old < n && pos_old < pos_less) ? old : fm) + threshold;
          st.mv[myk] = nv;
          if (myu < MM_UPD_LDS) sh.updmv[myu] = nv;
        }
      }
      __syncthreads();
    };
    // (a feasible pair: its symmetric distance is worked out when the pairs are put in order -- one more element of
    //  M per pair, fetched for all pairs at once)
    auto append_pair = [&](unsigned key, int x, int y) {
      const int slot = atomicAdd(&sh.npairs, 1);
      if (slot < MM_PAIRS_LDS) {
        sh.pk[0][slot] = key;
        sh.pxy[0][slot] = ((unsigned)x << 16) | (unsigned)y;
      } else if (slot - MM_PAIRS_LDS < p.pair_cap) {
        auto g = p.pair_g + (size_t)(slot - MM_PAIRS_LDS) * 3;
        g[0] = key;
        g[1] = ((unsigned)x << 16) | (unsigned)y;
      }
    };
    // (slot q of this thread's registers for a q known at run time only -- the few survivors of a test: a chain of
    //  selects, not an indexed array, which would live in scratch memory)
    auto slot_k = [&](int q) -> int {
      int k = -1;
#pragma unroll
      for (int x = 0; x < MAXQ; x++) k = x == q ? a_k[x] : k;
      return k;
    };
    // this thread's cluster k in slot q: its row minimum as A found it, or -- rebuilt in this merge -- as the rescans left it
    auto mv_now = [&](int q, int k) -> float {
      if (st.flag[k]) return st.mv[k];
      float x = INF;
#pragma unroll
      for (int y = 0; y < MAXQ; y++) x = y == q ? mvreg[y] : x;
      return x;
    };
    // candidate tests of the rows u0 .. u0+ROWS-1 of the list, held in v / w
    auto test_rows = [&](int u0) {
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (u0 + r >= nupd) continue;
        const unsigned rec = upd_at(u0 + r);
        const int up = rec_pos(rec), ku = rec_k(rec);
        const float mvk = updmv_at(u0 + r, ku);
        unsigned surv = 0;  // bit q: (row r, this thread's cluster q) passes the row's half of the test
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
          if (q >= nq) break;
          const int l = a_k[q];
          const bool ok = l >= 0 && l != i && l != j && l != ku && v[r][q] <= mvk;
          surv |= ok ? 1u << q : 0u;
        }
        while (surv) {  // (few)
          const int q = __ffs((int)surv) - 1;
          surv &= surv - 1;
          const int il = q * MM_BLOCK + tid, l = slot_k(q);
          // a later cluster meets the rebuilt ones before it; a rebuilt one meets them from its own row
          if (il > up && st.flag[l]) continue;
          if (!(MMY(ku, l) <= mv_now(q, l))) continue;  // d(l, ku): the other half of the pair, from memory
          if (il < up)  // the rebuilt cluster meets the clusters before it
            append_pair(((unsigned)up << 16) | (unsigned)il, ku, l);
          else
            append_pair(((unsigned)il << 16) | (unsigned)up, l, ku);
        }
      }
    };
    if (nupd <= ROWS) {  // (the usual case) one pass
      int ks[ROWS], kres[ROWS], us[ROWS];
      float patch[ROWS];
      bool anyres = false;
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const unsigned e = r < nupd ? sh.upd[r] : 0u;
        ks[r] = r < nupd ? rec_k(e) : -1;
        kres[r] = (r < nupd && rec_rescan(e)) ? ks[r] : -1;
        us[r] = r;
        patch[r] = r < nupd ? sh.updv[r] : INF;
        anyres |= kres[r] >= 0;
      }
      load_rows(ks);
      if (anyres) rescan_rows(kres, us, patch);
      LAP(3);
      test_rows(0);
    } else {
      for (int u = 0; u < nupd;) {  // the flagged rows, ROWS at a time
        int ks[ROWS], us[ROWS];
        float patch[ROWS];
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          ks[r] = -1;
          us[r] = 0;
          patch[r] = INF;
        }
        for (; u < nupd && cnt < ROWS; u++) {
          const unsigned e = upd_at(u);
          if (!rec_rescan(e)) continue;
          const int k = rec_k(e);
          const float pv = updv_at(u);
#pragma unroll
          for (int r = 0; r < ROWS; r++)
            if (r == cnt) {
              ks[r] = k;
              us[r] = u;
              patch[r] = pv;
            }
          cnt++;
        }
        if (cnt == 0) break;
        load_rows(ks);
        rescan_rows(ks, us, patch);
      }
      LAP(3);
      for (int u0 = 0; u0 < nupd; u0 += ROWS) {
        int ks[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) ks[r] = u0 + r < nupd ? rec_k(upd_at(u0 + r)) : -1;
        load_rows(ks);
        test_rows(u0);
      }
    }
    // -- C: candidates with the merged cluster j, behind all others (:2033-2064)
    {
      unsigned cand = 0;
#pragma unroll
      for (int q = 0; q < MAXQ; q++) {
        if (q >= nq) break;
        const int k = a_k[q];
        const bool ok = k >= 0 && k != i && k != j && cj[q] <= min_value_j;
        cand |= ok ? 1u << q : 0u;
      }
      while (cand) {  // (few)
        const int q = __ffs((int)cand) - 1;
        cand &= cand - 1;
        const int k = slot_k(q);
        if (MMY(j, k) <= mv_now(q, k)) append_pair(0x80000000u | (unsigned)(q * MM_BLOCK + tid), k, j);
      }
    }
    __syncthreads();
    LAP(4);
    // -- D: the pairs in the reference's order
    const int m = __builtin_amdgcn_readfirstlane(sh.npairs);
    if (m - MM_PAIRS_LDS > p.pair_cap) {
      bail = 2;
      break;
    }
    auto pair_at = [&](int side, int e, unsigned &key, unsigned &xy, float &sym) {
      if (e < MM_PAIRS_LDS) {
        key = sh.pk[side][e];
        xy = sh.pxy[side][e];
        sym = sh.psym[side][e];
      } else {
        auto g = p.pair_g + ((size_t)side * p.pair_cap + (size_t)(e - MM_PAIRS_LDS)) * 3;
        key = g[0];
        xy = g[1];
        sym = __uint_as_float(g[2]);
      }
    };
    // Every pair's symmetric distance (tree_builder.cpp:1699-1702): d(y,x) + d(x,y), or 0 when the pair is also
    // mutually closest under the prior -- one element M[x][y] per pair, all pairs at once -- and its place in the
    // reference's order (rank = number of smaller keys).
    int side = m > 0 ? 1 : 0;
    bool bucketed = false;
    if constexpr (AGES) bucketed = m > MM_BUCKET_MIN;
    if (bucketed) {
      // A merge that sends most clusters through the rebuilding branch has tens of thousands of feasible pairs and the
      // rank above is quadratic: the pairs are counted per later cluster (bucket n: the merged cluster's), moved to
      // their bucket, and ranked inside it -- sides 0 -> 1 -> 0.  (Counts are read back past the L1: atomics do not
      // update it.)
      auto pair_put = [&](int sd, int e, unsigned key, unsigned xy, float sym) {
        if (e < MM_PAIRS_LDS) {
          sh.pk[sd][e] = key;
          sh.pxy[sd][e] = xy;
          sh.psym[sd][e] = sym;
        } else {
          auto g = p.pair_g + ((size_t)sd * p.pair_cap + (size_t)(e - MM_PAIRS_LDS)) * 3;
          g[0] = key;
          g[1] = xy;
          g[2] = __float_as_uint(sym);
        }
      };
      auto bucket_of = [&](unsigned key) -> int { return (key & 0x80000000u) ? n : (int)(key >> 16); };
      auto count_of = [&](int b) -> int { return __hip_atomic_load(&p.bucket[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
      for (int x = tid; x <= n; x += MM_BLOCK) __hip_atomic_store(&p.bucket[x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      for (int e = tid; e < m; e += MM_BLOCK) {
        unsigned key, xy;
        float sym;
        pair_at(0, e, key, xy, sym);
        __hip_atomic_fetch_add(&p.bucket[bucket_of(key)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      int run = 0;
      for (int x0 = 0; x0 <= n; x0 += MM_BLOCK) {
        const int x = x0 + tid;
        const int c = x <= n ? count_of(x) : 0;
        int tot;
        const int off = block_scan(c, &tot, sh.wave_i);
        if (x <= n) p.bucket_off[x] = run + off;
        run += tot;
        __syncthreads();
      }
      for (int x = tid; x <= n; x += MM_BLOCK) __hip_atomic_store(&p.bucket[x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      for (int e = tid; e < m; e += MM_BLOCK) {
        unsigned key, xy;
        float sym;
        pair_at(0, e, key, xy, sym);
        const int b = bucket_of(key);
        const int at = p.bucket_off[b] + __hip_atomic_fetch_add(&p.bucket[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pair_put(1, at, key, xy, 0.0f);
      }
      __syncthreads();
      for (int e = tid; e < m; e += MM_BLOCK) {
        unsigned key, xy;
        float sym;
        pair_at(1, e, key, xy, sym);
        const int b = bucket_of(key);
        const int lo = p.bucket_off[b], hi = lo + count_of(b);
        int rank = lo;
        for (int g = lo; g < hi; g++) {
          unsigned kg, xg;
          float sg;
          pair_at(1, g, kg, xg, sg);
          rank += kg < key ? 1 : 0;
        }
        const int x = (int)(xy >> 16), y = (int)(xy & 0xffffu);
        const f32x4 f = MM(x, y);
        sym = f.y + f.x;
        if (p.has_prior && f.z <= st.mvcf[x] && f.w <= (y == j ? mvcf_j : st.mvcf[y])) sym = 0.0f;
        // (side 0 is read by nobody any more: every thread is past its last pair_at(0, ...) -- the barrier above)
        pair_put(0, rank, key, xy, sym);
      }
      __syncthreads();
      side = 0;
    } else if (m > 0) {
      for (int e = tid; e < m; e += MM_BLOCK) {
        unsigned key, xy;
        float sym;
        pair_at(0, e, key, xy, sym);
        const int x = (int)(xy >> 16), y = (int)(xy & 0xffffu);
        const f32x4 f = MM(x, y);  // (d(x,y), d(y,x), cf(x,y), cf(y,x))
        int rank = 0;
        const int ml = min(m, MM_PAIRS_LDS);
        for (int g = 0; g < ml; g++) rank += sh.pk[0][g] < key ? 1 : 0;
        for (int g = MM_PAIRS_LDS; g < m; g++) rank += p.pair_g[(size_t)(g - MM_PAIRS_LDS) * 3] < key ? 1 : 0;
        sym = f.y + f.x;
        if (p.has_prior && f.z <= st.mvcf[x] && f.w <= (y == j ? mvcf_j : st.mvcf[y])) sym = 0.0f;
        if (rank < MM_PAIRS_LDS) {
          sh.pk[1][rank] = key;
          sh.pxy[1][rank] = xy;
          sh.psym[1][rank] = sym;
        } else {
          auto g = p.pair_g + ((size_t)p.pair_cap + (size_t)(rank - MM_PAIRS_LDS)) * 3;
          g[0] = key;
          g[1] = xy;
          g[2] = __float_as_uint(sym);
        }
      }
      __syncthreads();
    }
    if (p.timers && tid == 0) sh.tacc[9] += m;  // (pairs drawn)
    LAP(5);
    // -- E (first half): the merged-away cluster leaves the list, the rebuilt marks are taken back -- under the
    // ordered part, which names clusters, not positions, from here on (the symmetric path, rare, keeps the list
    // until it is through)
    const bool sym_now = AGES || sh.use_sym != 0;  // (the AGES walk names positions: the list stays until it is through)
    // The positions behind i move up by one: a lane takes its neighbour's cluster, the last lane of a wave the first
    // lane's of the next wave (sh.edge, written before the barrier between the two halves).
    auto erase_read = [&]() {
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
          if (q >= nq) break;
          sh.edge[wave][q] = (short)a_k[q];
        }
      }
      for (int u = tid; u < nupd; u += MM_BLOCK) st.flag[rec_k(upd_at(u))] = 0;
    };
    auto erase_write = [&]() {
      const int ipos = sh.ipos;
      const bool mirror = CI_ALWAYS || sh.use_sym != 0;
#pragma unroll
      for (int q = 0; q < MAXQ; q++) {
        if (q >= nq) break;
        const int ik = q * MM_BLOCK + tid;
        // (lane l takes lane l + 1's: one DPP move across the wave, wave_shl:1; lane 63 -- it keeps -1 -- from the edge)
        int nx = __builtin_amdgcn_update_dpp(-1, a_k[q], 0x130, 0xf, 0xf, false);
        if (lane == 63) {
          if (wave + 1 < MM_WAVES) nx = sh.edge[wave + 1][q];
          else if (q + 1 < MAXQ) nx = sh.edge[0][q + 1];
          else nx = -1;
        }
        if (ik >= ipos) {
          a_k[q] = ik + 1 < n ? nx : -1;
          if (mirror && ik + 1 < n) st.ci[ik] = (cidx_t)nx;
        }
      }
      if (tid == 0) sh.n = n - 1;
    };
    // The best among the clusters that keep their candidate (a copy taken before the draws: they may still
    // change such a cluster's candidate, behind its turn)
    float ud = INF, ud2 = INF;
    double ud2d = (double)INF;  // (AGES)
    int upos = n, bl1 = -1, bl2 = -1;
    if (wave == 0) {
      ud = lane < MM_WAVES ? sh.lex_d[lane] : INF;
      ud2 = lane < MM_WAVES ? sh.lex_d2[lane] : INF;
      upos = lane < MM_WAVES ? sh.lex_p[lane] : n;
      const int upos_mine = upos;
      if constexpr (AGES) {
        ud2d = lane < MM_WAVES ? sh.lex_d2d[lane] : (double)INF;
        wave_lex_min_d(ud, ud2d, upos);
      } else {
        wave_lex_min(ud, ud2, upos);
      }
      if (upos < n) {  // (the cluster at that position: its wave left it in lex_k)
        const unsigned long long from = __ballot(lane < MM_WAVES && upos_mine == upos);
        const int kb = sh.lex_k[__builtin_ctzll(from)];
        bl1 = st.lin1[kb];
        bl2 = st.lin2[kb];
      }
    }
    if (!sym_now) {
      erase_read();
      __syncthreads();
      erase_write();
    }
    if (p.timers && tid == 0) sh.tacc[10] += wall_clock64() - sh.tmark;  // (of "ordered": before the first draw)
    if constexpr (AGES) {
      if (wave == 0) {
        // Coalesce's loop over the clusters in order (:613-881 / :2085-2341) as far as candidates go: a cluster that
        // is the LATER one of feasible pairs gets them at its turn (the reset of a rebuilt one happened in A: nothing
        // reaches a slot before its cluster's turn -- pairs are applied at the turn of their later cluster), then the
        // running best looks at what the cluster holds.  64 positions are fetched at a time; the empty ones are
        // skipped, and what was fetched for a cluster is what it holds at its turn unless it has pairs of its own.
        abest = AgeCand{INF, (double)INF, MM_AGE_EMPTY, sh.best.lin1, sh.best.lin2};  // (:611)
        int e = 0;
        unsigned key = 0x80000000u, xy = 0;
        float sym = 0.0f;
        if (m > 0) pair_at(side, 0, key, xy, sym);
        // One of the clusters that keep their candidate holds one within the clock (A): the best of the merge is the
        // smallest such candidate -- theirs, or what a cluster with pairs of its own holds behind them, or the merged
        // cluster's.  Otherwise: the walk.
        const bool reduced = upos < n;
        if (reduced) {
          AgeCand sb{INF, (double)INF, MM_AGE_EMPTY, -1, -1};
          int spos = n;
          while (e < m && !(key & 0x80000000u)) {
            const int cur = (int)(key >> 16);
            AgeCand t{INF, (double)INF, MM_AGE_EMPTY, -1, -1}, ys;
            while (e < m && !(key & 0x80000000u) && (int)(key >> 16) == cur) {
              const int x = (int)(xy >> 16), y = (int)(xy & 0xffffu);
              const float symc = sym;
              e++;
              if (e < m) pair_at(side, e, key, xy, sym);
              apply_ages(x, y, symc, t, ys);
            }
            if (t.lv <= a_lw && t.d < INF && (sb.d > t.d || (sb.d == t.d && sb.d2 > t.d2))) {  // (ascending positions)
              sb = t;
              spos = cur;
            }
          }
          abest = AgeCand{ud, ud2d, 0, bl1, bl2};
          if (spos < n && (sb.d < ud || (sb.d == ud && (sb.d2 < ud2d || (sb.d2 == ud2d && spos < upos))))) abest = sb;
        }
        for (int base = 0; base < n && !reduced; base += 64) {
          const int pos_l = base + lane;
          const int k_l = pos_l < n ? (int)st.ci[pos_l] : -1;
          const bool valid = k_l >= 0 && k_l != i && k_l != j;
          AgeCand r{INF, (double)INF, MM_AGE_EMPTY, -1, -1};
          if (valid) r = slot_of(k_l);
          unsigned long long mask = __ballot(valid && r.lv != MM_AGE_EMPTY);
          for (;;) {
            const unsigned key_u = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const int pnext = (e < m && !(key_u & 0x80000000u)) ? (int)(key_u >> 16) : 0x7fffffff;
            const int pa = mask ? base + (int)__builtin_ctzll(mask) : 0x7fffffff;
            const int pb = pnext < base + 64 ? pnext : 0x7fffffff;
            const int ppos = min(pa, pb);
            if (ppos == 0x7fffffff) break;
            const int ln = __builtin_amdgcn_readfirstlane(ppos - base);
            mask &= ~(1ull << ln);
            AgeCand t;
            if (ppos == pb) {  // its own pairs first
              AgeCand ys;
              t = AgeCand{INF, (double)INF, MM_AGE_EMPTY, -1, -1};
              while (e < m && !(key & 0x80000000u) && (int)(key >> 16) == ppos) {
                const int x = (int)(xy >> 16), y = (int)(xy & 0xffffu);
                const float symc = sym;
                e++;
                if (e < m) pair_at(side, e, key, xy, sym);
                apply_ages(x, y, symc, t, ys);
              }
            } else {
              const long long bits = __double_as_longlong(r.d2);
              const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(bits & 0xffffffffll), ln);
              const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), ln);
              t.d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.d), ln));
              t.d2 = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
              t.lv = __builtin_amdgcn_readlane(r.lv, ln);
              t.l1 = __builtin_amdgcn_readlane(r.l1, ln);
              t.l2 = __builtin_amdgcn_readlane(r.l2, ln);
            }
            best_takes(t);
          }
        }
        // the merged cluster: new minima, an empty slot, its pairs (:883-963 / :2343-2353), the last look of the best
        const int szi = st.csz[i], szj = st.csz[j];
        const int li = st.alv[i], lj = st.alv[j];
        if (lane == 0) {
          st.mv[j] = min_value_j;
          if (p.has_prior) st.mvcf[j] = mvcf_j;
          st.mcd[j] = INF;
          st.d2d[j] = (double)INF;
          st.lv[j] = (hidx_t)MM_AGE_EMPTY;
        }
        AgeCand js{INF, (double)INF, MM_AGE_EMPTY, -1, -1};
        while (e < m) {
          const int x = (int)(xy >> 16);
          const float symc = sym;
          e++;
          if (e < m) pair_at(side, e, key, xy, sym);
          AgeCand xs;
          apply_ages(x, j, symc, xs, js);
        }
        if (reduced) {
          if (js.lv <= a_lw && js.d < INF && (abest.d > js.d || (abest.d == js.d && abest.d2 > js.d2))) abest = js;
        } else {
          best_takes(js);
        }
        // ages[j], the clock (:1219-1226 / :2513-2524: with a prior it steps before the lineage count drops)
        const int newl = max(li, lj);
        const double before = a_age;
        if (p.has_prior) a_age = __dadd_rn(a_age, ages_step(a_lins, p.Ne));
        a_lins--;
        while (a_level < newl) {
          a_level++;
          a_lins += p.ages_count[a_level];
        }
        if (!p.has_prior) a_age = __dadd_rn(a_age, ages_step(a_lins, p.Ne));
        if (!(a_age >= before)) a_lw = -1;  // (0 or 1 lineages: the step is not a number the clock can add)
        clock_reaches();
        if (lane == 0) {
          st.alv[j] = (cidx_t)newl;
          sh.a_lw = a_lw;
          sh.best.dist = abest.d;
          sh.best.lin1 = abest.l1;
          sh.best.lin2 = abest.l2;
          st.csz[j] = (cidx_t)(szi + szj);
          sh.nupd = 0;
          sh.npairs = 0;
        }
      }
    } else if (wave == 0) {
      // the clusters whose candidates change, at their turn: after their own pairs
      float sd = INF, sd2 = INF;
      int sl1 = -1, sl2 = -1, spos = n;
      int cur = -1, curk = -1;
      auto settle = [&]() {
        const float d1 = st.mcd[curk], d2 = st.mcd2[curk];
        const int c1 = st.lin1[curk], c2 = st.lin2[curk];
        if (sd > d1 || (sd == d1 && sd2 > d2)) {
          sd = d1;
          sd2 = d2;
          sl1 = c1;
          sl2 = c2;
          spos = cur;
        }
      };
      int e = 0;
      unsigned key = 0, xy = 0;
      float sym = 0.0f;
      if (m > 0) pair_at(side, 0, key, xy, sym);
      for (; e < m; e++) {
        if (key & 0x80000000u) break;
        const int pos = (int)(key >> 16), x = (int)(xy >> 16), y = (int)(xy & 0xffffu);
        const float symc = sym;
        if (e + 1 < m) pair_at(side, e + 1, key, xy, sym);  // the next record, requested along with this pair's reads
        if (pos != cur) {
          if (cur >= 0) settle();
          cur = pos;
          curk = x;
        }
        apply(x, y, symc);
      }
      if (cur >= 0) settle();
      // the loop's running "best": smallest (dist, dist2), the earliest cluster among exact ties
      Best b;
      b.dist = INF;
      b.dist2 = INF;
      b.lin1 = sh.best.lin1;
      b.lin2 = sh.best.lin2;
      int pos = n;
      if (upos < n) {
        b.dist = ud;
        b.dist2 = ud2;
        b.lin1 = bl1;
        b.lin2 = bl2;
        pos = upos;
      }
      if (spos < n) {
        if (b.dist > sd || (b.dist == sd && (b.dist2 > sd2 || (b.dist2 == sd2 && spos < pos)))) {
          b.dist = sd;
          b.dist2 = sd2;
          b.lin1 = sl1;
          b.lin2 = sl2;
          pos = spos;
        }
      }
      if (lane == 0) {
        st.mv[j] = min_value_j;
        if (p.has_prior) st.mvcf[j] = mvcf_j;
        st.mcd[j] = INF;
        st.mcd2[j] = INF;
      }
      for (; e < m; e++) {
        const int x = (int)(xy >> 16);
        const float symc = sym;
        if (e + 1 < m) pair_at(side, e + 1, key, xy, sym);
        apply(x, j, symc);
      }
      const float jd = st.mcd[j], jd2 = st.mcd2[j];
      if (b.dist > jd || (b.dist == jd && b.dist2 > jd2)) {
        b.dist = jd;
        b.dist2 = jd2;
        b.lin1 = st.lin1[j];
        b.lin2 = st.lin2[j];
      }
      if (lane == 0) {
        sh.best = b;
        st.csz[j] = (cidx_t)(int)added;  // (exact integers in floats)
        sh.nupd = 0;
        sh.npairs = 0;
      }
    }
    LAP(6);
    // -- the same merge in the symmetric matrix once it is in use (coalesce_sym, tree_builder.cpp:968-1058)
    if (sh.use_sym) {
      if (tid == 0) sh.count = 0;  // (thread 0 is past its ordered part; the others wait at the barrier below)
      __syncthreads();
      for (int ik = tid; ik < n; ik += MM_BLOCK) {
        const int k = st.ci[ik];
        if (k == j || k == i) continue;
        // (the symmetric matrix is symmetric bit for bit -- a float sum commutes, and the two updates below
        //  apply one formula to equal operands --: the column entries are read from the rows of i and j)
        const float dik = SS(i, k), djk = SS(j, k), dkj = djk, dki = dik;
        const float mvk = p.min_values_sym[k];
        if (dik != djk) SS(j, k) = (csi * dik + csj * djk) / added;
        if (dki != dkj) SS(k, j) = (csi * dki + csj * dkj) / added;
        if (dkj != dki) {
          if ((double)fabsf(mvk - dkj) < 1e-6 || (double)fabsf(mvk - dki) < 1e-6)
            p.upd_pos[atomicAdd(&sh.count, 1)] = ik;  // rows to rescan
        } else {
          if (p.mcs_lin1[k] == i) p.mcs_lin1[k] = j;
          if (p.mcs_lin2[k] == i) p.mcs_lin2[k] = j;
        }
      }
      __syncthreads();
      const int nres_s = sh.count;
      for (int r = 0; r < nres_s; r++) {
        const int k = st.ci[p.upd_pos[r]];
        const float old = p.min_values_sym[k];
        auto row = symm + (size_t)k * N;
        float fm = INF, fm2 = 0.0f;
        int fpos = n, pos_old = n, pos_less = n;
        for (int il = tid; il < n; il += MM_BLOCK) {
          const int l = st.ci[il];
          if (l != i && l != k) {
            const float x = row[l];
            if (x < fm) {
              fm = x;
              fpos = il;
            }
            if (x == old) pos_old = min(pos_old, il);
            if (x < old) pos_less = min(pos_less, il);
          }
        }
        float dummy = 0.0f;
        block_min3(dummy, pos_old, pos_less, sh.wave_f, sh.wave_i, sh.wave_i2);
        block_lex_min(fm, fm2, fpos, sh.wave_f, sh.wave_f2, sh.wave_i3);
        if (tid == 0) {
          const bool stops = pos_old < n && pos_old < pos_less;
          const float x = stops ? old : fm;
          const int at = stops ? pos_old : fpos;
          p.min_values_sym[k] = x;
          p.mcs_dist[k] = x;
          if (x < INF) {
            p.mcs_lin1[k] = k;
            p.mcs_lin2[k] = st.ci[at];
          }
        }
      }
      __syncthreads();
      float b1 = INF, b2 = 0.0f, mj = INF, mj2 = 0.0f;
      int bp = n, mjp = n;
      auto srowj = symm + (size_t)j * N;
      for (int ik = tid; ik < n; ik += MM_BLOCK) {
        const int k = st.ci[ik];
        if (k == j || k == i) continue;
        const float dk = p.mcs_dist[k];
        if (dk < b1) {
          b1 = dk;
          bp = ik;
        }
        const float sj = srowj[k];
        if (sj < mj) {
          mj = sj;
          mjp = ik;
        }
      }
      block_lex_min(b1, b2, bp, sh.wave_f, sh.wave_f2, sh.wave_i);
      block_lex_min(mj, mj2, mjp, sh.wave_f, sh.wave_f2, sh.wave_i3);
      if (tid == 0) {
        Best b = sh.best_sym;
        b.dist = INF;
        if (bp < n && b1 < INF) {
          const int k = st.ci[bp];
          b.dist = b1;
          b.lin1 = p.mcs_lin1[k];
          b.lin2 = p.mcs_lin2[k];
        }
        p.min_values_sym[j] = mj;
        p.mcs_dist[j] = mj;  // (INF when nothing is left)
        if (mjp < n && mj < INF) {
          p.mcs_lin1[j] = st.ci[mjp];
          p.mcs_lin2[j] = j;
        }
        if (b.dist > mj) {
          b.dist = mj;
          b.lin1 = p.mcs_lin1[j];
          b.lin2 = p.mcs_lin2[j];
        }
        sh.best_sym = b;
      }
    }
    if (sym_now) {
      __syncthreads();
      erase_read();
      __syncthreads();
      erase_write();
    }
    LAP(7);
    __syncthreads();
    LAP(8);
  }
  if (bail < 0) {
    if constexpr (LAY != L_GLOBAL) {  // the carried state goes out (pinned host memory)
      for (int c = tid; c < N; c += MM_BLOCK) {
        p.io_lin[c] = (int)st.lin1[c];
        p.io_lin[(size_t)N + c] = (int)st.lin2[c];
        p.io_mvcf[c] = st.mvcf[c];
      }
    }
    if (tid == 0 && p.timers) {
      sh.tacc[11] = (clock64() - cstart) * 100 / (wall_clock64() - tstart + 1);  // shader clock, MHz
      for (int x = 0; x < 16; x++) p.timers[x] = sh.tacc[x];
    }
    bail = 0;
  }
  __threadfence_system();  // every wave's part of the tree and of the carried state
  __syncthreads();
  leave(bail);
#undef LAP
}

}  // namespace
}  // namespace rl
