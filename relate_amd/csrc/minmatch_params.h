// minmatch_params.h -- what the host and the device side of the GPU tree builder must agree on: the constants of a
// build, the layout of the woven matrix, where the per-cluster state lives, and a tree's parameters (MMParams).
// For the build's device code (minmatch_build.h) and both units, minmatch_worker.hip and minmatch_builder.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace rl {

constexpr int MM_BLOCK = 512;   // (8 waves; a thread keeps ~10 clusters of a merge in registers.  256 threads: 166 ms per N = 5000 tree, 1024: 156, 512: 110)
constexpr int MM_WAVES = MM_BLOCK / 64;
constexpr int MM_HITS = 64;       // mutually close pairs per row the weave keeps; more: the build scans that stretch of rows itself
constexpr int MM_UPD_MAX = 512;   // rebuilt clusters of one merge; more: the host builds the tree (the AGES build keeps a longer list)
constexpr int MM_UPD_LDS = 256;   // ... of which this many in LDS, the rest in global memory
constexpr int MM_PAIRS_LDS = 320; // feasible pairs of one merge kept in LDS (8 per merge on average); more go through global scratch
constexpr int MM_BUCKET_MIN = 2048;  // (the AGES build) more pairs than this are put in order bucket by bucket
// M is stored in column panels of 64: element (a, b) at ((b / 64) * N + a) * 64 + b % 64.  A row is N / 64 runs of
// 1 KB (a wavefront's 64 consecutive clusters: one run), 64 * N elements apart; a COLUMN -- what a merge scatters its
// one store per cluster down -- strides by 1 KB inside one panel of N KB, a few 2 MB pages, instead of by a whole
// row (80 KB at N = 5000: every store on another page, the address translation of 2500 pages per merge).
// (Rows in blocks of 128, so that a row spans fewer pages: no gain, DESIGN_NOTES.md 5.)
constexpr int MM_PANEL = 64;  // (narrower panels -- a column's stores 128 / 256 / 512 B apart instead of 1 KB -- are no faster:
                              //  118.1 / 115.5 / 114.9 ms per tree against 114.7, profiles/r06_panel_width.json)
__host__ __device__ inline unsigned mm_index(unsigned a, unsigned b, unsigned N) {
  return ((b / MM_PANEL) * N + a) * MM_PANEL + (b % MM_PANEL);
}
__host__ __device__ inline size_t mm_elements(size_t N) { return ((N + MM_PANEL - 1) / MM_PANEL) * N * MM_PANEL; }
constexpr int MM_MAXN = 10240;    // one thread holds up to 20 clusters of a merge in registers
constexpr int MM_Q_LDS = 5120 / MM_BLOCK, MM_Q_GLOB = MM_MAXN / MM_BLOCK;  // register slots per thread: N <= 5120 / N <= 10240
constexpr int MM_Q_SMALL = 2048 / MM_BLOCK;                                // ... and N <= 2048
// Where the per-cluster state of a build lives:
//   L_HOT    (the plain build, every N): what a merge reads or writes for EVERY cluster or on the ordered part's path --
//            the candidate (dist, dist2, lin1, lin2) and the rebuilt mark, 13 bytes per cluster -- in LDS; the rest
//            (row minima of both matrices, sizes, the live list) in global memory, read with the rows of a merge or
//            kept in registers.  65 KB at N = 5000: TWO workgroups per CU, 130 KB at N = 10,000;
//   L_LDS    (the AGES build, N <= 4100) everything in LDS, 33 bytes per cluster;
//   L_GLOBAL (the AGES build above that) everything in the global arrays of MMParams.
//   L_WARM   L_HOT with the row minima of both matrices in LDS too (21 bytes per cluster): one workgroup per CU.
enum { L_LDS = 0, L_GLOBAL = 1, L_HOT = 2, L_WARM = 3 };

// A tree's parameters.  The matrices of a build, woven: M[a][b] = (d(a,b), d(b,a), cf(a,b), cf(b,a)).  A merge needs,
// per cluster k, the entries (i,k), (k,i), (j,k), (k,j) of both matrices: two 16-byte loads along the rows of i and j
// instead of four loads along rows and four down columns (a scattered 4-byte access costs one CU ~3.5 cycles:
// measured 3.7 us per column of 2500 clusters, six of them per merge in the plain layout); what stays scattered is
// ONE 16-byte store per cluster, M[k][j], which waits for nobody.  Packed from the distance matrix (K3 + carrier
// penalty) and the clade prior by weave_kernel; row minima of both by the penalty / prior passes (rowmin_penalty_kernel,
// prior_kernel).
//
// One field list, two structs of the same layout: MMParams (plain pointers: what the host fills in) and MMParamsDev
// (GLOBAL pointers: what the build kernel works with).  A worker reads its parameters from a queue, not from
// kernel arguments, and a pointer of unknown address space compiles to flat_load / flat_store, which count against
// the LDS counter too and turn every wait for an LDS read into a wait for the loads in flight -- the phases of a
// merge overlap exactly these two.
#define MM_PARAM_FIELDS(PTR)                                                                                         \
  int N;                                                                                                             \
  int layout; /* L_LDS / L_GLOBAL / L_HOT: where the per-cluster state lives for the build */                       \
  float threshold, threshold_CF;                                                                                     \
  PTR(MM_F4) M; /* [N*N] destroyed */                                                                                \
  int has_prior; /* the cf halves of M are in use */                                                                 \
  PTR(const float) rowmin_D; /* [N] minimum of each row off the diagonal */                                          \
  PTR(const float) rowmin_CF;                                                                                        \
  /* the mutually close pairs (a, b > a) of the untouched matrix, row by row in order, from weave_kernel   */       \
  PTR(const int) hit_cnt;    /* [N] (more than MM_HITS: not all kept) */                                             \
  PTR(const unsigned) hit_b; /* [N][MM_HITS] */                                                                      \
  PTR(const float) hit_sym;  /* [N][MM_HITS] symmetric distance of the pair (0: the prior makes it a certain pair) */ \
  /* room for the symmetric matrix of the fallback (rare): a pool of the device, `sym_slots` matrices of N*N floats \
     at SYM, taken with a compare-and-swap on sym_locks[slot] when a tree first needs one and given back when it    \
     is out; none free (or no pool): the tree is the host's */                                                       \
  PTR(float) SYM;                                                                                                    \
  PTR(int) sym_locks;                                                                                                \
  int sym_slots;                                                                                                     \
  PTR(float) min_values_sym;                                                                                         \
  PTR(float) mcs_dist;                                                                                               \
  PTR(int) mcs_lin1;                                                                                                 \
  PTR(int) mcs_lin2;                                                                                                 \
  PTR(float) min_values; /* min_values_CF, mc_lin1, mc_lin2: carried from tree to tree (in and out) */               \
  PTR(float) min_values_CF;                                                                                          \
  /* (pinned host memory; L_LDS and L_HOT) where the worker reads the carried state and leaves it again: candidate  \
     indices [2N], min_values_CF [N] -- L_GLOBAL: the host copies to and from the arrays above */                    \
  PTR(int) io_lin;                                                                                                   \
  PTR(float) io_mvcf;                                                                                                \
  PTR(float) mc_dist;                                                                                                \
  PTR(float) mc_dist2;                                                                                               \
  PTR(int) mc_lin1;                                                                                                  \
  PTR(int) mc_lin2;                                                                                                  \
  PTR(int) cluster_index;                                                                                            \
  PTR(int) cluster_size;                                                                                             \
  PTR(unsigned char) kflag;                                                                                          \
  PTR(int) upd_pos;     /* [N] scratch of the symmetric path */                                                      \
  PTR(unsigned) pair_g; /* [6 * pair_cap] feasible pairs of a merge beyond MM_PAIRS_LDS: key, x<<16|y, sym */        \
  PTR(int) rowlist;     /* [MM_WAVES][N] pair-scan survivors per wave */                                             \
  PTR(int) merge_i;     /* [N-1] the merges as (cluster i, cluster j) in order: the host names the nodes from them */ \
  PTR(int) merge_j;                                                                                                  \
  PTR(int) status;                                                                                                   \
  /* (pinned host memory) the status again, stored when everything else of the tree is out and flushed: the         \
     builder's host thread watches it and takes its tree while the other workers still build theirs */              \
  PTR(volatile int) host_done;                                                                                       \
  long long pair_cap;                                                                                                \
  PTR(long long) timers; /* optional: 100 MHz ticks per phase (RELATE_AMD_TIMING) */                                 \
  PTR(unsigned) trace;   /* optional (RELATE_AMD_TIMING=2): [0] merge, [1] phase the workgroup has reached */     \
  /* --sample_ages (the AGES build): the candidates' draw as a double and their third key as the INDEX of the age   \
     among the sorted distinct sample ages (MM_AGE_EMPTY: no candidate); per cluster the index of its oldest sample \
     (age_lvl0: as the samples are, age_lvl: the build's own copy); the distinct ages, how many samples have each */ \
  PTR(double) mc_dist2d;                                                                                             \
  PTR(int) mc_lvl;                                                                                                   \
  PTR(int) age_lvl;                                                                                                  \
  PTR(const int) age_lvl0;                                                                                           \
  PTR(const double) unique_ages;                                                                                     \
  PTR(const int) ages_count;                                                                                         \
  int n_levels;                                                                                                      \
  int Ne; /* pipeline/BuildTopology.cpp:36 */                                                                        \
  /* the rebuilt clusters of a merge beyond MM_UPD_LDS (with sample ages a renamed candidate follows its lineage up  \
     the tree, :2342, and a merge of that lineage sends every cluster holding one through the rebuilding branch) */  \
  PTR(unsigned) upd_g; /* [N] */                                                                                     \
  PTR(float) updv_g;   /* [N] */                                                                                     \
  /* ... and, for a merge with thousands of feasible pairs, the pairs per later cluster: counts / fill marks and    \
     offsets */                                                                                                      \
  PTR(int) bucket;     /* [N + 1] */                                                                                 \
  PTR(int) bucket_off; /* [N + 1] */
#define MM_HOST_PTR(T) T *
#define MM_GLOBAL_PTR(T) __attribute__((address_space(1))) T *
// (a class type -- HIP's float4 -- has no member functions outside the generic address space: the device struct
//  takes the elements of M as native vectors)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define MM_F4 float4
struct MMParams {
  MM_PARAM_FIELDS(MM_HOST_PTR)
};
#undef MM_F4
#define MM_F4 f32x4
struct MMParamsDev {
  MM_PARAM_FIELDS(MM_GLOBAL_PTR)
};
#undef MM_F4
static_assert(sizeof(MMParams) == sizeof(MMParamsDev), "one layout");
constexpr int MM_PARAM_WORDS = 104;  // sizeof(MMParams) / 4 rounded up (static_assert below)
static_assert(sizeof(MMParams) % 4 == 0 && sizeof(MMParams) / 4 <= MM_PARAM_WORDS, "MM_PARAM_WORDS");

}  // namespace rl
