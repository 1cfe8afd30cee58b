/*
 * relate_amd.h -- C ABI of the MI355X-native Relate Paint -> BuildTopology path.
 *
 * Plain C types only (no torch, no C++ types).  Every entry point names the
 * reference interface it replaces; paths are relative to
 * /root/reference/include (MyersGroup/relate @ 2025-04-10).
 *
 * Conventions
 *   - all functions return 0 on success and a negative RL_E* code on failure;
 *     rl_last_error() returns a thread-local description of the last failure
 *     (the reference asserts / exit(1)s instead: pipeline/Paint.cpp:24,78).
 *   - caller owns every host buffer passed in or out; device memory is owned
 *     by the rl_ctx / rl_window objects.
 *   - one rl_ctx per host thread and GPU.  No CPU fallback exists: functions
 *     that need the GPU fail with RL_ENODEVICE when none is visible.
 */
#ifndef RELATE_AMD_H
#define RELATE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  RL_OK = 0,
  RL_EINVAL = -1,    /* bad argument                                  */
  RL_ENODEVICE = -2, /* no usable HIP device                          */
  RL_EHIP = -3,      /* HIP runtime error (see rl_last_error)         */
  RL_EIO = -4,       /* file could not be opened / read / written     */
  RL_EFORMAT = -5,   /* malformed chunk / paint file                  */
  RL_ESTATE = -6,    /* call sequence error (e.g. paint before load)  */
  RL_ENOMEM = -7,
  RL_ETIMEOUT = -8   /* a segmented rl_paint gave up waiting for a hand-off */
};

/* Summation order of the per-site normalising constants.
 *   RL_SUM_EXACT : the reference's serial left-to-right order over donors
 *                  n = 0..N-1 (src/fast_painting.cpp:300-303, 495-503),
 *                  reproduced bit for bit by a parallel algorithm
 *                  (relate_amd/csrc/exact_sum.h).  Paint files / .anc / .mut
 *                  are byte-identical to the reference's.
 *   RL_SUM_EXACT_SERIAL : the same result computed literally (one dependent
 *                  add per donor); slower, kept as the in-kernel fallback of
 *                  RL_SUM_EXACT and for cross-checking it.
 *   RL_SUM_LANES : per-lane partial sums + wavefront xor-butterfly.  Same
 *                  arithmetic, different association: distances agree to
 *                  ~1e-7 relative before min-subtraction, trees may differ
 *                  where MinMatch breaks float ties.
 *   RL_SUM_LANES32 : the FAST mode.  As RL_SUM_LANES, with the per-donor state of
 *                  the stepping-stone pass (rl_paint) in packed FP32 instead of
 *                  double (the stones are floats in the reference too,
 *                  fast_painting.cpp:241-245); sums, factors, logscales and all of
 *                  RePaintSection stay double.  Distances within 1e-5 *
 *                  max(|d|, |logscale|) of the reference's (asserted in the
 *                  tests); NOT byte-identical files.                           */
enum { RL_SUM_EXACT = 0, RL_SUM_LANES = 1, RL_SUM_EXACT_SERIAL = 2, RL_SUM_LANES32 = 3 };

typedef struct rl_ctx rl_ctx;
typedef struct rl_window rl_window;

const char *rl_last_error(void);
const char *rl_version(void);
/* number of visible HIP devices (0 when none; never initialises a context) */
int rl_device_count(void);

/* ---------------------------------------------------------------- context */
rl_ctx *rl_create(int device);
/* A process that runs one stage and ends (the CLI, relate_amd/csrc/main.cpp) says so: the device blocks its contexts
 * release then stay in the library's cache until the process is gone instead of going back to the driver one hipFree
 * at a time (C3: ~3000 blocks, 4 s).  No reference counterpart (the reference frees with the process too). */
void rl_keep_cache_until_exit(int on);
void rl_destroy(rl_ctx *ctx);

/* Replaces `Data::Data(chunk files)` (src/data.cpp:86-97) + the parameter
 * read of pipeline/Paint.cpp:23-31: loads <dir>/parameters_c<c>.bin and
 * <dir>/chunk_<c>.{hap,r,rpos,bp,dist,state}. */
int rl_load_chunk(rl_ctx *ctx, const char *dir, int chunk_index);

/* Same, from memory (what a cgo/JNI-style binding of the reference's `Data`
 * struct, src/data.hpp:44-103, would pass).  seq: L*N chars '0'/'1',
 * SNP-major; r: L; rpos: L+1; wb: W+1 window boundaries (wb[W]==L). */
int rl_set_chunk(rl_ctx *ctx, int N, int L, const uint8_t *seq,
                 const double *r, const double *rpos, const int *wb, int W);
/* Same, panel already bit-packed (bit n of row s = derived), row_words
 * uint32 per row. */
int rl_set_chunk_bits(rl_ctx *ctx, int N, int L, const uint32_t *bits,
                      int row_words, const double *r, const double *rpos,
                      const int *wb, int W);

/* `--painting theta,rho` (pipeline/Paint.cpp:38-61): data.theta = theta,
 * data.r[l] *= rho.  Must precede rl_paint / rl_window_open. */
int rl_set_painting(rl_ctx *ctx, double theta, double rho);

/* Target-haplotype sharding of ONE chunk (BASELINE.json config #5):
 * this context paints, re-paints and measures targets k_begin .. k_end-1 only
 * (default: all).  The panel is replicated; stepping stones, posteriors and
 * distance-matrix rows are held for those targets only (1/G of the memory on G
 * GPUs).  Every per-target output below then has k_end-k_begin rows in target
 * order; the caller all-gathers the distance rows (rl_window_matrix_rows_device
 * + RCCL, relate_amd/dist.py) for the tree builder.  No reference counterpart:
 * the reference shards a chunk by section only (RelateParallel.sh:231-257).
 * Call after rl_set_chunk / rl_load_chunk and before rl_prepare / rl_paint. */
int rl_set_target_range(rl_ctx *ctx, int k_begin, int k_end);
int rl_target_range(const rl_ctx *ctx, int *k_begin, int *k_end);

/* Window range of ONE chunk: rl_paint keeps the stepping stones of windows w_first .. w_last only (default: all W).
 * The reference deals a chunk out by section range, one BuildTopology process per range
 * (scripts/RelateParallel/RelateParallel.sh:231-257), and section w reads window w alone: the alpha stone at its begin
 * boundary and the beta stone at its end boundary (DistanceMeasure::GetTopologyWithRepaint, src/anc_builder.cpp:49-78;
 * written at src/fast_painting.cpp:354-374 and :559-578).  A range other than the default one also ends the passes
 * where their last stone is written: the forward pass of target k at the begin boundary of w_last, the backward pass at
 * the end boundary of w_first.  The stone buffers hold w_last - w_first + 1 windows; every entry point that takes a
 * window (rl_get_stones, rl_paint_record, rl_write_paint_file, rl_window_open* without a paint file) refuses one
 * outside the painted range with RL_ESTATE and a message naming the range, and rl_write_paint_files, which writes
 * every window, refuses any range but the default.  A bad range is RL_EINVAL before the device is touched.  Call after
 * rl_set_chunk / rl_load_chunk; after rl_paint it marks the context unpainted, as rl_set_target_range does, but the
 * plan and its uploads (rl_prepare) stay: they do not depend on the range. */
int rl_set_window_range(rl_ctx *ctx, int w_first, int w_last);
int rl_window_range(const rl_ctx *ctx, int *w_first, int *w_last);

int rl_chunk_dims(const rl_ctx *ctx, int *N, int *L, int *W);
/* sum_k D_k: visited (target, site) pairs of the chunk; 2*N*this is the
 * number of directional haplotype-pair.SNP updates of one Paint. */
long long rl_total_sites(rl_ctx *ctx);

/* ------------------------------------------------------------------ Paint */
/* Builds the per-target visited-site plan (host; src/fast_painting.cpp:41-157),
 * uploads panel + plan and allocates the stepping-stone buffers, so that a
 * following rl_paint finds everything resident in HBM.  Optional: rl_paint
 * does the same on first use. */
int rl_prepare(rl_ctx *ctx);

/* Replaces the hot loop `for hap: FastPainting::PaintSteppingStones`
 * (pipeline/Paint.cpp:81-87, src/fast_painting.cpp:18-618) for all N
 * targets: forward/backward Li-Stephens over the bit-packed panel, stepping
 * stones (alpha, beta, logscales at window boundaries) left in HBM.
 * kernel_ms (optional) receives the GPU time of the kernels (HIP events). */
int rl_paint(rl_ctx *ctx, int sum_mode, float *kernel_ms);
/* rl_paint normally paints both directions in ONE launch (2 workgroups per
 * target: the passes are independent in this stage, fast_painting.cpp:207-378
 * vs :380-586).  split != 0: one launch per direction (backward, then forward),
 * which is what rl_paint_times reports on. */
int rl_set_paint_split(rl_ctx *ctx, int split);
/* K1's FP64 kernels come in up to four variants per register tile, fitted to how far the N donors fill it
 * (relate_amd/csrc/launch.h tile_fit): fit != 0 (the default) runs the one the rule picks for the chunk, fit = 0
 * always the loose one, which every N of the tile may run.  The stones are the same bit for bit either way; the
 * switch is there to time and to test the one against the other. */
int rl_set_paint_fit(rl_ctx *ctx, int fit);
/* The merged launch may cut every pass into segments that hand their state over through HBM and deal the segments
 * segment by segment over all targets, so that all passes advance together and the launch ends with a full chip
 * (DESIGN.md "Segmented passes").  backward / forward: segments per backward / forward pass; 1 = off (one workgroup
 * per pass, the unsegmented kernels), 0 = automatic (the default): off when the launch's 2 * targets workgroups all
 * fit the chip at once -- there is no tail to fill then --, else the measured default.  The stones are the same bit
 * for bit for any setting.  RL_SUM_EXACT_SERIAL, RL_SUM_LANES32 and rl_set_paint_split never segment.  A segmented
 * launch whose hand-off does not arrive within tens of seconds (it normally waits not at all) gives up:
 * rl_paint returns RL_ETIMEOUT.  RL_EINVAL for a count below 0 or above 64. */
int rl_set_paint_segments(rl_ctx *ctx, int backward, int forward);
/* What the next rl_paint of the context will use in the RL_SUM_EXACT and RL_SUM_LANES orders (1, 1: unsegmented).
 * Needs a chunk; the automatic rule asks the device for its CUs.  One exception: the loose variant of the S = 8 tile
 * has no segmented kernel in the RL_SUM_LANES order (N <= 512 under rl_set_paint_fit(ctx, 0), or q < 4): this call
 * then reports the RL_SUM_EXACT order's answer and the RL_SUM_LANES Paint runs unsegmented. */
int rl_paint_segments(rl_ctx *ctx, int *backward, int *forward);
/* What the last rl_paint did launch: the segments per backward / forward pass of its merged launch, (1, 1) for the
 * unsegmented kernels whatever the setting (serial order, RL_SUM_LANES32, rl_set_paint_split, no twin).  RL_ESTATE
 * before the first rl_paint. */
int rl_paint_launched_segments(const rl_ctx *ctx, int *backward, int *forward);
/* The bounds rule of the segments, pure host code (the kernels run the same function): segment s of seg walks
 * [*first, *last) of the step range [lo, hi) -- every step once, in order; empty segments where hi - lo < seg.
 * RL_EINVAL unless 0 <= s < seg. */
int rl_paint_segment_range(int lo, int hi, int seg, int s, int *first, int *last);
/* The rule itself, pure host code: the tile of N haplotypes (S, waves as rl_register_tile reports them), the number
 * `tail` of its last registers that take the backward pass's validity masks and the number `live` of registers that
 * hold a donor in some lane (S or S - 1).  Any pointer may be NULL.  RL_EINVAL for N < 2 or N > 10240.
 * This is the rule, not necessarily the kernel launched: rl_set_paint_fit(ctx, 0) overrides it, RL_SUM_LANES32 has
 * one kernel per tile, and RL_SUM_LANES keeps the loose variant at S = 32 with one wave and S = 64 with two
 * (launch.h tile_fit_built). */
int rl_tile_fit(int N, int *S, int *waves, int *tail, int *live);
/* HIP-event durations of the last rl_paint's two launches (forward kernel,
 * backward kernel), in milliseconds; both 0 unless rl_set_paint_split(ctx, 1). */
int rl_paint_times(const rl_ctx *ctx, float *fwd_ms, float *bwd_ms);
/* What the last rl_paint was launched with: fwd_steps / bwd_steps, the steps of the forward loop
 * (src/fast_painting.cpp:262-376) and of the backward loop (:457-580) summed over the context's targets -- sum_k D_k - 1
 * each for the default window range, sum_k stone_ia[k][w_last] and sum_k D_k - 1 - stone_ie[k][w_first] under
 * rl_set_window_range --, and stone_bytes, the stone storage it asked for (2 * windows * targets * N floats).  Any
 * pointer may be NULL. */
int rl_paint_account(const rl_ctx *ctx, long long *fwd_steps, long long *bwd_steps, long long *stone_bytes);
/* Register tile of the loaded chunk: S doubles per lane, `waves` wavefronts
 * per target (relate_amd/csrc/launch.h) -- which kernel instantiation runs. */
int rl_register_tile(const rl_ctx *ctx, int *S, int *waves);

/* Test hook: `batch` arrays of n doubles each are summed with the summation
 * machinery of the painting kernels (sum_mode as for rl_paint); out[b]
 * receives the sum of array b.  RL_SUM_EXACT and RL_SUM_EXACT_SERIAL must
 * return the left-to-right IEEE sum bit for bit.  1 <= n <= 10240: an array
 * gets the waves a target of N = n donors gets (two for n > 5120).
 * rl_debug_wave_sum_ex: one workgroup sums rows_per_group consecutive arrays
 * in order (batch a multiple of it), as a step loop of the kernels does.
 * mismatch == NULL: the terms are x; else (uint8 [batch][n]) they are
 * (mismatch ? th : nth) * x, read through a lane-mask panel as in the
 * backward passes.  stats8 (may be NULL) receives the path counters of
 * RL_SUM_EXACT, counted per wave: sums, serial fallbacks, walked lanes,
 * multi-binade reruns, then four cycle counts.  sum_mode may carry
 * RL_DEBUG_SUM_STASH (with RL_SUM_EXACT and a mismatch array only): the
 * terms are computed once into the wave's LDS stash and every pass of the sum
 * reads them back, as the exact backward pass of rl_paint does; geometry and
 * counters as without it.  RL_DEBUG_SUM_REGSTASH (same conditions, not
 * together with RL_DEBUG_SUM_STASH): the terms split three ways as that pass
 * splits them -- the first through the stash, the last held in registers from
 * the loop that computed them, the rest recomputed (rl_debug_term_split).
 * Bad arguments: RL_EINVAL before any device work. */
#define RL_DEBUG_SUM_STASH 0x100
#define RL_DEBUG_SUM_REGSTASH 0x200
int rl_debug_wave_sum(const double *x, int n, int batch, int sum_mode, double *out);
int rl_debug_wave_sum_ex(const double *x, int n, int batch, int rows_per_group, int sum_mode,
                         const uint8_t *mismatch, double th, double nth, double *out,
                         unsigned long long *stats8);
/* Host only: of the S weighted terms of a backward step of register tile S
 * (8, 16, 32, 48, 64, 80), the exact order keeps the first *ks in LDS and the
 * last *r in registers and recomputes the rest.  RL_EINVAL for another S. */
int rl_debug_term_split(int S, int *ks, int *r);
/* Host only: the exact order's hop over a tie lane (relate_amd/csrc/exact_sum.h) for the entry offsets delta_lo ..
 * delta_hi.  A4: the exit offsets of the lane's four runs, p0 in 0..3, sh in 0..1.  out_reference[delta - delta_lo]:
 * the literal form A_h + ((delta - B_h) >> sh), h = (p0 + delta) & 3; out_table[...]: the same through the packed
 * table the kernels walk (walk_table_pack, walk_table_hop).  *packable = 0 where an entry of the table is no int16
 * (the kernels then redo that lane from its exact entry value); out_table is zeroed.  RL_EINVAL for bad arguments. */
int rl_debug_walk_table(const int *A4, int p0, int sh, int delta_lo, int delta_hi, int *packable, int *out_table,
                        int *out_reference);
/* Host only: the exact order's walk over the lanes of one wave (relate_amd/csrc/exact_sum.h walk_enter, walk_leave).
 * records: [lanes][7] ints {kind, U_0, U_1, U_2, U_3, p0, sh}, 1 <= lanes <= 64.  RL_WALK_TRANSLATION: delta -> delta + U_0
 * (any int, modulo 2^32).  RL_WALK_TABLE: a head, delta -> (delta >> sh) + U_h, h = (p0 + delta) & 3, every U_h an
 * int16.  RL_WALK_CONSTANT: a head whose exit offset is U_0 (an int16) whatever came before.  entry_delta: the offset
 * on entry of lane 0.  *out_literal: the exit offset lane by lane, a table lane in the literal form
 * (walk_hop_reference); *out_scan: as the kernels compute it, from the inclusive add-scan of the translations and a
 * walk over the heads.  RL_EINVAL for bad arguments. */
#define RL_WALK_TRANSLATION 0
#define RL_WALK_TABLE 1
#define RL_WALK_CONSTANT 2
int rl_debug_walk_lanes(const int *records, int lanes, int entry_delta, int *out_literal, int *out_scan);
/* Test hook: what a device block of the library's memory cache holds when it is handed out.  Takes a block for `bytes`
 * bytes as every device buffer of the library does, copies all of it to `out` (*got bytes: a cached block may be up
 * to bytes / 8 + 4096 bytes larger than asked for, and `out` must hold bytes + bytes / 8 + 4096 bytes; a larger block
 * is RL_ENOMEM and nothing is copied), then, if fill >= 0, writes the byte `fill` (0..255) over the whole block on the
 * device, and gives the block back to the cache.  The cache returns a block as it was left: with
 * RELATE_AMD_TEST_POISON unset a second call of the same size sees the first call's fill, with it set every call sees
 * the poison byte. */
int rl_debug_alloc_peek(size_t bytes, int fill, unsigned char *out, size_t *got);

/* Experiment builds only (kernels compiled with -DRL_STATS and
 * RELATE_AMD_TEST_STATS set): 16 event counters of the last rl_paint. */
int rl_debug_stats(rl_ctx *ctx, unsigned long long *out16);
/* ... and all 32 (16..24: cycles of the forward / backward step by segment, paint_kernels.hip) */
int rl_debug_stats32(rl_ctx *ctx, unsigned long long *out32);
/* Experiment builds (-DRL_STATS) with RELATE_AMD_TEST_TIMELINE set: when every workgroup of the last merged rl_paint was
 * resident -- [*groups][2] counts of the device's 100 MHz wall clock at its start and end (tools/paint_timeline.py).
 * cap: the pairs `out` holds; out may be NULL.  RL_ESTATE in the product build. */
int rl_debug_timeline(rl_ctx *ctx, unsigned long long *out, long long cap, long long *groups);

/* Copy stepping stones of window w to the host: alpha, beta: N*N floats
 * ([target][donor]); ls_alpha, ls_beta: N floats; bsnp_begin/end: N ints.
 * Any pointer may be NULL. */
int rl_get_stones(rl_ctx *ctx, int w, float *alpha, float *beta,
                  float *ls_alpha, float *ls_beta, int *bsnp_begin,
                  int *bsnp_end);

/* Replaces the dump at src/fast_painting.cpp:589-601 +
 * CollapsedMatrix::DumpToFile (src/collapsed_matrix.hpp:228-265): writes
 * <paint_dir>/relate_<w>.bin for every window, byte-compatible with the
 * reference (lossy RLE included). */
int rl_write_paint_files(rl_ctx *ctx, const char *paint_dir);
/* One window's file only (what a section-parallel consumer of the reference,
 * scripts/RelateParallel/RelateParallel.sh:231-257, reads), at `path`. */
int rl_write_paint_file(rl_ctx *ctx, int w, const char *path);
/* One record of window w's paint file: target k's `int start, int end`, then
 * the alpha and the beta stone as CollapsedMatrix::DumpToFile writes them
 * (src/fast_painting.cpp:589-601, src/collapsed_matrix.hpp:228-265) -- the
 * bytes FastPainting::PaintSteppingStones(data, wb, pfiles, k) appends to
 * pfiles[w].  Two rows of N floats leave the device.  *len receives the
 * record's length; with out == NULL only the bound a buffer needs. */
int rl_paint_record(rl_ctx *ctx, int w, int k, unsigned char *out, size_t cap, size_t *len);

/* The whole `Relate --mode Paint` stage (pipeline/Paint.cpp:17-108): load,
 * optional --painting, mkdir chunk_<c>/paint, paint, write files. */
int rl_stage_paint(const char *out_dir, int chunk_index, int use_painting,
                   double theta, double rho, int sum_mode, int device);

/* ------------------------------------------------------- RePaint + matrix */
/* Replaces DistanceMeasure::GetTopologyWithRepaint
 * (src/anc_builder.cpp:49-106): decodes window w's stepping stones from
 * paint_file (or, if NULL, from the stones resident after rl_paint, passed
 * through the same float/RLE quantisation the file applies) and runs
 * FastPainting::RePaintSection (src/fast_painting.cpp:621-1092) for all N
 * targets.  The posterior rows (`topology`) and logscales stay in HBM.
 * first_snp initialises the cursors v_snp_prev / v_rpos_prev / v_rpos_next
 * (anc_builder.cpp:81-101). */
rl_window *rl_window_open(rl_ctx *ctx, int w, const char *paint_file,
                          int first_snp, int sum_mode, float *kernel_ms);
/* The same with at most max_rows posterior rows resident (0 = all of them).
 * The reference's DistanceMeasure keeps the whole window (`topology`,
 * src/anc_builder.hpp:58, filled at anc_builder.cpp:75-78); a tree at `snp`
 * reads two rows per target and the tree builder only moves forward
 * (anc_builder.cpp:487-495), so a bounded window keeps the rows from its
 * cursors onwards and runs RePaintSection again (same operations, same bits)
 * when rl_window_matrix is asked for a SNP past them.  N = 5000 keeps 20 GB
 * per window otherwise, which bounds how many sections one GPU serves.
 * rl_window_repaints: how many times RePaintSection has run for the window. */
rl_window *rl_window_open_bounded(rl_ctx *ctx, int w, const char *paint_file,
                                  int first_snp, int sum_mode,
                                  long long max_rows, float *kernel_ms);
int rl_window_repaints(const rl_window *win);
/* Tests: where the window's last RePaint launch put target t (global index).
 * out8 = row_lo, row_hi (the resident posterior rows [lo, hi)), start_row,
 * save_row (the kept backward state the launch started from / left, -1:
 * none), fstart_row, fsave_row (the forward state likewise), 1 if the launch
 * was a part launch, 1 if its backward kernel ran without the LDS strip.
 * Host bookkeeping only: nothing is launched, no kernel argument changes.
 * RL_EINVAL for a null window or output and for t outside the window's
 * targets. */
int rl_debug_window_place(const rl_window *win, int t, int32_t *out8);
void rl_window_close(rl_window *win);
int rl_window_bounds(const rl_window *win, int *start, int *end);
/* rows D_n of target n's topology and copies of it (tests / debugging):
 * top: D_n*N floats in donor order, logscales: D_n floats. */
int rl_window_rows(const rl_window *win, int n);
int rl_window_get_topology(rl_window *win, int n, float *top,
                           float *logscales);

/* AncesTreeBuilder::BuildTopology's cursor update for the carriers of `snp`
 * (src/anc_builder.cpp:487-495). */
int rl_window_advance(rl_window *win, int snp);
/* Replaces DistanceMeasure::GetMatrix(snp) (src/anc_builder.cpp:109-207):
 * N*N float distance matrix at `snp` (the rows of the context's targets, all
 * by default), row-min subtracted, into d_host
 * (may be NULL to leave the result on the device only).
 * kernel_ms optional. */
int rl_window_matrix(rl_window *win, int snp, float *d_host, float *kernel_ms);
/* The same, written to a caller-owned DEVICE buffer of (targets of the
 * context) * N floats -- the send buffer of the all-gather when the chunk is
 * sharded by target (rl_set_target_range). */
int rl_window_matrix_rows_device(rl_window *win, int snp, void *d_rows, float *kernel_ms);
/* The same with what AncesTreeBuilder::BuildTopology does to the matrix next folded into the kernel's last pass over
 * each row: carriers (N flags, host memory; NULL: none) -- the carrier penalty of src/anc_builder.cpp:563-581,
 * d[c][j] += val along a carrier's row, -= val again at carrier columns --, and d_rowmin (device, one float per row
 * of the context's targets; NULL: not wanted) -- the row minima off the diagonal MinMatch::Initialize starts from
 * (src/tree_builder.cpp:1659-1666), of the rows as they then are. */
int rl_window_matrix_rows_device_ex(rl_window *win, int snp, void *d_rows, const char *carriers, float val,
                                    void *d_rowmin, float *kernel_ms);

/* --------------------------------------------------------------- host side */
/* Replaces MinMatch::QuickBuild (src/tree_builder.cpp:1061-1303 without
 * prior, :2358-2644 with prior) for sample_ages == empty: builds the tree
 * from the asymmetric N*N matrix d (destroyed).  parent[2N-1] receives the
 * parent of every node (-1 for the root); child_left/child_right (optional)
 * the children of the N-1 internal nodes N..2N-2. */
int rl_quickbuild(int N, double theta, float *d, const float *d_prior,
                  int *parent, int *child_left, int *child_right);
/* The same as an object, the way AncesTreeBuilder::BuildTopology uses one
 * MinMatch for all trees of a section (src/anc_builder.cpp:436, :447, :608):
 * the builder keeps what MinMatch keeps from one QuickBuild to the next
 * (min_values_CF, the stale candidate indices -- they steer the random
 * draws).  device >= 0: trees are built on that GPU, one workgroup per tree
 * with the matrices in HBM (src/tree_builder.cpp restated in
 * relate_amd/csrc/minmatch_build.h); a tree that needs the symmetric
 * fallback (tree_builder.cpp:255-293, :968-1058) is built by the host code
 * with the same state.  device < 0: the host builder.  d is destroyed.
 * rl_builder_last_on_gpu: 1 if the last tree was built on the GPU. */
typedef struct rl_builder rl_builder;
rl_builder *rl_builder_create(int N, double theta, int device);
int rl_builder_build(rl_builder *b, float *d, const float *d_prior,
                     int *parent, int *child_left, int *child_right);
/* MinMatch::QuickBuild's sample_ages (N doubles): from here on the builder's trees are built with the sample-age
 * key and clock of src/tree_builder.cpp:1123-1233 / :2407-2531 -- on the builder's device (device >= 0), else on the
 * host. */
int rl_builder_set_sample_ages(rl_builder *b, const double *ages, int n);
int rl_builder_last_on_gpu(const rl_builder *b);
void rl_builder_destroy(rl_builder *b);
/* Test hook (host only): what the lists of the last tree the HOST builder of `b` built had to hold -- the first n of
 * 9 counts: the most clusters rebuilt in one merge, merges with more than MM_UPD_LDS (256) of them; the most feasible
 * pairs (draws) of one merge, merges with more than MM_PAIRS_LDS (320) and with more than MM_BUCKET_MIN (2048); the
 * draws of the initialisation; the most mutually close partners b > a of one row a; the first merge taken from the
 * symmetric matrix (-1: none) and how many were.  The device builder is the same algorithm with the same draws:
 * whether its lists hold a tree follows from these (tests/builder_cases.py).  Returns 9. */
int rl_builder_census(const rl_builder *b, long long *out, int n);
/* Test hook (needs a device): the worker kernel that builds trees of N leaves (ages != 0: with sample ages) in this
 * process -- where the per-cluster state lives (0 LDS, 1 global memory, 2 the candidates in LDS, 3 candidates and row
 * minima in LDS), register slots per thread (4 / 10 / 20) and workgroups per CU (RELATE_AMD_BUILD_OCC is read once
 * per process). */
int rl_debug_builder_kind(int N, int ages, int *layout, int *slots, int *per_cu);
/* Test hook (host only): the device builder's restatement of std::mt19937 +
 * libstdc++'s uniform_real_distribution<double> against the library itself,
 * n draws from `seed`; returns how many differ. */
int rl_debug_rng_mismatches(unsigned seed, int n);
/* Measurement hook (tools/bench_builder_many.py): `builders` device builders, one host thread each, build the same tree
 * (d, prior: N*N floats, prior may be NULL) `reps` times side by side, the matrices staying on the device, with at most
 * `workers` resident workgroups (0: the queue's own limit).  seconds: wall-clock of all builds; mismatches: builds
 * whose parent array differs from builder 0's of the same repetition; first_parents (may be NULL): builder 0's
 * [reps][2N-1].  MinMatch::QuickBuild, src/tree_builder.cpp:2358-2644. */
int rl_debug_builder_throughput(int N, double theta, int device, int builders, int reps, int workers, const float *d,
                                const float *prior, double *seconds, int *mismatches, int *first_parents);
/* Test hook (host only): the stage's rule for how many resident tree-builder workgroups it asks for -- never more
 * than open sections (a section has one tree in flight: the unit of parallelism of
 * scripts/RelateParallel/RelateParallel.sh:231-257); 7/8 of the worker slots with whole windows resident, 29/64 of the
 * CUs (times the kernel's workgroups per CU) when the windows are bounded and RePaint runs all through the stage. */
int rl_debug_stage_worker_goal(int cus, int open_sections, int bounded_windows, int workers_per_cu);
/* Test hook (host only): how a stage sizes itself against HBM (relate_amd/csrc/stage_plan.h plan_sections), from plain
 * numbers.  In: the chunk's sizes (S, waves: a posterior row is S * 64 * waves floats); rows_of[num_windows], the
 * posterior rows of every section's window; the sections of the call; whether a window holds stones of its own (a
 * stage from paint files, or stones parked in host memory); trees on the device or the host; `room`, 0.9 of the free
 * HBM, if known; this rank's host threads; the knobs as the stage resolves them (environment, rl_stage_opts,
 * fallback: window_rows and section_threads with whether they were set at all, window_parts, repaint_lanes).
 * Out: ints_out[6] = section threads, sections the estimate sees open at once, rows a window keeps (0: all), second
 * RePaint lane wanted (0 / 1), its strips' bytes, and for `probe_section` the smallest cached block that counts as
 * room for its window; doubles_out[6] = the largest window's rows, bytes per row, per window next to its rows, per
 * device builder, per bounded window's kept RePaint states, and of `probe_section`'s open window. */
int rl_debug_stage_plan(int N, int nloc, int S, int waves, const double *rows_of, int num_windows, int first_section,
                        int last_section, int stones_per_window, int gpu_build, int room_known, double room,
                        int host_threads, int window_rows_set, long long window_rows, long long window_parts,
                        int section_threads_set, long long section_threads, long long repaint_lanes, int probe_section,
                        long long *ints_out, double *doubles_out);

/* Tree-sequence loop of one section, AncesTreeBuilder::BuildTopology
 * (src/anc_builder.cpp:398-656): first tree from the distance matrix at
 * `start`, then for every SNP map its carriers onto the current tree
 * (MapMutation, :1064-1139) and rebuild (carrier penalty + previous-tree clade
 * prior, :555-606; MinMatch) when it does not map.  The distance matrices come
 * from a provider: `matrix(user, snp, d)` must fill the N*N matrix of
 * DistanceMeasure::GetMatrix(snp) and `advance(user, snp)` (may be NULL) is
 * called for every SNP start < snp < end before its matrix can be requested
 * (the cursor update of :487-495).  rl_stage_build_topology plugs rl_window
 * in; any other DistanceMeasure implementation can be plugged the same way.
 * bits/row_words: bit-packed panel as for rl_set_chunk_bits; bp_pos (L, only
 * for --fb) and state (L, chunk_<c>.state) may be NULL.
 * flags bit0 = --no_consistency; fb = --fb (0 = off). */
typedef struct rl_treeseq rl_treeseq;
typedef int (*rl_matrix_fn)(void *user, int snp, float *d);
typedef int (*rl_advance_fn)(void *user, int snp);
rl_treeseq *rl_treeseq_create(int N, int L, const uint32_t *bits, int row_words,
                              const double *rpos, const int *bp_pos,
                              const int *state, double theta);
void rl_treeseq_destroy(rl_treeseq *ts);
/* sample ages (N doubles; n = 0: none) for the trees of rl_treeseq_build: MinMatch::QuickBuild's sample_ages argument
 * (src/anc_builder.cpp:373-390). */
int rl_treeseq_set_sample_ages(rl_treeseq *ts, const double *ages, int n);
/* device >= 0: rl_treeseq_build builds its trees on that GPU (see rl_builder_create),
 * < 0 (default): on the host. */
int rl_treeseq_set_build_device(rl_treeseq *ts, int device);
/* With a build device: where the distance matrix of `snp` comes from when it
 * is to stay on the device (N*N floats at d_dev, e.g. through
 * rl_window_matrix_rows_device); carrier penalty, clade prior and the build
 * then run there too and no matrix crosses PCIe. */
typedef int (*rl_matrix_dev_fn)(void *user, int snp, void *d_dev);
int rl_treeseq_set_device_matrix(rl_treeseq *ts, rl_matrix_dev_fn matrix_dev);
/* ... and a provider that also applies the carrier penalty and leaves the row minima (rl_window_matrix_rows_device_ex):
 * with it the device builder skips its own pass over the matrix.  carriers: N flags or NULL. */
typedef int (*rl_matrix_dev_ex_fn)(void *user, int snp, void *d_matrix, const char *carriers, float val,
                                   void *d_rowmin);
int rl_treeseq_set_device_matrix_ex(rl_treeseq *ts, rl_matrix_dev_ex_fn matrix_dev_ex);
int rl_treeseq_build(rl_treeseq *ts, int start, int end, rl_matrix_fn matrix,
                     rl_advance_fn advance, void *user, int flags, int fb);
int rl_treeseq_num_trees(const rl_treeseq *ts);
/* position (first SNP) and parent array (2N-1, root = -1) of tree t */
int rl_treeseq_get_tree(const rl_treeseq *ts, int t, int *pos, int *parent);
/* AncesTree::DumpBin (src/anc.cpp:1104-1167) and Mutations::DumpShortFormat
 * (src/mutations.cpp:548-581); either path may be NULL. */
int rl_treeseq_write(const rl_treeseq *ts, const char *anc_path,
                     const char *mut_path);

/* The whole `Relate --mode BuildTopology` stage
 * (pipeline/BuildTopology.cpp:14-167) for sections first..last: writes
 * <out>/chunk_<c>/<out>_<section>.anc and .mut.
 * flags: bit0 = --no_consistency, fb = --fb value (0 = off). */
int rl_stage_build_topology(const char *out_dir, int chunk_index,
                            int first_section, int last_section,
                            int use_painting, double theta, double rho,
                            int flags, int fb, int sum_mode, int device);

/* Everything a stage call can be told, per call (the positional entry points above and below take the reference's
 * command-line options only: pipeline/BuildTopology.cpp:20-40).  rl_stage_opts_init fills in the defaults and the
 * struct's size; a caller built against an older header passes a shorter struct and gets the defaults for the rest;
 * a struct whose size field was never set (0) is refused with RL_EINVAL.
 * 0 / -1 = "decide from the chunk and the device" wherever noted.  The RELATE_AMD_* environment variables of the
 * same names override the struct -- they exist for experiments (tools/, profiles/), not as the interface. */
typedef struct rl_stage_opts {
  size_t size;              /* sizeof(rl_stage_opts), set by rl_stage_opts_init                                   */
  int sum_mode;             /* RL_SUM_*                                                                            */
  int device;               /* HIP device                                                                          */
  int use_painting;         /* --painting given: theta, rho (pipeline/Paint.cpp:38-61)                             */
  double theta, rho;
  int flags;                /* bit 0: --no_consistency                                                             */
  int fb;                   /* --fb (0: off)                                                                       */
  const char *sample_ages_path; /* --sample_ages (NULL: none); replaces rl_stage_set_sample_ages                   */
  int gpu_build;            /* trees on the device (1), on the host (0); -1: device when several sections are asked for */
  long long window_rows;    /* posterior rows a window keeps resident; 0: from the HBM that is free; < 0: all      */
  int window_parts;         /* a window keeps at least 1/window_parts of its rows (0: 32)                          */
  int section_threads;      /* sections open at once at most (0: from HBM and the device)                          */
  int workers;              /* tree-builder workgroups on the device (0: the rule of stage.cpp stage_worker_goal -- one per open section, 29/64 of the CUs when the windows are bounded, times the kernel's workgroups per CU) */
  int repaint_lanes;        /* RePaint launches side by side: 1 or 2 (0: 1)                                        */
  int park_stones;          /* fused stage: stepping stones to pinned host memory after Paint (rl_park_stones)     */
  int pin_threads;          /* section threads pinned to L3 groups: 1 / 0 (-1: 1)                                  */
  int find_equivalent_branches; /* 1: the next stage, FindEquivalentBranches (pipeline/FindEquivalentBranches.cpp:13-167), fused
                               behind BuildTopology -- the sections' trees are associated in memory while other sections
                               still build, every .anc is written ONCE, as that stage would leave it (same bytes as
                               BuildTopology followed by rl_stage_find_equivalent_branches).  Only for a call that covers
                               all sections of the chunk; host memory: ~0.3 MB per tree at N = 5000                  */
  int paint_windows;        /* fused stage (rl_stage_paint_build_topology_ex): 1 / -1 (default): Paint keeps the windows of
                               [first_section, min(last_section, W-1)] only (rl_set_window_range), what one process of
                               scripts/RelateParallel/RelateParallel.sh:231-257 reads; 0: every window, as before            */
} rl_stage_opts;
void rl_stage_opts_init(rl_stage_opts *opts);
int rl_stage_paint_ex(const char *out_dir, int chunk_index, const rl_stage_opts *opts);
int rl_stage_build_topology_ex(const char *out_dir, int chunk_index, int first_section,
                               int last_section, const rl_stage_opts *opts);
int rl_stage_paint_build_topology_ex(const char *out_dir, int chunk_index, int first_section,
                                     int last_section, const rl_stage_opts *opts);

/* DEPRECATED (process-wide state): use rl_stage_opts.sample_ages_path.
 * `--sample_ages <file>` of BuildTopology (pipeline/BuildTopology.cpp:93-108; ancient samples): the file (plain or
 * gzip text, one age per haplotype) the FOLLOWING rl_stage_build_topology / rl_stage_paint_build_topology calls of
 * this process read; NULL or "" for none.  With ages the trees are built by the host's sequential restatement of
 * MinMatch's third candidate key and coalescence clock (src/tree_builder.cpp:7-22, 149-252, 601-965, 1123-1233,
 * 1738-1841, 2073-2355, 2407-2531). */
int rl_stage_set_sample_ages(const char *file);

/* Paint and BuildTopology of one chunk in one process, as `Relate --mode All` runs
 * them back to back per chunk (pipeline/Relate.cpp:257-283): the stepping stones
 * never leave HBM -- no chunk_<c>/paint/relate_<w>.bin (2.4 GB per 20 windows at
 * N = 5000) is written or read; the float / run-length quantisation the file
 * would apply (src/collapsed_matrix.hpp:228-296) is applied on the device.  Same
 * .anc / .mut as rl_stage_paint followed by rl_stage_build_topology. */
/* (between rl_paint and the windows of a context, for chunks whose stones would not leave room for the sections'
 * windows) moves the painted stepping stones to pinned host memory and frees their HBM; a window opened without a
 * paint file afterwards takes its slice back.  What the fused stage does under RELATE_AMD_PARK_STONES=1. */
int rl_park_stones(rl_ctx *ctx);

int rl_stage_paint_build_topology(const char *out_dir, int chunk_index,
                            int first_section, int last_section,
                            int use_painting, double theta, double rho,
                            int flags, int fb, int sum_mode, int device);

/* ---------------------------------------------------- OptimizeParameters */
/* `Relate --mode OptimizeParameters` (pipeline/OptimizeParameters.cpp:22-206): for every (theta, recombination factor)
 * of a grid, the number of SNPs that do not map onto the tree built at that very SNP.
 *   rl_optimize_section replaces AncesTreeBuilder::OptimizeParameters (src/anc_builder.cpp:821-973) for one section
 *     of a context whose stepping stones are painted (rl_paint): RePaintSection with theta and r = stored r *
 *     rec_factor (OptimizeParameters.cpp:151-157; the stones are NOT re-painted, as in the reference, where
 *     Paint(options, c) at :159 reads the chunk files afresh), then a tree at every SNP from the matrix with the SNP
 *     cancelled (:869-882), MinMatch::QuickBuild without a prior, MapMutation without random flipping (:1064-1139);
 *     *count receives the SNPs whose mapping came back > 1.  The reference's `seed` argument seeds a generator the
 *     path never draws from: there is none here.  Trees on the context's GPU (RELATE_AMD_GPU_BUILD=0: on the host).
 *     The context KEEPS the grid point's theta and factor as its painting parameters afterwards: a later rl_paint
 *     would paint with them -- call rl_set_painting first if the stones are to be painted again.
 *   rl_stage_optimize_parameters replaces the loop over grid points and sections of ONE chunk
 *     (OptimizeParameters.cpp:142-177): the chunk is painted once (opts: --painting, sum_mode, device and the
 *     stage's knobs), every pair runs all sections under the BuildTopology stage's admission rule, and
 *     counts[i * n_factor + j] is ADDED TO (the caller sums over chunks, :172).  theta in (0,1), factor > 0
 *     (:92-95, :103-106), else RL_EINVAL with the reference's message. */
int rl_optimize_section(rl_ctx *ctx, int section, float theta, float rec_factor, int *count);
int rl_stage_optimize_parameters(const char *out_dir, int chunk_index, const float *theta, int n_theta,
                                 const float *factor, int n_factor, const rl_stage_opts *opts, int *counts);
/* Test hook (host only): AncesTreeBuilder::MapMutation without random flipping (src/anc_builder.cpp:1064-1139,
 * PropagateMutationGlobal :1237-1341) for the tree `parent` (2N-1 entries, root = -1, a parent's label above its
 * children's, as MinMatch numbers them) and N carrier flags: 1 = maps, 2 = maps flipped, 3 = does not map. */
int rl_debug_map_mutation(int N, const int *parent, const char *carriers);
/* Test hook: the per-tree pass of the mode over a distance matrix on the GPU (relate_amd/csrc/optimize_kernels.hip
 * cancel_rowmin_kernel): d (N*N floats, in place) gets the cancellation of src/anc_builder.cpp:869-882 for the
 * carriers, rowmin (N floats) the minimum of every row off its diagonal as the rows then are
 * (src/tree_builder.cpp:59-146 starts from them).  2 <= N <= 10240. */
int rl_debug_cancel_rowmin(float *d, int N, const char *carriers, float log_ratio, float *rowmin);

/* ------------------------------------- one chunk sharded by target haplotype */
/* BASELINE.json config #5 (N = 10,000 x L = 200k: 8 N^2 W = 288 GB of stepping stones, more than one GPU holds).
 * The reference's unit is the section (scripts/RelateParallel/RelateParallel.sh:231-257): each BuildTopology process
 * decodes the stones of ALL targets of its window, re-paints them and fills whole matrices (src/anc_builder.cpp:49-106,
 * :109-207).  Here a rank (one process per GPU) is an rl_shard: the chunk loaded with rl_set_target_range(k_begin,
 * k_end), its own targets painted (from_paint_files = 0: stones stay in HBM, W*(k_end-k_begin)*N floats per
 * direction) or their records read from the Paint stage's files (from_paint_files = 1).
 *   rl_shard_rows: rows k_begin..k_end-1 of DistanceMeasure::GetMatrix(snp) of `section` into a device buffer of
 *     (k_end-k_begin)*N floats.  The first call for a section opens its window (GetTopologyWithRepaint for the
 *     shard's targets); every call replays the cursor updates of anc_builder.cpp:487-495 from the SNP of the previous
 *     call up to snp (they are a function of the panel), so SNPs must not decrease within a section.
 *   rl_shard_release_section: the section's trees are done, its window goes.
 *   rl_shard_build_section: the tree-sequence loop of ONE section (AncesTreeBuilder::BuildTopology,
 *     anc_builder.cpp:398-656) on this rank, its OWNER: every matrix comes from `matrix` (N*N floats to the host) or
 *     -- build_device >= 0 and matrix_dev given -- from `matrix_dev` (N*N floats to a device buffer of that GPU;
 *     penalty, prior and the build run there), which the caller implements by asking every shard for its rows and
 *     exchanging them (relate_amd/dist.py run_chunk_by_targets: an RCCL all-gather per matrix).  Writes
 *     <out>/chunk_<c>/<out>_<section>.anc/.mut like rl_stage_build_topology.
 *   rl_shard_expect_builders: how many sections this rank will own at once with build_device >= 0 (sizes the device
 *     tree builder's worker pool); 0 when done.
 *   rl_shard_set_window_rows: posterior rows a window keeps resident (rl_window_open_bounded's max_rows; 0 = all).
 *   rl_device_copy: device-to-device copy on `device` (received row blocks into the matrix_dev buffer). */
typedef struct rl_shard rl_shard;
rl_shard *rl_shard_open(const char *out_dir, int chunk_index, int k_begin, int k_end,
                        int use_painting, double theta, double rho, int sum_mode,
                        int device, int from_paint_files);
void rl_shard_close(rl_shard *s);
int rl_shard_dims(const rl_shard *s, int *N, int *L, int *W, int *k_begin, int *k_end);
int rl_shard_section_bounds(const rl_shard *s, int section, int *start, int *end);
int rl_shard_set_window_rows(rl_shard *s, long long rows);
int rl_shard_rows(rl_shard *s, int section, int snp, void *d_rows);
int rl_shard_release_section(rl_shard *s, int section);
int rl_shard_expect_builders(rl_shard *s, int builders);
int rl_shard_build_section(rl_shard *s, int section, int flags, int fb, int build_device,
                           rl_matrix_fn matrix, rl_matrix_dev_fn matrix_dev, void *user,
                           int *num_trees);
int rl_device_copy(void *dst, const void *src, size_t bytes, int device);

/* ------------------------------------------------------------ MakeChunks */
/* Replaces Data::MakeChunks (src/data.cpp:117-518): parses .haps / .sample
 * (plain or gzip) and the genetic map, decides chunks and windows from the
 * memory allowance (GB, reference default 5) and writes parameters.bin,
 * parameters_c<i>.bin, chunk_<i>.{hap,state,bp,dist,rpos,r} and props.bin into
 * the existing directory out_dir, byte-identical to the reference.  dist_fn may
 * be NULL ("unspecified").  use_transitions = 0 is --transversion. */
int rl_make_chunks(const char *haps_fn, const char *sample_fn, const char *map_fn,
                   const char *dist_fn, const char *out_dir, int use_transitions,
                   float memory_gb);
/* The `Relate --mode MakeChunks` stage (pipeline/MakeChunks.cpp:13-114):
 * refuses an existing out_dir, creates it, then rl_make_chunks. */
int rl_stage_make_chunks(const char *haps_fn, const char *sample_fn,
                         const char *map_fn, const char *dist_fn,
                         const char *out_dir, int transversion, float memory_gb);

/* ------------------------------------------------- FindEquivalentBranches */
/* The stage after BuildTopology (pipeline/FindEquivalentBranches.cpp:13-167;
 * AncesTreeBuilder::BranchAssociation / AssociateTrees, src/anc_builder.cpp:
 * 1454-1613, 658-800): reads <out_dir>/chunk_<c>/<name>_<w>.anc of every window,
 * finds equivalent branches in neighbouring trees and rewrites the files with
 * num_events / SNP_begin / SNP_end carried along them.  Host code. */
int rl_stage_find_equivalent_branches(const char *out_dir, int chunk_index);
/* Test hook (no GPU): the association fused behind BuildTopology (rl_stage_opts.find_equivalent_branches) fed from the
 * chunk's .anc FILES, sections handed over in `order` (all of them, any order), pool_threads associating. */
int rl_debug_feb_fused_from_files(const char *out_dir, int chunk_index, const int *order, int n_order,
                                  int pool_threads);

/* -------------------------------------------------------- CompareTopology */
/* Clade distance (Robinson-Foulds, rooted, unnormalised) between trees on the leaves 0..N-1, each given as the parent
 * array this library's builder returns (2N-1 ints, root = -1).  The clades of a tree are the leaf sets of its internal
 * nodes other than the root; d(A,B) = |clades(A) \ clades(B)| + |clades(B) \ clades(A)|, an integer in 0..2(N-2).
 * No reference counterpart in the pipeline (the sibling is PartitionMetric of the reference's tree_comparer); the
 * definition is the contract.  Integers throughout: the host and the device return the same numbers.
 *   A tree must be binary with labels rising from child to parent (parent[v] > v, leaves 0..N-1 childless, node 2N-2
 *   the root), as MinMatch numbers them; anything else is RL_EINVAL with a message naming the tree and the node.
 *   rl_compare_trees: parentsA / parentsB hold as many trees as `pairs` refers to (pairs[2k], pairs[2k+1] = index of
 *     pair k's tree in A / in B, >= 0); out[k] = d.  device >= 0: on that GPU (relate_amd/csrc/compare_kernels.hip,
 *     one workgroup per pair, 2 <= N <= 10240; RL_ENODEVICE without one); device < 0: the host implementation
 *     (compare.cpp), one thread, any N >= 2.
 *   rl_compare_anc: two .anc files position by position.  A file covers the SNPs from its first tree's position to
 *     the largest SNP_end of its last tree, inclusive (what BuildTopology writes there: the section's last SNP); the
 *     comparison runs over the SNPs both files cover (none: RL_EINVAL, as are different N).  The positions of the
 *     trees of both files are merged; every interval [snp_begin, snp_end) of the merge pairs one tree of A with one
 *     of B.  per_interval_path (may be NULL): a text file, one line `snp_begin snp_end treeA treeB d` per interval.
 *     summary: see the struct; mean_normalised is summed in double in interval order on the host. */
typedef struct rl_compare_summary {
  int N;                  /* leaves                                                            */
  int trees_a, trees_b;   /* trees in each file                                                */
  int intervals;          /* intervals of the merge                                            */
  int snp_begin, snp_end; /* the compared SNPs: [snp_begin, snp_end)                           */
  int max_distance;       /* largest d of an interval                                          */
  long long snps_identical; /* SNPs in intervals with d == 0                                   */
  double mean_normalised; /* sum over intervals of length * d / (2(N-2)), over snp_end - snp_begin (0 for N = 2) */
  double share_identical; /* snps_identical / (snp_end - snp_begin)                            */
} rl_compare_summary;
int rl_compare_trees(const int *parentsA, const int *parentsB, int N, int npairs, const int *pairs, int device,
                     int *out);
int rl_compare_anc(const char *ancA, const char *ancB, int device, rl_compare_summary *summary,
                   const char *per_interval_path_or_null);

/* ---------------------------------------------------- PairwiseCoalescence */
/* The most recent common ancestor (MRCA) of every pair of haplotypes, summed over a tree sequence: for trees on the
 * leaves 0..N-1 given as CompareTopology takes them (2N-1 parents, binary, parent[v] > v, node 2N-2 the root with
 * parent -1; anything else is RL_EINVAL with a message naming the tree and the node) and leaves i != j,
 *   RL_PAIRWISE_SIZE: v_t(i,j) = the number of leaves below MRCA(i,j) in tree t, an integer in 2..N (topology only);
 *   RL_PAIRWISE_TIME: v_t(i,j) = height(MRCA(i,j)), height(leaf) = 0, height(n) = height(c) + branch_length[c] with c
 *     n's first child in node order (the child_left of the reference's Tree::ReadTreeBin; the recursion of
 *     PairwiseTMRCA, src/tree_comparer.cpp:307, which this is the per-tree sibling of), in double, one addition per
 *     node.  (The reference rounds heights to float and sums nothing over a sequence: the definition is the contract.)
 *   S(i,j) = sum over the trees, in the order given, of w_t * v_t(i,j); S symmetric, its diagonal 0; W = sum of w_t;
 *   the mean matrix is S / W.  SIZE: S is uint64, exact.  TIME: S is double, per element and tree
 *   S = S + (double)w_t * v_t, the product rounded, then the sum (no fused multiply-add), trees strictly in order.
 *   The host and the device return equal bits for both metrics.
 *   rl_pairwise_trees: parents [ntrees][2N-1]; branch_length [ntrees][2N-1] (of the branch above each node; required
 *     for TIME, ignored for SIZE); weights [ntrees], >= 0; sum_out: N*N uint64 (SIZE) or double (TIME), row-major;
 *     *total_weight = W.  device >= 0: on that GPU (relate_amd/csrc/pairwise_kernels.hip, 2 <= N <= 10240, S kept on
 *     the device while the trees go up in batches; RL_ENODEVICE without one); device < 0: the host implementation
 *     (pairwise.cpp), one thread, any N >= 2.
 *   rl_pairwise_anc: the trees of .anc files, files in the order given and one in memory at a time.  w_t = the SNPs
 *     the tree covers, by the rule of rl_compare_anc: from its position to the next tree's, the last tree of a file
 *     up to and including the largest SNP_end of its nodes.  All files must hold the same N (else RL_EINVAL); a file
 *     with sample ages is RL_EINVAL for TIME (its leaves are not at height 0), fine for SIZE.  *N_out = N; with
 *     sum_out NULL nothing else happens (N from the first file's header: what the caller sizes sum_out by). */
enum { RL_PAIRWISE_SIZE = 0, RL_PAIRWISE_TIME = 1 };
int rl_pairwise_trees(const int *parents, const double *branch_length_or_null, const long long *weights, int N,
                      int ntrees, int metric, int device, void *sum_out, long long *total_weight);
int rl_pairwise_anc(const char *const *anc_paths, int npaths, int metric, int device, void *sum_out_or_null,
                    long long *total_weight, int *N_out);

/* --------------------------------------------------------- CopyingMatrix */
/* The Li-Stephens coancestry ("chunk length") matrix of a painted chunk: C[n][j] = the number of SNPs recipient n is
 * expected to copy from donor j, from the posterior rows RePaintSection leaves (rl_window_get_topology).  No reference
 * counterpart in the pipeline (it is the chunk-length matrix of ChromoPainter / fineSTRUCTURE); the definition is the
 * contract, and the host and the device return equal bits.
 *   Window w owns the SNPs wb[w] <= s < wb[w+1].  Target n has D rows top[p][0..N-1] there (floats, top[p][n] == 0) at
 *   the sites site[0] = boundarySNP_begin, the SNPs in between at which n is derived, site[D-1] = boundarySNP_end.
 *   1. Row weights, doubles, s rising: p = the largest index with site[p] <= s.  s == site[p]: Wt[p] += 1.  Else with
 *      a = rpos[site[p]], b = rpos[site[p+1]]: a == b: wl = wr = 0.5 (src/anc_builder.cpp:146-153), else
 *      wl = (b - rpos[s]) / (b - a), wr = (rpos[s] - a) / (b - a); Wt[p] += wl, Wt[p+1] += wr: GetMatrix's
 *      interpolation between a target's neighbouring rows (src/anc_builder.cpp:130-168), on normalised rows.
 *   2. Z_p = the sum of (double)top[p][j]: 256 partial sums, partial t over j = t, t + 256, ... rising, then halved,
 *      x[t] += x[t + h] for t < h, h = 128, 64, .. 1.  A row with Wt[p] != 0 whose Z_p is not finite and positive is
 *      RL_ESTATE with a message naming window, target and row.
 *   3. c_p = Wt[p] / Z_p; C[n][j] = C[n][j] + c_p * (double)top[p][j], the product rounded, then the sum (no fused
 *      multiply-add); p rising within a window, the windows rising; rows with Wt[p] == 0 are skipped.
 *   C: doubles, row = recipient, column = donor, zero diagonal; W = the SNPs covered; every row of C sums to W up to
 *   rounding, C / W are the copying shares.
 *   rl_window_copying: adds one window into a DEVICE buffer of (targets of the context) * N doubles
 *     (relate_amd/csrc/copying_kernels.hip).  A bounded window (rl_window_open_bounded) is reduced part by part,
 *     RePaintSection run again as for its matrices, every row once: the bits of the unbounded window.  Afterwards its
 *     resident rows are the window's last part; its cursors are as before.  kernel_ms (optional): the reduce kernels.
 *   rl_window_copying_host: the same into a host buffer (copied to the device, added to, copied back).
 *   rl_copying_matrix: windows w_first .. w_last of a painted context (rl_paint; rl_set_window_range must cover them),
 *     opened, reduced and closed one after another, each with the posterior rows the free HBM has room for.  C_host:
 *     (targets of the context) * N doubles, overwritten; *W = wb[w_last+1] - wb[w_first].
 *   rl_copying_weights_host / rl_copying_rows_host (no GPU): step 1 for one target and window (site[D] rising, the
 *     window's SNPs [s_begin, s_end)), and steps 2 and 3 on the host for rows [D][N], added to c_row[N]: the twin the
 *     device is held to.
 *   rl_stage_copying_matrix: loads the chunk, paints the windows of [first_section, min(last_section, W-1)]
 *     (rl_set_window_range), reduces them and writes out_path: int32 N, int32 chunk, int32 first_snp, int32 end_snp,
 *     int64 W, then N*N doubles. */
int rl_window_copying(rl_window *win, void *d_C, float *kernel_ms);
int rl_window_copying_host(rl_window *win, double *C_host, float *kernel_ms);
int rl_copying_matrix(rl_ctx *ctx, int w_first, int w_last, int sum_mode, double *C_host, long long *W);
int rl_copying_weights_host(const int *site, int D, const double *rpos, int s_begin, int s_end, double *weights);
int rl_copying_rows_host(const float *rows, const double *weights, int D, int N, double *c_row);
int rl_stage_copying_matrix(const char *out_dir, int chunk_index, int first_section, int last_section,
                            const rl_stage_opts *opts, const char *out_path);

/* ------------------------------------------------ CoalescentRateForSection */
/* Epoch-binned pairwise coalescence counts and opportunities of a dated tree sequence, and the rates they give: the
 * reference's `RelateCoalescentRate --mode CoalescentRateForSection` and `--mode FinalizePopulationSize`
 * (include/evaluate/coalescent_rate/), whose .bin and .coal files these entries reproduce byte for byte.
 *   Epochs ep[0..E-1]: floats, ep[0] = 0, rising; 2 <= E <= 64.  Trees as CompareTopology takes them (2N-1 parents,
 *   binary, parent[v] > v, node 2N-2 the root); branch lengths >= 0 and finite; anything else is RL_EINVAL with a
 *   message naming the tree and the node.
 *   Per tree with the float `factor`: t(leaf) = 0, t(m) = (float)((double)t(c) + branch_length[c]), c the first child
 *   of m in node order -- a float at every node (GetCoalescentRate, CoalescentRateForSection.cpp:17-89).  For i < j
 *   with t = t(MRCA(i,j)) and e = 0 .. E-2 in turn: if t < ep[e+1]: D[e][i][j] += factor,
 *   D[e][j][i] += factor * (t - ep[e]), stop; else D[e][j][i] += factor * (ep[e+1] - ep[e]).  Float arithmetic, the
 *   product rounded before the sum; plane E-1 and the diagonals stay 0.  One addition per element and tree, the trees
 *   in order: the host and the device return the reference's bits.
 *   rl_coalrate_epochs (replaces :296-380): the default 31 epochs of years_per_gen (the reference's default: 28), or
 *     those of `--bins lower,upper,step`.  *nepochs: on entry the room in epochs, on return the count (RL_EINVAL if it
 *     does not fit, the count still set).
 *   rl_coalrate_trees (replaces :17-89 and the loop body :475-479): parents, branch_length [ntrees][2N-1], factors
 *     [ntrees] (any finite value), out [E][N][N] floats, overwritten.  device >= 0: on that GPU
 *     (relate_amd/csrc/coalrate_kernels.hip; 2 <= N <= 10240, D kept on the device -- 4 E N^2 bytes, RL_ENOMEM if the
 *     device has not that much free -- while the trees go up in batches of rl_coalrate_batch_trees(N); RL_ENODEVICE
 *     without one); device < 0: the host implementation (coalrate.cpp), one thread, any N >= 2.
 *   rl_coalrate_anc (replaces :265-294, :441-481 and AncMutIterators, src/mutations.cpp:713-774, :854-912): the trees
 *     of a TEXT .anc, one in memory at a time, each with the factor of NextTree from the .mut -- half the dist before
 *     its first SNP, plus its SNPs' dists, minus half the last; 0 for a tree without SNPs -- and, as the reference's
 *     loop runs once more after NextTree has returned -1, the last tree again with the factor -1.  *N_out = N; with
 *     out NULL nothing else happens.  RL_EINVAL: sample ages in the header, .gz inputs, tree indices that fall in the
 *     .mut.  (--mask and --dist are refused by the CLI.)
 *   rl_coalrate_write_bin / rl_coalrate_read_bin (replace :565-583 and FinalizePopulationSize.cpp:43-53): int32 E,
 *     E floats, then E times CollapsedMatrix<float>::DumpToFile (src/collapsed_matrix.hpp:204-213): two 64-bit words
 *     N, N and N*N floats.  read_bin with data NULL (and epochs NULL or room for *nepochs of the first call) returns
 *     E and N alone.
 *   rl_coalrate_finalize (replaces FinalizePopulationSize.cpp:57-91, :191-235): over i < j in that order, float sums
 *     of D[e][i][j] (num) and D[e][j][i] (denom) per (group pair, epoch e < E-1); rates [g][g][E] = num / denom of the
 *     unordered group pair, a float division (0 / 0 in the last epoch and for a pair of groups without pairs).
 *     group_of_haplotype NULL: one group (ngroups = 1).
 *   rl_coalrate_finalize_files (replaces FinalizePopulationSize.cpp:13-136, :138-291 and Sample::Read,
 *     src/sample.cpp:4-110): bin_path -> coal_path as the reference writes it with operator<<; poplabels: the second
 *     column is the group, two haplotypes per line unless a fourth column is `1`; `hap` is RL_EINVAL. */
int rl_coalrate_batch_trees(int N);
int rl_coalrate_epochs(float years_per_gen, const char *bins_or_null, float *epochs, int *nepochs);
int rl_coalrate_trees(const int *parents, const double *branch_length, const float *factors, int N, int ntrees,
                      const float *epochs, int nepochs, int device, float *out);
int rl_coalrate_anc(const char *anc_path, const char *mut_path, const float *epochs, int nepochs, int device,
                    float *out_or_null, int *N_out);
int rl_coalrate_write_bin(const char *path, const float *epochs, int nepochs, const float *data, int N);
int rl_coalrate_read_bin(const char *path, float *epochs_or_null, int *nepochs, float *data_or_null, int *N);
int rl_coalrate_finalize(const float *data, int N, int nepochs, const int *group_of_haplotype_or_null, int ngroups,
                         double *rates);
int rl_coalrate_finalize_files(const char *bin_path, const char *poplabels_or_null, const char *coal_path);

/* ------------------------------------------------------------------ Frequency and Selection
 * The two modes of the reference's RelateSelection that DetectSelection.sh runs
 * (include/evaluate/selection/RelateSelection.cpp): allele frequency through time, and its p-values.
 *
 * Frequency.  Node times are those of Tree::GetCoordinates (src/anc.cpp:525-537): t(leaf) = 0, t(m) =
 * (float)max((double)t(c2) + bl[c2], (double)t(c1) + bl[c1]).  The boundaries are rl_coalrate_epochs' (the reference's
 * :381-464 yields the same floats).  A SNP on branch b of its tree, b neither -1 nor the root, has a row: with T the
 * internal nodes of the tree and S those in the subtree of b (b included if internal), for every boundary e, from the
 * oldest to 0,
 *   lineages (.lin)  = 0 if t(root) < e, else 1 + |{u in T : t(u) > e}|
 *   carriers (.freq) = 0 if t(root) < e or t(parent(b)) <= e, else 1 + |{u in S : t(u) > e}|
 * and, with DAF the leaves below b and h = (DAF + 1) / 2: when_DAF_is_half = -1 if h <= 1, else 1 + |{u in T : t(u) >=
 * x}| with x the (h-1)-th largest time in S; when_mutation_has_freq2 = -1 if b is a leaf, else 1 + |{u in T : t(u) >=
 * t(b)}|; TreeFreq = 0.  That closed form equals the reference's walk (:556-788) on trees in which no two internal
 * nodes have equal float times and none has a time <= 0; on every other tree the rows are those of the walk itself,
 * restated on the host (relate_amd/csrc/frequency.cpp), whose live asserts are RL_EINVAL naming the tree and the SNP.
 *   rl_frequency_trees (replaces :510-516, :541-547, :556-788): parents, branch_length [ntrees][2N-1]; nsnps SNPs with
 *     snp_tree (rising, in [0, ntrees)) and snp_branch (in [-1, 2N-2]); freq [nsnps][E+1]: the carriers per boundary,
 *     then TreeFreq; lin [nsnps][E+2]: the lineages per boundary, when_DAF_is_half, when_mutation_has_freq2; marks
 *     [nsnps]: 1 where the row is there, 0 where the branch is -1 or the root (the row is untouched); root_time
 *     [ntrees]; *host_trees: trees with a marked SNP whose rows came from the host walk.  device >= 0: on that GPU
 *     (relate_amd/csrc/frequency_kernels.hip; 2 <= N <= 10240, the trees go up in batches of
 *     rl_frequency_batch_trees(N), trees with tied or non-positive times come back for the host walk; RL_ENODEVICE
 *     without one); device < 0: the host walk for every tree, one thread, any N >= 2.  2 <= E <= 64.
 *   rl_frequency_anc (replaces :354-363, :467-814 and AncMutIterators::FirstSNP / NextSNP, src/mutations.cpp:933-1009):
 *     the trees of a TEXT .anc that have SNPs in the .mut; a SNP is written iff it has exactly one branch, is not
 *     flipped, age_begin <= t(root) and the branch is neither -1 nor the root (:539-554).  Writes freq_path and
 *     lin_path as the reference does (`pos rs_id`, every count followed by a space; .freq ends ` TreeFreq DataFreq`
 *     behind a second space, DataFreq 0).  *rows: rows written; *host_trees as above (either may be NULL).
 *     RL_EINVAL: sample ages in the header, .gz inputs, a .mut with population-frequency columns, tree indices that
 *     fall.  (--first_snp / --last_snp of the reference are not offered.)
 * Selection, on the host (its bytes are libm's):
 *   rl_selection_logp (replaces log_pvalue, :136-178): log10 of P(at least fN of N lineages carry | fk of k did), in
 *     the reference's float / double arithmetic; 1 if fk < 2 or k == -1.  The reference's asserts (fN < N, fk < k,
 *     fN > 0) and an index outside its table of log(k!) are RL_EINVAL.
 *   rl_selection_files (replaces :190-328): in_prefix.freq + in_prefix.lin (this library's or the reference's) ->
 *     out_path, the reference's .sele: the .lin's header, then per row `pos rs_id`, a cell per boundary and the two
 *     trailing cells (fk = (int)((fN + 1) / 2) at when_DAF_is_half, fk = 2 at when_mutation_has_freq2), all `1` for a
 *     row with fN <= 2; written with the precision of operator<<.  Rows in parallel on RELATE_AMD_THREADS threads. */
int rl_frequency_batch_trees(int N);
int rl_frequency_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_tree,
                       const int *snp_branch, int nsnps, const float *epochs, int nepochs, int device, int *freq, int *lin,
                       unsigned char *marks, float *root_time, int *host_trees);
int rl_frequency_anc(const char *anc_path, const char *mut_path, const float *epochs, int nepochs, int device,
                     const char *freq_path, const char *lin_path, long long *rows, int *host_trees);
int rl_selection_logp(int k, float fk, int N, float fN, float *logp);
int rl_selection_files(const char *in_prefix, const char *out_path);

/* ------------------------------------------------------------------ AvgMutationRate
 * The reference's `RelateMutationRate --mode Avg` (include/evaluate/mutation_rate/AvgMutationRate.cpp), the step of
 * EstimatePopulationSize.sh whose _avg.rate file is the --mrate input of the next branch-length pass.
 *
 * The epoch boundaries are DOUBLES here (:373-456): `log_10` and years_per_gen are floats inside double expressions.
 * Node times are those of Tree::GetCoordinates (src/anc.cpp:525-537), a float at every node, as for Frequency.
 *
 * Branch length of a tree per epoch (GetCoordsAndLineages :19-95, GetBranchLengthsInEpoch :228-291).  With t_1 <= ...
 * <= t_{N-1} the sorted times of the internal nodes and t_0 = 0, the interval (t_{k-1}, t_k] carries n = N - (k-1)
 * lineages -- leaves sort before internal nodes at time 0, so this holds with tied times and with internal nodes at
 * 0; an empty interval adds nothing.  A cursor walks the epochs, from epoch 0, over the intervals (a, b] in order:
 *   b <  ep[c+1]:  out[c] += (double)((float)n * (b - a))                     a float product of a float difference
 *   b >= ep[c+1]:  out[c] += (double)n * (ep[c+1] - (double)a); c++;
 *                  while ep[c+1] < b: out[c] = (double)n * (ep[c+1] - ep[c]); c++   whole epochs, assigned
 *                  out[c] = (double)n * ((double)b - ep[c])                    (b == ep[c+1] leaves the cursor at c)
 * and the walk ends for good once c == E-1: what lies above the last boundary is dropped and out[E-1] stays 0 (the
 * reference shrinks its vector to E-1 entries and its caller reads E).  So a time exactly on a boundary decides
 * whether the next interval is added as a float product or assigned as a double one; both sides restate that.
 *
 * Per SNP with exactly one branch, in the .mut's order, flipped or not (:519-586): the mutation is spread over the
 * epochs that [age_begin, age_end] spans, in proportion; opportunity[e] += out_of_its_tree[e] * count_bases[s], with
 * count_bases[s] = 0.5*dist[j-1]/1e9 + 0.5*dist[j]/1e9, j the SNP's index in the position list (0.5*dist[0]/1e9 alone
 * for j = 0; :458-494).  Both are serial double sums on the host.  rate[e] = (mutation[e] / opportunity[e]) / 1e9.
 *   rl_mutrate_epochs (replaces :373-456): the default 31 boundaries, or those of --bins lower,upper,step.
 *     *nepochs: room on entry, the count on return.
 *   rl_mutrate_trees (replaces :58-95 and :228-291): parents, branch_length [ntrees][2N-1]; out [ntrees][E] doubles,
 *     entry E-1 equal to 0.  device >= 0: on that GPU (relate_amd/csrc/mutrate_kernels.hip; 2 <= N <= 10240, 2 <= E
 *     <= 64, the trees go up in batches of rl_mutrate_batch_trees(N); every tree is answered there, none comes back;
 *     RL_ENODEVICE without one -- there is no fallback); device < 0: the reference's walk restated on one host thread
 *     (relate_amd/csrc/mutrate.cpp), same limits.  RL_EINVAL names the tree: a parent that is not above its child, a
 *     branch length that is negative or not finite; epochs[0] must be 0 and the boundaries rise.
 *   rl_mutrate_anc (replaces :296-590 and AncMutIterators::FirstSNP / NextSNP): the trees of a TEXT .anc that have a
 *     one-branch SNP in the .mut.  dist_path_or_null: the --dist file (one header line, then `pos dist`; it may hold
 *     more positions than the .mut); NULL: the .mut's own pos and dist columns.  mutation [E], opportunity [E];
 *     *mapped_snps (may be NULL): SNPs with one branch.  RL_EINVAL: sample ages in the header, .gz inputs (the dist
 *     file included), tree indices that fall, a .mut position that the dist file does not hold (the reference reads
 *     past the end), naming the SNP.
 *   rl_mutrate_write (replaces :967-991): `epoch rate` per line with the precision of operator<<; the last epoch's
 *     opportunity is 0 and its rate prints as the division leaves it (`-nan`, or `inf`).
 * Multi-chromosome inputs (--chr, --first_chr, --last_chr), MutationDensity and the per-category modes are not
 * offered. */
int rl_mutrate_batch_trees(int N);
int rl_mutrate_epochs(float years_per_gen, const char *bins_or_null, double *epochs, int *nepochs);
int rl_mutrate_trees(const int *parents, const double *branch_length, int N, int ntrees, const double *epochs,
                     int nepochs, int device, double *out);
int rl_mutrate_anc(const char *anc_path, const char *mut_path, const char *dist_path_or_null, const double *epochs,
                   int nepochs, int device, double *mutation, double *opportunity, long long *mapped_snps);
int rl_mutrate_write(const char *path, const double *epochs, int nepochs, const double *mutation,
                     const double *opportunity);

/* ------------------------------------------------------------------ MutationRateWithContext / FinalizeMutationRate
 * The reference's `RelateMutationRate --mode WithContextForChromosome` and `--mode Finalize` (include/evaluate/
 * mutation_rate/RelateMutationRate.cpp): the mutation rate through time of the 96 trinucleotide categories.  The
 * epochs are those of rl_mutrate_epochs (:661-744 is the text of AvgMutationRate.cpp:373-456; its `age` is 0), the
 * branch length of a tree per epoch that of rl_mutrate_trees.
 *
 * Categories (:746-794): 192 keys `upstream downstream ancestral derived` over ACGT map onto 96 indices, 6 * (4 * up +
 * down) + {C>A, C>G, C>T, A>T, A>G, A>C}, a key and its reverse complement onto the same index.
 *
 * Bases per SNP and category (CountBasesByType, :40-260): the ancestor FASTA (first line skipped, case kept) and the
 * mask FASTA (upper-cased) are padded with N to the longer one; one pass moves a base p along them with a count d of
 * non-P mask characters in a window around p.  p starts at min(1001, position of the first SNP) with the window [0,
 * 1000 + p]; while the window's right end is inside (main phase, threshold 2000) both ends move, afterwards (tail
 * phase, threshold 1000) only the left one.  Base p counts for the current SNP s -- +1 on the three categories
 * (flanks, ancestral -> each other base) -- when it lies between the midpoints to the neighbours of the current
 * position pos[j] of the position list (the midpoint in front of pos[0] is 0.5 * pos[0]), its mask is P, d is within
 * the threshold, SNP s has exactly one branch and the three ancestor bases are nucleotides in either case.  s advances
 * when p reaches the midpoint behind pos[j], j while pos[j] is below SNP s's position.  Both phases end at the LAST
 * SNP, whose row stays zero.
 *
 * Per SNP in the .mut's order (:829-908).  It qualifies with exactly one branch, both flanks not `NA`, alleles `X/Y`
 * of three characters with X != Y both in ACGT; ind = table[upstream + downstream + X + Y], 0 for a key the table
 * lacks.  age_end = min(age_end, the float time of its tree's root); the SNP is spread over the epochs [age_begin,
 * age_end] spans as for AvgMutationRate, onto mutation[e][ind]; and for every epoch e and category c
 *     opportunity[e][c] += length_of_its_tree[e] * (double)count[s][c]      a double product, then a double sum,
 * one serial chain per cell through the qualifying SNPs.
 *   rl_mutctx_category_names (replaces :397-410): the 96 names, '\n' after each, in index order; *bytes: room on
 *     entry, the bytes needed (with the final 0) on return.  rl_mutctx_category: the index of a 4-letter key, -1 for
 *     one the table lacks.
 *   rl_mutctx_count_bases (replaces :40-260): pos [npos] the position list, snp_pos and one_branch [nsnps] the .mut's;
 *     counts [nsnps][96] uint32.  RL_EINVAL names the SNP where the reference reads outside its sequences (a mask
 *     that ends inside the first window, a counted base 0) or past the end of its position list.
 *   rl_mutctx_trees (replaces :888-893 over :821-838): parents, branch_length [ntrees][2N-1]; the qualifying SNPs as
 *     snp_tree [nsnps] (not falling) and snp_counts [nsnps][96]; opportunity [E][96]; root_time_or_null [ntrees];
 *     seconds_or_null [3]: on the device, the seconds of the tree arrays and the per-tree kernel | of the SNP copies |
 *     of the chains kernel.  device >= 0: relate_amd/csrc/mutctx_kernels.hip, in batches of rl_mutrate_batch_trees(N)
 *     trees, 2 <= N <= 10240, 2 <= E <= 64, RL_ENODEVICE without one; device < 0: the reference's loop on one host
 *     thread, the same bits.  RL_EINVAL names a tree as rl_mutrate_trees does; nothing of its batch is added.
 *   rl_mutctx_anc (replaces :578-908): a TEXT .anc and its .mut, the mask, the ancestor, the --dist file or NULL;
 *     mutation, opportunity [E][96]; snps3 (may be NULL): SNPs read, with one branch, qualifying.  RL_EINVAL: sample
 *     ages, .gz inputs, an age_end that is not below the last boundary (the reference's assert :869).
 *   rl_mutctx_write / rl_mutctx_read (replace :916-932, :365-382): prefix_mut.bin (int E, E doubles, u64 E, u64 96,
 *     E*96 doubles) and prefix_opp.bin (the matrix alone).  *nepochs: room on entry, the count on return.
 *   rl_mutctx_sum (replaces :445-576): prefix_chr<c>_{mut,opp}.bin of the chromosomes ('\n' separated) added in order
 *     into out_prefix_{mut,opp}.bin; the per-chromosome files stay (the reference removes them).
 *   rl_mutctx_finalize (replaces :385-425): in_prefix_{mut,opp}.bin -> the .rate text: the 96 names, then per epoch but
 *     the last its start and mutation / opportunity per category as operator<< prints a double (0/0: `-nan`).
 * The ForCategory, ForPattern, XY and MutationDensity modes are not offered. */
int rl_mutctx_category_names(char *names, int *bytes);
int rl_mutctx_category(const char *key);
int rl_mutctx_count_bases(const char *ancestor_path, const char *mask_path, const int *pos, long long npos,
                          const int *snp_pos, const unsigned char *one_branch, long long nsnps, uint32_t *counts);
int rl_mutctx_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *snp_tree,
                    const uint32_t *snp_counts, long long nsnps, const double *epochs, int nepochs, int device,
                    double *opportunity, float *root_time_or_null, double *seconds_or_null);
int rl_mutctx_anc(const char *anc_path, const char *mut_path, const char *mask_path, const char *ancestor_path,
                  const char *dist_path_or_null, const double *epochs, int nepochs, int device, double *mutation,
                  double *opportunity, long long *snps3);
int rl_mutctx_write(const char *prefix, const double *epochs, int nepochs, const double *mutation,
                    const double *opportunity);
int rl_mutctx_read(const char *prefix, double *epochs, int *nepochs, double *mutation, double *opportunity);
int rl_mutctx_sum(const char *prefix, const char *chromosomes, const char *out_prefix);
int rl_mutctx_finalize(const char *in_prefix, const char *rate_path);

/* ------------------------------------------------------------------ CoalRateForTree
 * The reference's `RelateCoalescentRate --mode CoalRateForTree` (CoalescenceRateForTree, include/evaluate/
 * coalescent_rate/CoalescentRateForSection.cpp:605-858, and coal_tree::populate / coal_tree::Dump(const std::string&),
 * coal_tree.cpp), the step EstimatePopulationSize.sh runs in every iteration: dated trees in, the .coal file of the
 * next branch-length pass out.  The boundaries are the doubles of rl_mutrate_epochs (:630-713 is the text of
 * AvgMutationRate.cpp:373-456).  Node times are those of Tree::GetCoordinates, a float at every node.
 *
 * Per tree with `bases` the float of AncMutIterators::NextTree widened to double (coal_tree.cpp:98-199): all 2N-1
 * node times are sorted by (time, label); num_lins[r] is the lineage count after the group of equal times that holds
 * rank r.  Ranks 1 .. 2N-2 are walked with an epoch cursor c and lower = ep[0]:
 *   while coords[r] <= ep[c] (a float against a double):
 *     an internal node:  num[c-1] += bases / 1e9
 *     denom[c-1] += bases * n * (n-1) / 2.0 * (coords[r] - lower) / 1e9, n = num_lins[r-1];  lower = coords[r]
 *   otherwise: denom[c-1] += bases * n * (n-1) / 2.0 * (ep[c] - lower) / 1e9;  lower = ep[c];  c++
 * every operation in double, left to right; the walk ends at the root or with the boundaries, and entry E-1 of both
 * vectors stays 0.  The terms go straight onto the accumulators of the current block of block_size trees (1000 in
 * the reference): one serial sum per block and epoch through the block's trees in order, not a sum per tree.  There
 * are (int)(ntrees / (double)block_size + 1) blocks; the last may stay empty.
 * On the device (relate_amd/csrc/coaltree_kernels.hip) the terms come from the sorted times S of the internal nodes
 * alone -- node k lies in epoch j with ep[j] < S[k] <= ep[j+1], n = N - k, lower = max(S[k-1], ep[j]) -- in one
 * kernel, and a second adds them in the walk's order; the host twin (coaltree.cpp) is the walk itself.
 *   rl_coaltree_batch_trees: trees per upload of the device path at N leaves.
 *   rl_coaltree_num_blocks: the block count of a sequence (coal_tree.cpp:78); 0 for bad arguments.
 *   rl_coaltree_trees (replaces coal_tree.cpp:98-199): parents, branch_length [ntrees][2N-1], factors [ntrees] (the
 *     bases, finite and >= 0); num, denom [blocks][E] doubles.  *num_blocks: room in blocks on entry, the count on
 *     return.  block_size >= 1.  device >= 0: on that GPU (2 <= N <= 10240, 2 <= E <= 64; RL_ENODEVICE without
 *     one -- there is no fallback); device < 0: the walk on one host thread, same limits.  RL_EINVAL names the tree:
 *     a parent that is not above its child, a branch length or a factor that is negative or not finite; epochs[0]
 *     must be 0 and the boundaries rise.
 *   rl_coaltree_anc (replaces CoalescentRateForSection.cpp:748-770 and coal_tree.cpp:242-297): the trees of a TEXT
 *     .anc with the factors its .mut gives them as for rl_coalrate_anc, in blocks of 1000, until a factor is
 *     negative; num, denom [E]: the blocks added in order.  *ntrees (may be NULL): the trees taken.  RL_EINVAL:
 *     sample ages in the header, .gz inputs.
 *   rl_coaltree_rates (replaces coal_tree.cpp:309-319): rates[i] = num[i] / denom[i] where denom[i] != 0, otherwise
 *     the rate before it, or 0 at i = 0.
 *   rl_coaltree_write (replaces coal_tree.cpp:299-343): `0 `, the boundaries, `0 0 ` and the rates, three lines with
 *     the precision of operator<<.
 * Several chromosomes (--chr), --dist and the dead --coal input (is_coal_fail = true, :799) are not offered. */
int rl_coaltree_batch_trees(int N);
int rl_coaltree_num_blocks(long long ntrees, int block_size);
int rl_coaltree_trees(const int *parents, const double *branch_length, const float *factors, int N, int ntrees,
                      const double *epochs, int nepochs, int block_size, int device, double *num, double *denom,
                      int *num_blocks);
int rl_coaltree_anc(const char *anc_path, const char *mut_path, const double *epochs, int nepochs, int device,
                    double *num, double *denom, int *ntrees);
int rl_coaltree_rates(const double *num, const double *denom, int nepochs, double *rates);
int rl_coaltree_write(const char *path, const double *epochs, int nepochs, const double *rates);

/* ------------------------------------------------------------------ SubTreesForSubpopulation
 * The reference's `RelateExtract --mode SubTreesForSubpopulation` (include/extract/
 * CreateAncesTreeFileForSubpopulation.cpp), the step that opens EstimatePopulationSize.sh under --pop_of_interest: a
 * dated tree sequence in, the sequence of its subtrees for the haplotypes of some groups out, as a text .anc / .mut
 * and a .poplabels that the other modes read.
 *
 * Per tree (Tree::GetSubTree, src/anc.cpp:655-738) with the subset's M leaves in rising label order:
 * number_in_subpop[v] is the number of subset leaves below v.  Subset leaf k becomes node k; the internal nodes are
 * taken in rising label order: one both of whose children have subset leaves below them is KEPT, takes the next free
 * label M, M+1, ... and its own branch length; one with exactly one such child is contracted -- it converts to what
 * that child converts to, and its branch length is added (a double addition) onto that subtree node; any other node
 * converts to -1.  The ancestors above the topmost kept node end in the subtree root's branch length.  M = N is the
 * identity.  The times are those of Tree::GetCoordinates (:525-565) ON THE SUBTREE, a float at every node:
 * t(m) = (float)max((double)t(c2) + bl[c2], (double)t(c1) + bl[c1]), t(leaf) = 0.
 * On the device (relate_amd/csrc/subtrees_kernels.hip) a workgroup takes a tree: the counts are one pull scan, the
 * new labels an exclusive scan of the keep flags, and every subset leaf and kept node walks its own chain of
 * contracted ancestors; the host twin (subtrees.cpp) is the reference's loop.
 *   rl_subtrees_batch_trees: trees per upload of the device path at N leaves.
 *   rl_subtrees_trees (replaces src/anc.cpp:655-738 and :525-565): parents, branch_length [ntrees][2N-1]; subset [M]
 *     leaf labels, rising; out: sub_parent, sub_bl, sub_time [ntrees][2M-1], convert_index, number_in_subpop
 *     [ntrees][2N-1].  device >= 0: on that GPU (RL_ENODEVICE without one -- there is no fallback); device < 0: the
 *     reference's loop on one host thread.  2 <= N <= 10240, 2 <= M <= N on both.  RL_EINVAL names the tree: a
 *     parent that is not above its child, a branch length (the root's included) that is negative or not finite; a
 *     subset label out of range or not above the one before it.
 *   rl_subtrees_poplabels (replaces Sample::Read and Sample::AssignPopOfInterest, src/sample.cpp:4-171): the group of
 *     every haplotype (a diploid file counts every line twice, one with ploidy 1 once, a mix is RL_EINVAL), the group
 *     names sorted and joined with '\n', and, if pops is not NULL, a flag per group: named in pops (comma separated,
 *     duplicates ignored, `All`; an unknown name is RL_EINVAL).  *num_haplotypes, *num_groups, *names_bytes: room on
 *     entry, the counts on return; an array without room (or NULL) is not filled.
 *   rl_subtrees_files (replaces CreateAncesTreeFileForSubpopulation.cpp:17-401): a TEXT .anc and its .mut, a
 *     .poplabels and the groups of interest in; <out>.anc, <out>.mut and <out>.poplabels out, the reference's bytes:
 *     the SNPs with one branch that converts to a subtree node other than the root are kept (after the filter on
 *     the groups' frequency columns, if the .mut has them), a tree without a kept SNP is dropped, neighbouring
 *     subtrees are associated (FindEquivalentBranches at N = M) and num_events, SNP_begin and SNP_end carried along.
 *     RL_EINVAL: sample ages in the header, .gz inputs, a .poplabels whose haplotypes are not the .anc's, M < 2, a
 *     .mut whose tree indices fall, a tree without SNPs before the .mut's last tree (an assert of the reference).
 *   rl_subtrees_rewrite: a text .anc and .mut read with every column and written again (the readers and writers
 *     of the above; a file the reference wrote comes back byte for byte). */
typedef struct rl_subtrees_summary {
  int trees_read;  /* trees of the .anc the walk visited */
  int trees_kept;
  int snps_read;   /* lines of the .mut */
  int snps_kept;
  int M, N;
  int has_freq;    /* the .mut's first line carries frequency columns */
} rl_subtrees_summary;
int rl_subtrees_batch_trees(int N);
int rl_subtrees_trees(const int *parents, const double *branch_length, int N, int ntrees, const int *subset, int M,
                      int device, int *sub_parent, double *sub_bl, float *sub_time, int *convert_index,
                      int *number_in_subpop);
int rl_subtrees_poplabels(const char *poplabels_path, const char *pops_or_null, int *group_of_haplotype,
                          int *num_haplotypes, int *of_interest, int *num_groups, char *names, int *names_bytes);
int rl_subtrees_files(const char *anc_path, const char *mut_path, const char *poplabels_path, const char *pops,
                      const char *out_prefix, int device, rl_subtrees_summary *summary);
int rl_subtrees_rewrite(const char *anc_in, const char *mut_in, const char *anc_out, const char *mut_out);

/* ------------------------------------------------------------------ tools */
/* Synthetic block-coalescent panel (stand-in for MakeChunks input,
 * SURVEY.md 8d).  seq_chars (L*N) and/or bits (L*row_words) may be NULL. */
int rl_synth_panel(int N, int L, uint64_t seed, int block, int jitter,
                   uint8_t *seq_chars, uint32_t *bits, int row_words, int *bp,
                   double *r, double *rpos);
/* the reference's window rule (src/data.cpp:213-229); returns W (<0 on error) */
int rl_synth_windows(int N, int L, const uint8_t *seq_chars, double budget,
                     int *wb, int max_windows);
int rl_synth_windows_bits(int N, int L, const uint32_t *bits, int row_words,
                          double budget, int *wb, int max_windows);
/* chunk files as Data::MakeChunks writes them (src/data.cpp:261-298,485-516) */
int rl_write_chunk_files(const char *dir, int chunk, int N, int L,
                         const uint8_t *seq_chars, const int *bp,
                         const double *r, const double *rpos, const int *wb,
                         int W);

#ifdef __cplusplus
}
#endif
#endif
