// paint_kernels.hip -- K1: stepping-stone painting of all targets.
//
// Replaces FastPainting::PaintSteppingStones (fast_painting.cpp:18-618).
// The two directions are independent in this stage: by default ONE launch of
// 2N workgroups paints both (blocks 0 .. N-1 the backward passes, blocks
// N .. 2N-1 the forward passes; longest target first in each), so that the last
// round of workgroups of one direction does not leave the chip half empty while
// the other direction waits.  DIR = 0 / 1 launch one direction alone (profiling).
// The forward step body and row pipeline and the stones are paint_pass.h,
// shared with paint32_kernels.hip and repaint_kernels.hip; the backward pass
// keeps its own (DESIGN_NOTES.md 13).
#include <cstdlib>
#include <type_traits>
#include "paint_pass.h"
#include "launch.h"

#ifndef RL_MODE
#error "compile with -DRL_MODE=0 (lanes), 1 (exact, parallel), 2 (exact, literal serial)"
#endif
#ifndef RL_FIT
#define RL_FIT 0  // the variant of every tile this translation unit holds (below, launch_paint_variant)
#endif

namespace rl {

// experiment builds (-DRL_STATS): per-segment cycle counters of the forward step, lanes mode
#ifdef RL_STATS
#define RL_TICK(n) const unsigned long long tick##n = __builtin_readcyclecounter()
#define RL_TOCK(acc, a, b) acc += tick##b - tick##a
#else
#define RL_TICK(n) do { } while (0)
#define RL_TOCK(acc, a, b) do { } while (0)
#endif

// A tile as the kernels see it (launch.h tile_fit): S registers per lane, of which the first LIVE (S or S - 1) hold a
// donor in some lane -- every unrolled loop leaves the rest out, so a dead register costs neither instructions nor
// VGPRs; the last TAIL registers take the backward pass's per-lane validity masks (whole chunks of 4), and registers
// S - FTAIL .. LIVE - 1 the forward pass's validity compare.
// SEG: the pass is one segment of a segmented pass (paint_pass.h): it walks its share of the steps, takes the state
// over from the segment before it instead of running the prologue and leaves it to the next one.
template <int S, int FTAIL, int MODE, int WAVES, int LIVE, bool SEG = false>
RL_DEV void paint_forward(const PaintParams &p, int k, float *stage, WaveLink<WAVES> &lk, SegShared *sh = nullptr) {
  const int wv = lk.w;  // this wave of the target's workgroup (wave-uniform)
  PaintLane<S> pl;
  pl.init(p.lay, k, wv);
  const PaintConsts &c = p.c;
  const auto [Dk, st, cfp, nx] = plan_slice(p, k);
  const int D = forward_steps(k, Dk);  // (paint_device.h: ends at the range's last stone)

  double a[S];
  typedef RegTerm<S, LIVE> Term;
  double ssum, ls, cfac;
  int wa, next_stone, i0 = 1, i1 = D;
  if constexpr (SEG) {
    i0 = paint_segment_first(1, D, sh->nseg, sh->s);
    i1 = paint_segment_first(1, D, sh->nseg, sh->s + 1);
  }
  if (SEG && sh->s > 0) {
    seg_restore<S, LIVE, WAVES>(p, a, pl.lane, wv, sh->chain, ls, cfac, wa);
    next_stone = forward_stone_index(k, wa);
  } else {
  // ---- SNP 0 (fast_painting.cpp:207-253)
  for_each_chunk<S, 8>(site_row(p.masks, S, p.L, st[0], WAVES, wv), [&](int j0, const u64x8 &m) {
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
      if (j0 + jj >= LIVE) continue;
      double v = c.init0;
      masked_mov(v, m[jj], c.init1);
      if (j0 + jj >= S - FTAIL) masked_mov(v, ~pl.valid(j0 + jj), 0.0);
      a[j0 + jj] = v;
    }
  });
  set_slot<S, LIVE>(a, pl.jk, pl.kbit, 0.0);
  ssum = wave_sum<MODE, S, WAVES>(Term{a, 0.0, 0.0, p.stats}, local_sum<S>(Term{a}), lk);
  ls = 0.0;
  wa = 0, next_stone = forward_stone_index(k, 0);
  while (next_stone == 0) {
    write_forward_stone<S, LIVE>(wa, pl, wv, a, ls, stage);
    next_stone = forward_stone_index(k, wa);
  }
  cfac = cfp[0] * ssum;  // :260
  }

  ForwardRows<S, WAVES> pipe(st, D, i0);
  const double K1 = in_vgpr(c.K1);
  constexpr int CH = S % 16 == 0 ? 16 : 8;  // registers per chunk of masks
  typedef typename MaskChunk<CH>::type Chunk;
  MaskRow row = pipe.row(p, wv);
  Chunk first = load_masks<CH>(row, 0);
  unsigned long long seg1 = 0, seg2 = 0, seg3 = 0, seg4 = 0, seg5 = 0;
  (void)seg1; (void)seg2; (void)seg3; (void)seg4; (void)seg5;
  for (int i = i0; i < i1; i++) {
    RL_TICK(0);
    pipe.retire();
    RL_TICK(1);
    pipe.advance(p, i, pl.lane, wv);
    // requested here, used after the sum: the chunk loop's waits cover the latency
    const double nx_i = nx[i - 1], cf_i = cfp[i];
    set_slot<S, LIVE>(a, pl.jk, pl.kbit, -cfac);  // donor k: (-c) + c = +0.0
    RL_TICK(2);
    const double lsum = forward_update<S, FTAIL, CH, LIVE>(a, row, first, pl.len, cfac, K1);  // :288-295
    RL_TICK(3);
    row = pipe.row(p, wv);
    first = load_masks<CH>(row, 0);
    ssum = wave_sum<MODE, S, WAVES>(Term{a, 0.0, 0.0, p.stats}, lsum, lk);
    RL_TICK(4);
    ls += nx_i;  // :281-282
    cfac = ssum;
    if (cfac < c.lower || cfac > c.upper) {  // :334-347
#pragma unroll
      for (int j = 0; j < LIVE; j++) a[j] /= ssum;
      ls += log(ssum);
      cfac = 1.0;
    }
    cfac *= cf_i;  // :349-352
    RL_TICK(5);
    RL_TOCK(seg1, 0, 1); RL_TOCK(seg2, 1, 2); RL_TOCK(seg3, 2, 3); RL_TOCK(seg4, 3, 4); RL_TOCK(seg5, 4, 5);
    while (next_stone == i) {  // :354-374
      write_forward_stone<S, LIVE>(wa, pl, wv, a, ls, stage);
      next_stone = forward_stone_index(k, wa);
    }
  }
  pipe.retire();
  if constexpr (SEG) {
    if (sh->s + 1 < sh->nseg) seg_save<S, LIVE, WAVES>(a, pl.lane, wv, ls, cfac, wa, sh);
  }
#ifdef RL_STATS
  if (MODE != 0 && p.stats && pl.lane == 0 && wv == 0) {  // whole step | chunk loop | sum | rescale test + factor
    atomicAdd(&p.stats[16], seg1 + seg2 + seg3 + seg4 + seg5);
    atomicAdd(&p.stats[17], seg3); atomicAdd(&p.stats[18], seg4); atomicAdd(&p.stats[19], seg1 + seg2 + seg5);
  }
  if (MODE == 0 && p.stats && pl.lane == 0 && wv == 0) {  // wait for prefetch | loads + slot | chunk loop | sum | rescale test
    atomicAdd(&p.stats[0], (unsigned long long)(D - 1));
    atomicAdd(&p.stats[1], seg1); atomicAdd(&p.stats[2], seg2); atomicAdd(&p.stats[3], seg3);
    atomicAdd(&p.stats[4], seg4); atomicAdd(&p.stats[5], seg5);
  }
#endif
}

template <int S, int TAIL, int MODE, int WAVES, int LIVE, bool SEG = false>
RL_DEV void paint_backward(const PaintParams &p, int k, float *stage, WaveLink<WAVES> &lk, SegShared *sh = nullptr) {
  const int wv = lk.w;
  PaintLane<S> pl;
  pl.init(p.lay, k, wv);
  const PaintConsts &c = p.c;
  const auto [D, st, cfp, nx] = plan_slice(p, k);

  double b[S];
  // exact: the first KS weighted terms of a step go from the update loop to the sum through LDS (StashTerm,
  // exact_sum.h), in the wave's strip, which no stone uses during a step
  // ... and the last R stay in registers of their own from the update loop to the end of the sum
  constexpr int KS = MODE == 1 ? stash_terms(S) : 0, R = MODE == 1 ? reg_stash_terms(S) : 0;
  StashPtr sp = stash_of(stage);  // (not const: kept opaque in place, see the update loop)
  (void)sp;
  double xr[R > 0 ? R : 1];
  (void)xr;

  // the walk: j from j_first down to j_last (a segment: its share of the steps D - 2 .. backward_last, counted from
  // the top)
  int j_first = D - 2, j_last = 0;
  if constexpr (SEG) {
    j_last = backward_last(k);
    const int n = D - 1 - j_last;
    j_first = D - 2 - paint_segment_first(0, n, sh->nseg, sh->s);
    j_last = D - 1 - paint_segment_first(0, n, sh->nseg, sh->s + 1);
  }
  double ls, bsum, cfac;
  int we, next_stone;
  if (SEG && sh->s > 0) {
    seg_restore<S, LIVE, WAVES>(p, b, pl.lane, wv, sh->chain, ls, cfac, we);
    next_stone = backward_stone_index(k, we);
  } else {
  // ---- last SNP (:396-448)
  ls = c.log_Nm1 - D * c.log_ntheta;  // normalizing_constant :399
#pragma unroll
  for (int i = 0; i < LIVE; i++) {
    double v = 1.0;
    if (i >= S - TAIL) masked_mov(v, ~pl.valid(i), 0.0);
    b[i] = v;
  }
  set_slot<S, LIVE>(b, pl.jk, pl.kbit, 0.0);  // written as beta[k] = 1 below, +0.0 from then on
  bsum = p.binit[k];  // serial sum of theta/ntheta minus ntheta (:421-431)
  we = p.W - 1, next_stone = backward_stone_index(k, we);
  while (next_stone == D - 1) {
    write_backward_stone<S, LIVE>(we, pl, wv, b, ls, 1.0f, stage);  // beta[k] = 1 at the last SNP
    next_stone = backward_stone_index(k, we);
  }
  cfac = cfp[D - 1] * bsum;  // :454-455
  }

  // row pipeline as in paint_forward: step j reads the rows of s0 (site j+1)
  // and s1 (site j); the row of s2 (site j-1) goes to L2 during the step
  int s0 = st[D - 1], s1 = D > 1 ? st[D - 2] : 0, s2 = D > 2 ? st[D - 3] : 0;
  if constexpr (SEG) s0 = st[j_first + 1], s1 = j_first >= 0 ? st[j_first] : 0, s2 = j_first >= 1 ? st[j_first - 1] : 0;
  uint32_t touched = 0;
  MaskRow rown = site_row(p.masks, S, p.L, s0, WAVES, wv);  // the later site's mismatches drive the update (:481-488)
  MaskRow rowh = site_row(p.masks, S, p.L, s1, WAVES, wv);
  u64x4 firstn = load_masks<4>(rown, 0), firsth = load_masks<4>(rowh, 0);
  const double K1 = in_vgpr(c.K1), theta = in_vgpr(c.theta), ntheta = in_vgpr(c.ntheta);
  unsigned long long bseg1 = 0, bseg2 = 0, bseg3 = 0, bseg4 = 0;
  (void)bseg1; (void)bseg2; (void)bseg3; (void)bseg4;
  typedef typename std::conditional<MODE == 1, StashTerm<S, LIVE>, MaskTerm<S, LIVE>>::type BackwardTerm;
  const auto make_term = [&](MaskRow row) {
    unsigned long long *const stats = p.stats ? p.stats + 8 : nullptr;
    if constexpr (MODE == 1)
      return BackwardTerm{row, b, theta, ntheta, stats, sp, xr};
    else
      return BackwardTerm{row, b, theta, ntheta, stats};
  };
  if constexpr (!SEG) j_last = backward_last(k);  // (paint_device.h: D and ls above keep the whole pass, the walk ends at the range's first stone)
  for (int j = j_first; j >= j_last; j--) {
    retire_touch(touched);
    if (j > 0) touched = touch_row(p.masks, S, s2, pl.lane, WAVES, wv);
    s0 = s1;
    s1 = s2;
    if (j > 1) s2 = st[j - 2];
    RL_TICK(0);
    const double nx_j = nx[j + 1], cf_j = cfp[j];  // used after the sum (see paint_forward)
    const double b1 = div_by_const(cfac, ntheta, c.inv_ntheta);     // cfac / ntheta, :474
    const double bt = div_by_const(cfac, theta, c.inv_theta) - b1;  // cfac / theta - b1, :475
    set_slot<S, LIVE>(b, pl.jk, pl.kbit, -b1);   // donor k: (-b1) + b1 = +0.0 (never a mismatch with itself)
    double lsum = 0.0;
    MaskRow vrow = (MaskRow)(p.masks + ((size_t)(p.L + 1) * WAVES + wv) * S);
    asm volatile("" : "+s"(vrow));
    RL_TICK(1);
    double xp[4] = {0.0, 0.0, 0.0, 0.0};  // exact: the previous chunk's terms on their way to the stash
    for_each_chunk2_tail<S, 4, TAIL>(rown, rowh, vrow, firstn, firsth,
                                     [&](int j0, const u64x4 &mn, const u64x4 &mh, const u64x4 &va) {
      double v[4], x[4];
      // Stored a chunk late, behind the loop's wait for this chunk's masks and the request of the next: an LDS write
      // counts on lgkmcnt like the mask loads, and issued at the end of its own chunk it would be waited for at once.
      if (KS > 0 && j0 > 0 && j0 - 4 < KS) {
        asm volatile("" : "+v"(sp));  // (pins the store behind the wait)
        stash_put4(sp, j0 / 4 - 1, xp);
      }
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
        if (j0 + jj < LIVE) v[jj] = b[j0 + jj];
      if (j0 + 4 <= S - TAIL)
        backward4(v, x, mn, mh, bt, b1, K1, theta, ntheta);
      else if (j0 + 4 <= LIVE)
        backward4_tail(v, x, mn, mh, va, bt, b1, K1, theta, ntheta);
      else  // (TAIL >= 4: the chunk of the dead register is a tail chunk)
        backward3_tail(v, x, mn, mh, va, bt, b1, K1, theta, ntheta);
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        if (j0 + jj >= LIVE) continue;
        b[j0 + jj] = v[jj];
        lsum += x[jj];  // the lane's share of :495-503
        if (KS > 0 && j0 < KS) xp[jj] = x[jj];
        hold_term<S, R>(xr, j0 + jj, x[jj]);
      }
    });
    if (KS == S) {
      if (LIVE == S)
        stash_put4(sp, S / 4 - 1, xp);
      else
        stash_put3(sp, S / 4 - 1, xp);
    }
    RL_TICK(2);
    const BackwardTerm term = make_term(rowh);
    rown = rowh;
    rowh = site_row(p.masks, S, p.L, s1, WAVES, wv);
    if (MODE == 0) {  // lanes: the sum reads no masks, request the next step's first chunks across it
      firstn = load_masks<4>(rown, 0);
      firsth = load_masks<4>(rowh, 0);
    }
    bsum = wave_sum<MODE, S, WAVES>(term, lsum, lk);  // :495-503
    if (MODE != 0) {
      firstn = load_masks<4>(rown, 0);
      firsth = load_masks<4>(rowh, 0);
    }
    RL_TICK(3);
    ls += nx_j;  // :471-472
    cfac = bsum;
    if (cfac < c.lower || cfac > c.upper) {  // :538-551
#pragma unroll
      for (int i = 0; i < LIVE; i++) b[i] /= bsum;
      ls += fast_log_dev((float)bsum);
      cfac = 1.0;
    }
    cfac *= cf_j;  // :553-556
    RL_TICK(4);
    RL_TOCK(bseg1, 0, 1); RL_TOCK(bseg2, 1, 2); RL_TOCK(bseg3, 2, 3); RL_TOCK(bseg4, 3, 4);
    while (next_stone == j) {  // :559-578
      write_backward_stone<S, LIVE>(we, pl, wv, b, ls, 0.0f, stage);
      next_stone = backward_stone_index(k, we);
    }
  }
  retire_touch(touched);
  if constexpr (SEG) {
    if (sh->s + 1 < sh->nseg) seg_save<S, LIVE, WAVES>(b, pl.lane, wv, ls, cfac, we, sh);
  }
#ifdef RL_STATS
  if (p.stats && pl.lane == 0 && wv == 0) {  // whole step | divisions + slot + loads | chunk loop | sum | rescale test + factor
    atomicAdd(&p.stats[20], bseg1 + bseg2 + bseg3 + bseg4);
    atomicAdd(&p.stats[21], bseg1); atomicAdd(&p.stats[22], bseg2); atomicAdd(&p.stats[23], bseg3);
    atomicAdd(&p.stats[24], bseg4);
  }
#endif
}

// S <= 80: hold the kernel to 256 registers so that two waves share a SIMD.
// WAVES = 2: a workgroup of two waves paints one target (N > 5120).
// SEGMENTED (DIR = 2 only): a workgroup is one segment of one pass, drawn by ticket (paint_pass.h seg_draw).
template <int S, int TAIL, int MODE, int WAVES, int DIR, int LIVE = S, int FTAIL = TAIL, bool SEGMENTED = false>
__global__ void __launch_bounds__(64 * WAVES, 2) paint_kernel(const PaintParams p) {
  // per wave: the staging strip of the stones (4 KB) and, where an exact backward pass runs, its stash of weighted
  // terms (up to 18 KB) in the same storage -- a stone is never written during a sum
  constexpr int STASH = (MODE == 1 && DIR != 0) ? stash_bytes(S) : 0;
  constexpr int WAVE_FLOATS = STASH > 16 * 64 * 4 ? STASH / 4 : 16 * 64;
  __shared__ __attribute__((aligned(16))) float stage[WAVES][WAVE_FLOATS];
  __shared__ WaveLinkStorage link;
  WaveLink<WAVES> lk = make_wave_link<WAVES>(&link);
#ifdef RL_STATS
  // experiment builds: when the workgroup was resident (tools/paint_timeline.py); its end is stamped by WorkgroupStamp's
  // destructor on every way out
  struct WorkgroupStamp {
    unsigned long long *at, t0;
    __device__ ~WorkgroupStamp() {
      if (at && threadIdx.x == 0) {
        at[0] = t0;
        at[1] = (unsigned long long)wall_clock64();
      }
    }
  } stamp{p.seg.timeline ? p.seg.timeline + 2 * (size_t)blockIdx.x : nullptr, (unsigned long long)wall_clock64()};
#endif
  if constexpr (SEGMENTED) {
    static_assert(DIR == 2, "segmented twins exist for the merged launch only");
    __shared__ SegShared sh;
    if (!seg_draw(p, &sh)) return;
    const int k = p.order[sh.b];
    if (sh.s > 0 && !seg_wait(p, &sh)) return;
    if (sh.backward)
      paint_backward<S, TAIL, MODE, WAVES, LIVE, true>(p, k, stage[lk.w], lk, &sh);
    else
      paint_forward<S, FTAIL, MODE, WAVES, LIVE, true>(p, k, stage[lk.w], lk, &sh);
    return;
  }
  int b = blockIdx.x;
  bool backward = DIR == 1;
  if (DIR == 2) {
    // (merge_order is always 0: backward blocks first.  The dead branch stays: without it the register allocator
    //  gives this kernel 68 B of scratch at S >= 32, DESIGN_NOTES.md 13)
    if (p.merge_order == 1) {
      backward = !(b & 1);
      b >>= 1;
    } else {
      backward = b < p.nloc;
      if (!backward) b -= p.nloc;
    }
  }
  const int k = p.order[b];
#ifdef RL_STATS
  // experiment builds: the counters are gathered in LDS (an atomic to global memory per sum and counter made the
  // kernel 25 x slower and the cycle counts meaningless) and added to the global ones once per workgroup
  __shared__ unsigned long long lstats[32];
  if (threadIdx.x < 32) lstats[threadIdx.x] = 0;
  __syncthreads();
  PaintParams q = p;
  if (p.stats) q.stats = lstats;
  if (backward)
    paint_backward<S, TAIL, MODE, WAVES, LIVE>(q, k, stage[lk.w], lk);
  else
    paint_forward<S, FTAIL, MODE, WAVES, LIVE>(q, k, stage[lk.w], lk);
  __syncthreads();
  if (p.stats && threadIdx.x < 32 && lstats[threadIdx.x]) atomicAdd(&p.stats[threadIdx.x], lstats[threadIdx.x]);
#else
  if (backward)
    paint_backward<S, TAIL, MODE, WAVES, LIVE>(p, k, stage[lk.w], lk);
  else
    paint_forward<S, FTAIL, MODE, WAVES, LIVE>(p, k, stage[lk.w], lk);
#endif
}

// This translation unit holds one variant of every tile (launch.h tile_fit): RL_FIT = 0 the loose one, which is the
// tile list's, 1 / 2 the tight ones, 3 tight minus one.
#ifdef RL_SEG
// ... and, at -DRL_SEG, the segmented twins of that variant's merged launch, alone in a translation unit of their own
template <>
hipError_t launch_paint_seg_variant<RL_MODE, RL_FIT>(const PaintParams &p, int tile, int waves, hipStream_t stream) {
  return dispatch_tile(tile, waves, [&](auto s, auto t, auto w) {
    constexpr int S = s(), WAVES = w();
    constexpr int TAIL = RL_FIT == 0 ? t() : 4, LIVE = RL_FIT == 3 ? S - 1 : S;
    constexpr int FTAIL = RL_FIT == 0 ? TAIL : RL_FIT == 1 ? 1 : RL_FIT == 2 ? 4 : 2;
    if constexpr ((RL_FIT == 0 || tile_fit_built(RL_MODE, S, WAVES)) && paint_segments_built(RL_MODE, S, WAVES, RL_FIT)) {
      return launch_paint_segments(&paint_kernel<S, TAIL, RL_MODE, WAVES, 2, LIVE, FTAIL, true>, p, WAVES, stream);
    } else {
      return hipErrorInvalidValue;
    }
  });
}
#else
template <>
hipError_t launch_paint_variant<RL_MODE, RL_FIT>(const PaintParams &p, int tile, int waves, int dir,
                                                 hipStream_t stream) {
  return dispatch_tile(tile, waves, [&](auto s, auto t, auto w) {
    constexpr int S = s(), WAVES = w();
    constexpr int TAIL = RL_FIT == 0 ? t() : 4, LIVE = RL_FIT == 3 ? S - 1 : S;
    constexpr int FTAIL = RL_FIT == 0 ? TAIL : RL_FIT == 1 ? 1 : RL_FIT == 2 ? 4 : 2;
    if constexpr (RL_FIT == 0 || tile_fit_built(RL_MODE, S, WAVES)) {
      const auto kernel_of = [](auto d) {
        return &paint_kernel<S, TAIL, RL_MODE, WAVES, decltype(d)::value, LIVE, FTAIL>;
      };
      return launch_paint_dir(kernel_of, p, WAVES, dir, stream);
    } else {
      return hipErrorInvalidValue;
    }
  });
}

#if RL_FIT == 0
template <>
hipError_t launch_paint_mode<RL_MODE>(const PaintParams &p, int tile, int waves, int dir, hipStream_t stream,
                                      int fit) {
  const int variant = tile_fit(p.lay, tile, fit != 0 && tile_fit_built(RL_MODE, tile, waves)).variant;
#if RL_MODE < 2
  if (p.seg.nb > 1 || p.seg.nf > 1) {  // (context.cpp paint_segments_rule: the merged launch alone)
    if (dir != 2) return hipErrorInvalidValue;
    switch (variant) {
      case 0: return launch_paint_seg_variant<RL_MODE, 0>(p, tile, waves, stream);
      case 1: return launch_paint_seg_variant<RL_MODE, 1>(p, tile, waves, stream);
      case 2: return launch_paint_seg_variant<RL_MODE, 2>(p, tile, waves, stream);
      default: return launch_paint_seg_variant<RL_MODE, 3>(p, tile, waves, stream);
    }
  }
#endif
  switch (variant) {
    case 0: return launch_paint_variant<RL_MODE, 0>(p, tile, waves, dir, stream);
    case 1: return launch_paint_variant<RL_MODE, 1>(p, tile, waves, dir, stream);
    case 2: return launch_paint_variant<RL_MODE, 2>(p, tile, waves, dir, stream);
    default: return launch_paint_variant<RL_MODE, 3>(p, tile, waves, dir, stream);
  }
}
#endif
#endif  // RL_SEG

}  // namespace rl
