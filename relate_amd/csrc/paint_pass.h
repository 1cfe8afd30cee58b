// paint_pass.h -- what a pass of the Li-Stephens kernels is made of, once: the FP64 forward step body, the forward
// row pipeline, a target's slice of the plan and the stepping stones.  paint_kernels.hip (K1), paint32_kernels.hip
// (K1 on packed FP32) and repaint_kernels.hip (K2) put their passes together from these; the primitives underneath
// (masks, exec-masked operations, set_slot) are paint_device.h, the sums exact_sum.h.
//
// Everything here is inlined into its caller (RL_DEV): the kernels sit at 225-256 VGPRs, and a helper that changed a
// register or scratch number of one of them would not be here (DESIGN_NOTES.md 13).
#pragma once
#include "paint_device.h"
#include "exact_sum.h"

namespace rl {

typedef float f32x2 __attribute__((ext_vector_type(2)));  // two donors of the packed-FP32 state
typedef const __attribute__((address_space(4))) PaintParams *ColdParams;

// ---- a target's slice of the plan -------------------------------------------
// visited sites ib .. ib + D - 1 of target k: their site words, interval coefficients and nor_x_theta terms (the
// plan arrays come in by vector loads, requested a step ahead)
struct PlanSlice {
  int D;
  const int32_t *st;
  const double *cfp, *nx;
};
template <typename P>
RL_DEV PlanSlice plan_slice(const P &p, int k, int ib, int D) {
  const int64_t off = p.plan_off[k] + ib;
  return {D, p.sites + off, p.cf + off, p.nxt + off};
}
template <typename P>
RL_DEV PlanSlice plan_slice(const P &p, int k) {  // all of them
  return plan_slice(p, k, 0, (int)(p.plan_off[k + 1] - p.plan_off[k]));
}

// ---- the forward step body (FP64) -------------------------------------------
// forward: a = (a + cfac) * (mismatch ? K1 : 1.0) over the masks of `row`, chunk 0 of it already requested
// (fast_painting.cpp:288-295); returns the lane's share of the serial sum (:300-303).  Registers S - TAIL .. LIVE - 1
// carry the validity test; registers from LIVE on (a K1 tile fitted to N: at most the last one) hold no donor in any
// lane and are left out.
template <int S, int TAIL, int CH, int LIVE = S>
RL_DEV double forward_update(double (&a)[S], MaskRow row, typename MaskChunk<CH>::type first, const int &len,
                             const double &cfac, const double &K1) {
  typedef typename MaskChunk<CH>::type Chunk;
  double lsum = 0.0;
  for_each_chunk_from<S, CH>(row, first, [&](int j0, const Chunk &m) {
    double v[CH];
#pragma unroll
    for (int jj = 0; jj < CH; jj++) {
      if (j0 + jj >= LIVE) continue;
      v[jj] = a[j0 + jj];
      if (j0 + jj < S - TAIL)
        v[jj] = v[jj] + cfac;
      else
        tail_add(v[jj], len, j0 + jj, cfac);  // slots past the lane's run stay +0.0
    }
    // v *= (mismatch ? K1 : 1.0)
    if (j0 + 8 <= LIVE)
      masked_mul8<0>(v, m, K1);
    else
      masked_mul7<0>(v, m, K1);
    if constexpr (CH == 16) {
      if (j0 + 16 <= LIVE)
        masked_mul8<8>(v + 8, m, K1);
      else
        masked_mul7<8>(v + 8, m, K1);
    }
#pragma unroll
    for (int jj = 0; jj < CH; jj++) {
      if (j0 + jj >= LIVE) continue;
      a[j0 + jj] = v[jj];
      lsum += v[jj];
    }
  });
  return lsum;
}

// ---- row pipeline -----------------------------------------------------------
// A step reads its site's row of masks with scalar loads, the first chunk requested before the previous step's sum;
// the row of the step after it is pulled into L2 by a vector load during the step (touch_row).  P is PaintParams or
// RepaintParams (masks, L); st, D the target's visited sites, whatever part of them the pass walks.
template <int S, int WAVES>
struct ForwardRows {
  const int32_t *st;
  int D;
  int s1, s2;  // at the top of step i the sites of steps i, i + 1; below advance() those of i + 1, i + 2
  uint32_t touched = 0;
  RL_DEV ForwardRows(const int32_t *st_, int D_, int i0)  // i0: the first step
      : st(st_), D(D_), s1(D_ > i0 ? st_[i0] : 0), s2(D_ > i0 + 1 ? st_[i0 + 1] : 0) {}
  RL_DEV void retire() const { retire_touch(touched); }
  template <typename P>
  RL_DEV void advance(const P &p, int i, int lane, int wv) {
    if (i + 1 < D) touched = touch_row(p.masks, S, s2, lane, WAVES, wv);
    s1 = s2;
    if (i + 2 < D) s2 = st[i + 2];
  }
  template <typename P>
  RL_DEV MaskRow row(const P &p, int wv) const {
    return site_row(p.masks, S, p.L, s1, WAVES, wv);
  }
};

// ---- stepping stones --------------------------------------------------------
// Write the lane's registers as one stepping stone in donor order.  Stones
// are rare (W per target against D_k steps); to keep S per-register store
// addresses out of the hot loop's register budget the registers are staged,
// 16 at a time, through a 4 KiB LDS strip private to the wave and written by a
// rolled loop (each lane reads back only what it wrote: no barrier needed).
// The slot of donor k itself (held at +0.0) is written as self_value.
// Two overloads, for the two forms of state: doubles, one per register ...
template <int S, int LIVE = S>
RL_DEV void emit_stone(const PaintLane<S> &pl, const double (&v)[S], float *__restrict__ out, float self_value,
                       float *stage) {
  static_assert(S % 8 == 0, "S must be a multiple of 8");
  constexpr int R = S % 16 == 0 ? 16 : 8;
#pragma unroll
  for (int c = 0; c < S / R; c++) {
#pragma unroll
    for (int ii = 0; ii < R; ii++) {
      // pin the conversion to its chunk: hoisted, all S floats would be live at once
      if (c * R + ii >= LIVE) continue;  // (no lane's run reaches it: never read back below)
      double x = v[c * R + ii];
      asm volatile("" : "+v"(x) : : "memory");
      stage[ii * 64 + pl.lane] = (float)x;
    }
#pragma clang loop unroll(disable)
    for (int ii = 0; ii < R; ii++) {
      const int i = c * R + ii;
      const int n = pl.start + i;
      if (i < pl.len) out[n] = (n == pl.k) ? self_value : stage[ii * 64 + pl.lane];
    }
  }
}
// ... and packed floats, two per register (paint32_kernels.hip).  (One body over a per-chunk staging helper costs the
// packed-FP32 kernel registers: DESIGN_NOTES.md 13.)
template <int S, int LIVE = S>
RL_DEV void emit_stone(const PaintLane<S> &pl, const f32x2 (&v)[S / 2], float *__restrict__ out, float self_value,
                       float *stage) {
  constexpr int R = S % 16 == 0 ? 16 : 8;
#pragma unroll
  for (int c = 0; c < S / R; c++) {
#pragma unroll
    for (int ii = 0; ii < R; ii += 2) {
      f32x2 x = v[(c * R + ii) / 2];
      asm volatile("" : "+v"(x) : : "memory");
      stage[ii * 64 + pl.lane] = x.x;
      stage[(ii + 1) * 64 + pl.lane] = x.y;
    }
#pragma clang loop unroll(disable)
    for (int ii = 0; ii < R; ii++) {
      const int i = c * R + ii;
      const int n = pl.start + i;
      if (i < pl.len) out[n] = (n == pl.k) ? self_value : stage[ii * 64 + pl.lane];
    }
  }
}

// index of forward stone w (behind the range: none)
RL_DEV int forward_stone_index(int k, int w) {
  const ColdParams cp = cold_params<PaintParams>();
  return w <= cp->w_last ? cp->stone_ia[(size_t)k * cp->W + w] : -1;
}
RL_DEV int backward_stone_index(int k, int w) {
  const ColdParams cp = cold_params<PaintParams>();
  return w >= cp->w_first ? cp->stone_ie[(size_t)k * cp->W + w] : -2;
}
// forward stone w: the state a, its logscale ls; then on to stone w + 1
template <int S, int LIVE = S, typename V>
RL_DEV void write_forward_stone(int &w, const PaintLane<S> &pl, const int &wv, const V &a, const double &ls,
                                float *stage) {
  const ColdParams cp = cold_params<PaintParams>();
  if (w >= cp->w_first) {
    const size_t N = cp->lay.N, row = (size_t)(w - cp->w_first) * cp->nloc + (pl.k - cp->k0);
    emit_stone<S, LIVE>(pl, a, cp->alpha + row * N, 0.0f, stage);
    if (pl.lane == 0 && wv == 0) cp->ls_alpha[row] = (float)ls;
  }
  w++;
}
// backward stone w (self_value: beta[k] = 1 at the last SNP, +0.0 from then on); then on to stone w - 1
template <int S, int LIVE = S, typename V>
RL_DEV void write_backward_stone(int &w, const PaintLane<S> &pl, const int &wv, const V &b, const double &ls,
                                 float self_value, float *stage) {
  const ColdParams cp = cold_params<PaintParams>();
  if (w <= cp->w_last) {
    const size_t N = cp->lay.N, row = (size_t)(w - cp->w_first) * cp->nloc + (pl.k - cp->k0);
    emit_stone<S, LIVE>(pl, b, cp->beta + row * N, self_value, stage);
    if (pl.lane == 0 && wv == 0) cp->ls_beta[row] = (float)ls;
  }
  w--;
}

}  // namespace rl
