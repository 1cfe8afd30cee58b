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

// ---- segmented passes (K1's merged launch) ------------------------------------
// A pass cut into segments that hand their state over through HBM: the workgroups of a launch are dealt segment by
// segment over all chains (a chain: one pass of one target), so that all chains advance together and the launch ends
// with one segment's tail instead of one pass's (DESIGN.md "Segmented passes").  A workgroup draws a ticket; tickets
// map to items direction-major and segment-major -- every chain's backward segment 0 in launch order, then segment 1,
// ..., then the forward segments alike --, so an item waits only for an item with a smaller ticket, whose holder is
// resident or done: no wait can form a cycle whatever order the dispatcher starts workgroups in.
// Hand-off: plain stores of the state, every storing wave's vmcnt(0), the workgroup's barrier, one lane's agent-scope
// release and wait, a relaxed agent-scope store of the chain's flag; the consumer polls that word relaxed, acquires
// once at agent scope, waits and joins the barrier in front of the other lanes' loads.  The state comes back by vector
// loads alone (nothing handed over goes through the scalar cache).
typedef __attribute__((address_space(1))) unsigned SegWord;
struct SegShared {
  int backward, b, chain, s, nseg;  // this workgroup's item: segment s of nseg of chain `chain` (launch position b)
  int left, failed;                 // the launch was given up before / while this workgroup waited
};
constexpr unsigned long long PAINT_SEG_TIMEOUT = PAINT_SEG_TIMEOUT_S * 100000000ull;  // wall_clock64 counts at 100 MHz
#define RL_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// draw the workgroup's ticket and look at the error word; false: leave
RL_DEV bool seg_draw(const PaintParams &p, SegShared *sh) {
  if (threadIdx.x == 0) {
    SegWord *const ctl = (SegWord *)p.seg.ctl;
    int t = (int)__hip_atomic_fetch_add(ctl, 1u, RL_RELAXED_AGENT);
    sh->left = __hip_atomic_load(ctl + 1, RL_RELAXED_AGENT) != 0u;
    const int nback = p.seg.nb * p.nloc;
    sh->backward = t < nback;
    if (t >= nback) t -= nback;
    sh->s = t / p.nloc;
    sh->b = t % p.nloc;
    sh->nseg = sh->backward ? p.seg.nb : p.seg.nf;
    sh->chain = (sh->backward ? 0 : p.nloc) + sh->b;
  }
  __syncthreads();
  return !sh->left;
}
// wait until the segment before this one has published the chain's state; false: the wait ran out (or another
// workgroup's had) and the launch is given up -- the error word is set, every later workgroup leaves at its ticket
RL_DEV bool seg_wait(const PaintParams &p, SegShared *sh) {
  if (threadIdx.x == 0) {
    SegWord *const ctl = (SegWord *)p.seg.ctl, *const flag = ctl + PAINT_SEG_CTL + sh->chain;
    const unsigned want = (unsigned)sh->s;
    const unsigned long long t0 = wall_clock64();
    int failed = 0;
    while (__hip_atomic_load(flag, RL_RELAXED_AGENT) != want) {
      __builtin_amdgcn_s_sleep(32);
      if (wall_clock64() - t0 > PAINT_SEG_TIMEOUT || __hip_atomic_load(ctl + 1, RL_RELAXED_AGENT) != 0u) {
        __hip_atomic_store(ctl + 1, 1u, RL_RELAXED_AGENT);
        failed = 1;
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh->failed = failed;
  }
  __syncthreads();
  return !sh->failed;
}
RL_DEV double uniform_f64(double v) {
  const long long x = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// the state of a chain as its last segment left it: the LIVE state registers of every lane, raw; the logscale, the
// step's factor and the stone cursor from the chain's record (stored by one lane, loaded by all, made uniform)
template <int S, int LIVE, int WAVES>
RL_DEV void seg_restore(const PaintParams &p, double (&v)[S], int lane, int wv, int chain, double &ls, double &cfac,
                        int &cursor) {
  const double *st = p.seg.state + ((size_t)chain * WAVES + wv) * (LIVE * 64) + lane;
  const double *rec = p.seg.rec + (size_t)chain * PAINT_SEG_REC;
  asm volatile("" : "+v"(st), "+v"(rec));  // vector loads
#pragma unroll
  for (int j = 0; j < LIVE; j++) v[j] = st[j * 64];
  ls = uniform_f64(rec[0]);
  cfac = uniform_f64(rec[1]);
  cursor = __builtin_amdgcn_readfirstlane((int)rec[2]);
}
// ... and left for the next one, behind the last step's stones; then the chain's flag says so
template <int S, int LIVE, int WAVES>
RL_DEV void seg_save(const double (&v)[S], int lane, int wv, const double &ls, const double &cfac, int cursor,
                     const SegShared *sh) {
  const ColdParams cp = cold_params<PaintParams>();
  const int chain = sh->chain;
  double *st = cp->seg.state + ((size_t)chain * WAVES + wv) * (LIVE * 64) + lane;
#pragma unroll
  for (int j = 0; j < LIVE; j++) st[j * 64] = v[j];
  if (lane == 0 && wv == 0) {
    double *rec = cp->seg.rec + (size_t)chain * PAINT_SEG_REC;
    rec[0] = ls;
    rec[1] = cfac;
    rec[2] = (double)cursor;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store((SegWord *)cp->seg.ctl + PAINT_SEG_CTL + chain, (unsigned)(sh->s + 1), RL_RELAXED_AGENT);
  }
}

}  // namespace rl
