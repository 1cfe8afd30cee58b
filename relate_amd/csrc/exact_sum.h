// exact_sum.h -- the reference's SERIAL double-precision sum, reproduced bit
// for bit by a wavefront in parallel.
//
// Problem.  The reference adds the N donor terms left to right
// (fast_painting.cpp:300-303, 495-503); the result is not the correctly
// rounded sum but carries that particular order's roundings, and the tree
// builder downstream breaks exact float ties, so the order must be kept
// (SURVEY.md 7 H1).  A literal serial sum costs one dependent add per donor
// (sum_exact: 64*S wave instructions per step).
//
// Idea.  Lane l owns a contiguous run of terms.  If lane l knew its exact
// entry value s_l it could add its run serially on its own, and all lanes
// could do so at once.  It does not, but:
//   (1) an ordinary parallel scan gives P_l with |s_l - P_l| <= 10250 ulp
//       (each of the <= 10240 additions of either order errs by <= 1/2 ulp
//       of a partial sum; typically a few tens of ulp);
//   (2) within one binade, fl(a + x) - a depends on `a` only through the
//       parity of a/ulp (round-half-even), and across ONE binade crossing only
//       through a mod 4 ulp.  So lane l runs its serial sum from four starts
//       r_0..r_3 with r_h = h (mod 4 ulp), and the true run is the run of the
//       matching r_h translated by the constant s_l - r_h (a multiple of 4 ulp)
//       -- provided the true run and that r_h-run change binade at the same
//       terms;
//   (3) r_0 and r_3 are placed 16384 ulp below / above P_l, so s_l lies between
//       them; fl-addition is monotone in its start value, hence if the r_0 and
//       r_3 runs show the same exponent after every term (their high words are
//       xor-ed and or-accumulated term by term) so does every run in between,
//       the true one included.
// In integer offsets delta_l = (s_l - P_l)/ulp a lane without a rounding tie that
// stays in its binade acts as the translation delta -> delta + C; translations
// compose by adding, so one plain integer add-scan over the wavefront composes
// them all at once (wave_scan_u32, walk_enter below).  What remains sequential is
// a walk over the few other lanes, the heads: where a tie made the four runs
// disagree or the run crosses one binade (delta -> (delta >> s) + U_h from a
// 4-entry table, walk_head_hop below; ~2.5 tie lanes per sum at N = 5000 and
// about as many crossings, DESIGN_NOTES 17), or where the run jumps two or more
// binades (a term much larger than the prefix, ~0.65 per sum: that lane redoes
// its run from its exact entry value).  Anything else irregular (P_l within
// 16384 ulp of a power of two, ...) falls back to the literal serial sum for
// that step (measured: < 1e-4 of the steps).  (Targets spread over two waves,
// N > 5120, still compose the crossing lanes in a segmented scan and walk the
// rest: sum_exact_fast_segmented.)
// The result is ALWAYS the serial sum, bit for bit.
#pragma once
#include "paint_device.h"

namespace rl {

// ---- DPP helpers (gfx9 row/bcast controls) -------------------------------
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
RL_DEV double dpp_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, BANK_MASK, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, BANK_MASK, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
RL_DEV int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, BANK_MASK, true);
}
enum { DPP_ROW_SHR = 0x110, DPP_WAVE_SHR1 = 0x138, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143 };

// inclusive scan over the 64 lanes (zeros shifted in)
RL_DEV double wave_scan_f64(double v) {
  v += dpp_f64<DPP_ROW_SHR + 1>(v);
  v += dpp_f64<DPP_ROW_SHR + 2>(v);
  v += dpp_f64<DPP_ROW_SHR + 4>(v);
  v += dpp_f64<DPP_ROW_SHR + 8>(v);
  v += dpp_f64<DPP_ROW_BCAST15, 0xa>(v);
  v += dpp_f64<DPP_ROW_BCAST31, 0xc>(v);
  return v;
}
// the same over unsigned integers modulo 2^32: each step is one v_add_u32 with a DPP operand (the zero shifted in,
// and read by the rows a broadcast step does not select, is the identity: such a row keeps its value)
RL_DEV unsigned wave_scan_u32(unsigned v) {
  v += (unsigned)dpp_i32<DPP_ROW_SHR + 1>((int)v);
  v += (unsigned)dpp_i32<DPP_ROW_SHR + 2>((int)v);
  v += (unsigned)dpp_i32<DPP_ROW_SHR + 4>((int)v);
  v += (unsigned)dpp_i32<DPP_ROW_SHR + 8>((int)v);
  v += (unsigned)dpp_i32<DPP_ROW_BCAST15, 0xa>((int)v);
  v += (unsigned)dpp_i32<DPP_ROW_BCAST31, 0xc>((int)v);
  return v;
}
RL_DEV int hi32(double v) { return (int)(__double_as_longlong(v) >> 32); }
RL_DEV int expo_field(double v) { return (hi32(v) >> 20) & 0x7ff; }  // v >= 0
RL_DEV double rd_lane_f64(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// 2^(k) for a biased exponent field f = k + 1023
RL_DEV double pow2_field(int f) { return __longlong_as_double((long long)f << 52); }

// Term generators.  for_each(th, nth, f) calls f(i, term_i) for the lane's S
// terms in order; the two weights are passed in so that each pass of
// sum_exact_fast can use its own opaque copies: otherwise the compiler shares
// the S selected weights (or the S products) between the passes and keeps them
// alive in registers.
// LIVE (S or S - 1): the registers that hold a donor in some lane; a K1 tile fitted to N (launch.h tile_fit) leaves
// the last one out of every pass.  Its term would be +0.0, which changes no partial sum.
template <int S, int LIVE = S>
struct RegTerm {  // forward: the terms are the alpha registers themselves
  static constexpr bool REG = true;
  const double (&a)[S];
  double th = 0.0, nth = 0.0;
  unsigned long long *stats = nullptr;  // experiment builds (-DRL_STATS) only
  RL_DEV double get(int i, double, double) const { return a[i]; }
  template <typename F>
  RL_DEV void for_each(double &, double &, F &&f) const {
#pragma unroll
    for (int i = 0; i < LIVE; i++) f(i, a[i]);
  }
};
template <int S, int LIVE = S>
struct MaskTerm {  // backward, lane-mask panel: e(i) * beta[i] with the site's row words as EXEC masks
  static constexpr bool REG = false;
  MaskRow row;  // mismatch row of the site (S words)
  const double (&b)[S];
  double th, nth;
  unsigned long long *stats = nullptr;
  template <typename F>
  RL_DEV void for_each(double &t, double &n, F &&f) const {
    for_each_chunk<S, 4>(row, [&](int j0, const u64x4 &m) {
      double x[4];
      if (j0 + 4 <= LIVE)
        weighted4(x, b[j0], b[j0 + 1], b[j0 + 2], b[j0 + 3], m, t, n);
      else
        weighted3(x, b[j0], b[j0 + 1], b[j0 + 2], m, t, n);
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
        if (j0 + jj < LIVE) f(j0 + jj, x[jj]);
    });
  }
};

// K1's backward pass: the update loop has just produced every weighted term (backward4); the first KS of them are
// kept in a wave-private LDS region instead of being recomputed by each pass of the sum (the chains, a rerun of
// the walk, the literal fallback) -- 2 VALU, 1.25 SALU and a quarter of a mask chunk per term and pass.  The region
// is [pair of terms][lane][2] doubles, one ds_write_b128 / ds_read_b128 per lane and pair; a lane reads back only
// what it wrote, bit for bit, so no barrier is needed and the sum cannot change.  Of the remaining S - KS terms
// the last R stay in registers (reg_stash_terms below), the others are recomputed as in MaskTerm.
//
// KS: the stash never takes LDS that another wave needs.  A tile's registers allow tile_waves_per_simd(S) waves on
// a SIMD (tools/kernel_resources.sh); the stash gets that wave's share of the CU's 160 KB less 512 B (WaveLink, the
// counters of experiment builds, allocation granule), in whole chunks of 4 terms, 36 at the most: 36 of the 80
// terms at the headline tile (18 KB per wave, eight waves per CU).  (Config #4's tile with all its 32 terms
// stashed: 16 KB per wave, 10 instead of 16 waves per CU, the Paint 35 % slower.)
constexpr int STASH_MAX = 36;
constexpr int LDS_PER_CU = 160 * 1024;
// (tile_waves_per_simd: device_types.h, the host sizes the segmented launch by it)
constexpr int stash_terms(int S) {
  const int fit = (LDS_PER_CU / (4 * tile_waves_per_simd(S)) - 512) / (64 * (int)sizeof(double));
  const int ks = fit < S ? fit : S;
  return (ks < STASH_MAX ? ks : STASH_MAX) / 4 * 4;
}
constexpr int stash_bytes(int S) { return stash_terms(S) * 64 * (int)sizeof(double); }
// The LAST R weighted terms of a step stay where the update loop produced them, in registers (StashTerm::xr): the
// chunks produced last add the least pressure inside the update loop, and a held term costs no LDS traffic at all.
// R is what the tile's registers leave free: the largest multiple of 4 at which every exact K1 kernel of the tile --
// four fit variants, one and two waves per target, each launch direction -- keeps zero scratch and the waves per SIMD
// of tile_waves_per_simd (tools/kernel_resources.sh, profiles/regstash_kernel_resources.txt).  The two tiles of the
// two-wave-per-SIMD configurations have the most terms left to recompute (28 and 44): S = 64 holds all of them
// (KS + R = S, its recompute loop is empty), S = 80 the 12 that fit; the smaller tiles have no register to spare and
// keep their step loops instruction for instruction.
constexpr int reg_stash_terms(int S) { return S == 80 ? 12 : S == 64 ? 28 : 0; }
// the update loop's side: term i of the step (register j0 + jj of chunk j0) goes into xr if it is one of the last R
template <int S, int R>
RL_DEV void hold_term(double (&xr)[R > 0 ? R : 1], int i, double x) {
  if constexpr (R > 0)
    if (i >= S - R) xr[i - (S - R)] = x;
}
constexpr int STASH_AHEAD = 2;  // pairs of terms requested ahead of the one in work (StashTerm::for_each)
typedef double f64x2 __attribute__((ext_vector_type(2)));
// (may_alias: the region shares storage with the float staging strip of the stones)
typedef f64x2 __attribute__((may_alias)) StashPair;
typedef __attribute__((address_space(3))) StashPair *StashPtr;
// this lane's view of its wave's region (16-byte aligned): pair p = terms 2p, 2p + 1 at sp[64 * p]
RL_DEV StashPtr stash_of(void *wave_region) { return (StashPtr)wave_region + (threadIdx.x & 63); }
RL_DEV void stash_put4(StashPtr sp, int chunk, const double (&x)[4]) {
  StashPair lo, hi;
  lo.x = x[0]; lo.y = x[1]; hi.x = x[2]; hi.y = x[3];
  sp[128 * chunk] = lo;
  sp[128 * chunk + 64] = hi;
}
// a chunk whose fourth term does not exist (LIVE = S - 1 where the stash holds all S terms, S = 8): its half of the
// second pair stays unwritten and unread
RL_DEV void stash_put3(StashPtr sp, int chunk, const double (&x)[4]) {
  StashPair lo;
  lo.x = x[0]; lo.y = x[1];
  sp[128 * chunk] = lo;
  *(__attribute__((address_space(3))) double __attribute__((may_alias)) *)&sp[128 * chunk + 64] = x[2];
}
// Terms 0 .. KS-1 come from LDS, terms S-R .. LIVE-1 from registers, terms KS .. S-R-1 are recomputed.
template <int S, int LIVE = S, int R = reg_stash_terms(S)>
struct StashTerm {
  static constexpr bool REG = false;
  static constexpr int KS = stash_terms(S);
  static_assert(R % 4 == 0 && KS + R <= S, "the register-held chunks lie behind the stashed ones");
  MaskRow row;  // mismatch row of the site (S words)
  const double (&b)[S];
  double th, nth;
  unsigned long long *stats;
  StashPtr sp;                       // terms 0 .. KS-1 as the update loop left them
  const double (&xr)[R > 0 ? R : 1];  // terms S-R .. LIVE-1 as the update loop left them (R = 0: never read)
  template <typename F>
  RL_DEV void for_each(double &t, double &n, F &&f) const {
    constexpr int NP = KS / 2, NS = KS / 4, NC = (S - R) / 4, A = STASH_AHEAD;
    // The LDS reads run A pairs of terms ahead, as the mask loads of for_each_chunk run a chunk ahead: wait for pair
    // p, request pair p + A, then work on pair p.  (Without the tie to pair p the scheduler requests all KS terms at
    // once and keeps them.)
    StashPtr q = sp;
    MaskRow r = row;
    asm volatile("" : "+v"(q));  // (the fallback's round loop must not hoist the reads either)
    StashPair w[A + 1];
#pragma unroll
    for (int pr = 0; pr < A && pr < NP; pr++) w[pr] = q[64 * pr];
    u64x4 m = {0, 0, 0, 0};
#pragma unroll
    for (int pr = 0; pr < NP; pr++) {
      const StashPair &cur = w[pr % (A + 1)];
      if (pr + A < NP) {
        asm volatile("" : "+v"(q) : "v"(cur));
        w[(pr + A) % (A + 1)] = q[64 * (pr + A)];
      } else if (pr + 1 == NP && NS < NC) {  // no LDS read is left in flight: the masks of the first recomputed chunk
        asm volatile("" : "+s"(r) : "v"(cur));
        m = load_masks<4>(r, NS);
      }
      f(2 * pr, cur.x);
      if (2 * pr + 1 < LIVE) f(2 * pr + 1, cur.y);
    }
#pragma unroll
    for (int c = NS; c < NC; c++) {
      u64x4 nm = m;
      if (c + 1 < NC) {
        asm volatile("" : "+s"(r) : "s"(m[0]));
        nm = load_masks<4>(r, c + 1);
      }
      double x[4];
      if (4 * c + 4 <= LIVE)
        weighted4(x, b[4 * c], b[4 * c + 1], b[4 * c + 2], b[4 * c + 3], m, t, n);
      else
        weighted3(x, b[4 * c], b[4 * c + 1], b[4 * c + 2], m, t, n);
#pragma unroll
      for (int jj = 0; jj < 4; jj++)
        if (4 * c + jj < LIVE) f(4 * c + jj, x[jj]);
      m = nm;
    }
#pragma unroll
    for (int i = S - R; i < LIVE; i++) f(i, xr[i - (S - R)]);
  }
};

// ---- targets spread over several waves ------------------------------------
// For N > 5120 the stepping-stone kernel gives a target to a workgroup of
// WAVES = 2 waves (virtual lanes 0..127, wave w holds lanes 64w..64w+63) so
// that each lane keeps S <= 80 registers.  A sum then runs over the waves in
// order; they meet in LDS (WaveLink) at workgroup barriers.  With WAVES = 1
// every exchange below compiles away.
struct WaveLinkStorage {
  double tot[2][2];  // [phase][wave]: approximate total of the wave's lane sums
  double result;     // the finished sum / the hand-over value of the serial fallback
  int bad[2];        // wave w needs the fallback
  int delta;         // exact offset at the exit of wave 0 (units: ulp of its exit binade)
};
template <int WAVES>
struct WaveLink {
  WaveLinkStorage *s = nullptr;
  int w = 0;          // this wave
  unsigned phase = 0;  // alternates per sum: a wave may run one sum ahead of the other
  RL_DEV void barrier() const {
    if constexpr (WAVES > 1) __syncthreads();
  }
};
// the link of this wave of a workgroup of WAVES waves (the prologue of every kernel that sums)
template <int WAVES>
RL_DEV WaveLink<WAVES> make_wave_link(WaveLinkStorage *storage) {
  WaveLink<WAVES> lk;
  lk.s = storage;
  lk.w = WAVES > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  return lk;
}
// The `lanes` order: the wave's (workgroup's) total of one value per lane as a balanced tree, in double.
template <int WAVES>
RL_DEV double lanes_total(double lane_sum, WaveLink<WAVES> &lk) {
  lk.phase++;
  const double t = wave_sum_butterfly(lane_sum);
  if constexpr (WAVES == 1) {
    return t;
  } else {  // the top level of the balanced tree over 128 lane sums
    const unsigned ph = lk.phase & 1u;
    if ((threadIdx.x & 63) == 0) lk.s->tot[ph][lk.w] = t;
    lk.barrier();
    return lk.s->tot[ph][0] + lk.s->tot[ph][1];
  }
}

// The literal serial sum as the rare-path fallback of sum_exact_fast: same
// result as sum_exact, but the terms are recomputed in every round (the empty
// asm stops the compiler from hoisting S doubles of terms out of the round
// loop, which would cost the hot path its registers).
template <int S, typename T>
RL_DEV double sum_exact_fallback(const T &term, double s = 0.0) {
  for (int l = 0; l < 64; l++) {
    double th = term.th, nth = term.nth;
    double tmp = s;
    term.for_each(th, nth, [&](int, double x) {
      tmp += x;
      if constexpr (!T::REG) asm volatile("" : "+v"(th), "+v"(nth), "+v"(tmp));
    });
    s = wave_bcast(tmp, l);
  }
  return s;
}
// the same over the waves of a workgroup, in order; every wave returns the total
template <int S, int WAVES, typename T>
RL_DEV double sum_exact_fallback_linked(const T &term, const WaveLink<WAVES> &lk) {
  if constexpr (WAVES == 1) {
    return sum_exact_fallback<S>(term);
  } else {
    double r = 0.0;
    if (lk.w == 0) {
      r = sum_exact_fallback<S>(term);
      if ((threadIdx.x & 63) == 0) lk.s->result = r;
    }
    lk.barrier();
    if (lk.w == 1) {
      r = sum_exact_fallback<S>(term, lk.s->result);
    }
    lk.barrier();  // wave 0 has handed over; wave 1 may now overwrite
    if (lk.w == 1 && (threadIdx.x & 63) == 0) lk.s->result = r;
    lk.barrier();
    r = lk.s->result;
    lk.barrier();  // everyone has read it before the next sum writes
    return r;
  }
}

// ---- the walk's hop over a tie lane ----------------------------------------
// A lane whose four runs disagree (a rounding tie) maps its entry offset delta to
//   A_h + ((delta - B_h) >> sh),   h = (p0 + delta) & 3,
// A_h the exit offsets of the four runs, B_h the entry offsets of their starts (walk_hop_reference, the literal form).
// B_h = h - p0 (mod 4) for all four starts (G4 is a multiple of 4) and delta = h - p0 (mod 4) by the choice of h, so
// delta - B_h is a multiple of 4 and for sh in {0, 1} the shift distributes exactly:
//   A_h + ((delta - B_h) >> sh)  =  (delta >> sh) + U_h,   U_h = A_h - (B_h >> sh).
// U_h is a run's increment less Q - P (small; where sh = 0 and all four agree, the lane is a translation by it), so
// the four fit signed 16-bit fields of two registers, built by all lanes at once during classification, which needs
// them anyway; the walk's dependent path per head with a table is then a shift, an add, a 64-bit shift, a sign
// extension, and one shift of delta and an add -- no select of A_h or B_h by h, and every read from the lane comes
// before it.
// One function each for the kernels and the host (rl_debug_walk_table); integers only.
constexpr int WALK_G4 = 16384;  // half-width of the bracket [r_0, r_3] in ulps
RL_HD inline int walk_hop_reference(int A0, int A1, int A2, int A3, int p0, int sh, int delta) {
  const int h = (p0 + delta) & 3;
  const int A = (h & 2) ? ((h & 1) ? A3 : A2) : ((h & 1) ? A1 : A0);
  const int B = h == 0 ? (-p0 - WALK_G4) : (h == 3 ? (3 - p0 + WALK_G4) : (h - p0));
  return A + ((delta - B) >> sh);
}
// U_h = A_h - (B_h >> sh): run h's exit offset less its shifted entry offset
RL_HD inline int walk_run_offset(int A, int h, int p0, int sh) {
  const int B = h - p0 + (h == 0 ? -WALK_G4 : h == 3 ? WALK_G4 : 0);
  return A - (B >> sh);
}
struct WalkTable {
  int lo, hi;  // U_0 | U_1 << 16,  U_2 | U_3 << 16
  bool ok;     // every U_h is an int16
};
RL_HD inline WalkTable walk_table_pack_runs(int U0, int U1, int U2, int U3) {
  WalkTable t;
  t.ok = (short)U0 == U0 && (short)U1 == U1 && (short)U2 == U2 && (short)U3 == U3;
  t.lo = (int)(((unsigned)U0 & 0xffffu) | ((unsigned)U1 << 16));
  t.hi = (int)(((unsigned)U2 & 0xffffu) | ((unsigned)U3 << 16));
  return t;
}
RL_HD inline WalkTable walk_table_pack(int A0, int A1, int A2, int A3, int p0, int sh) {
  return walk_table_pack_runs(walk_run_offset(A0, 0, p0, sh), walk_run_offset(A1, 1, p0, sh),
                              walk_run_offset(A2, 2, p0, sh), walk_run_offset(A3, 3, p0, sh));
}
// p16 = 16 * p0: the bit offset of the field of the run that starts at the lane's own residue
RL_HD inline int walk_table_hop(int lo, int hi, int p16, int sh, int delta) {
  const unsigned long long t = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  return (delta >> sh) + (int)(short)(unsigned short)(t >> (((delta << 4) + p16) & 48));
}
// The head's meta word of the one-wave walk: p0 in bits 4..5, where the field offset wants it, above it the redo flag
// and sh (sh last: a multi-binade lane's sh spills upwards only, and is read for table lanes alone, where it is 0 or
// 1).  walk_head_hop is walk_table_hop from that word: the field offset is the low six bits of (delta << 4) + meta,
// which is all a 64-bit shift reads, so nothing of meta has to be masked out first.
enum { WALK_META_REDO = 64, WALK_META_SH_BIT = 7 };
RL_HD inline int walk_meta(int p0, int sh, bool redo) {
  return (p0 << 4) | (redo ? WALK_META_REDO : 0) | (sh << WALK_META_SH_BIT);
}
RL_HD inline int walk_head_hop(int lo, int hi, int meta, int delta) {
  const unsigned long long t = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  return (delta >> ((meta >> WALK_META_SH_BIT) & 1)) + (int)(short)(unsigned short)(t >> (((delta << 4) + meta) & 63));
}

// ---- the walk between two heads ----------------------------------------------
// A tie-free lane that stays in its binade (and an exact-entry lane) is a pure translation delta -> delta + C, and
// translations compose by adding: T = the inclusive scan over the wave of (head ? 0 : C), one register, no segments.
// Between heads the walk keeps rel = delta - T, which no translation changes: in front of head q the offset is
// walk_enter(rel, T[q]), behind it rel = walk_leave(delta, T[q]) -- a head adds 0 to the scan, so T[q] = T[q-1], and
// lane q itself is read, never lane q - 1.  rel starts as the entry offset (T
// is 0 in front of lane 0), as walk_leave(A0, T[qc]) behind a `constant` lane qc, and the exit offset of the wave is
// walk_enter(rel, T[63]).
// Only differences of T are used, so its wrap-around modulo 2^32 is harmless: the arithmetic is unsigned.
// The same functions for the kernels and the host (rl_debug_walk_lanes); integers only.
RL_HD inline int walk_enter(int rel, unsigned T) { return (int)((unsigned)rel + T); }
RL_HD inline int walk_leave(int delta, unsigned T) { return (int)((unsigned)delta - T); }

#ifdef RL_STATS
#define RL_CLK() __builtin_readcyclecounter()
#define RL_STAT(i, v) do { if (term.stats && (threadIdx.x & 63) == 0) atomicAdd(&term.stats[i], (unsigned long long)(v)); } while (0)
#else
#define RL_CLK() 0ull
#define RL_STAT(i, v) do { } while (0)
#endif

// L: this lane's serial sum of its terms from +0.0 (the caller accumulates it
// inside its update loop, where the dependent adds hide behind other work).
template <int S, typename T>
RL_DEV double sum_exact_fast(const T &term, double L) {
  constexpr bool REG_TERM = T::REG;
  constexpr int G4 = WALK_G4;  // half-width of the bracket [r_0, r_3] in ulps

  const unsigned long long tk0 = RL_CLK();
  // ---- A. approximate prefix from the lanes' local serial sums
  double Q = wave_scan_f64(L);                // ~ sum over lanes <= l (of this wave)
  double P = dpp_f64<DPP_WAVE_SHR1>(Q);       // ~ entry value of this lane (lane 0: +0.0)
  const long long pb = __double_as_longlong(P);
  // Lanes whose entry value is known exactly need no bracket: nothing but zeros before the lane (entry
  // +0.0; lane 0 always), and lane 1, whose entry is lane 0's local sum -- a serial sum
  // from +0.0, i.e. the true prefix.  Their four runs start AT the entry, so the run is the true one whatever
  // it crosses (lane 1 is where two-binade jumps are most frequent), and the lane's map is the constant
  // exit offset.
  const bool zero_entry = pb == 0 || (threadIdx.x & 63) == 1;

  const unsigned long long tk1 = RL_CLK();
  // ---- B. four runs from r_h = h (mod 4 ulp), r_0 / r_3 bracketing the true entry
  const long long base = pb & ~3ll;
  const int p0 = (int)(pb & 3);
  double c0 = __longlong_as_double(base - G4);
  double c1 = __longlong_as_double(base + 1);
  double c2 = __longlong_as_double(base + 2);
  double c3 = __longlong_as_double(base + 3 + G4);
  if (zero_entry) { c0 = P; c1 = P; c2 = P; c3 = P; }
  const double r0 = c0, r3 = c3;
  const int e_in = expo_field(r0);
  const bool entry_ok = zero_entry || (e_in == expo_field(r3) && e_in > 64);
  int exdiff = 0;  // OR over the terms of (high word of c0) xor (high word of c3)
  double thB = term.th, nthB = term.nth;
  term.for_each(thB, nthB, [&](int, double x) {
    c0 += x;
    c1 += x;
    c2 += x;
    c3 += x;
    // exponent fields of the two bracketing runs must agree after every term:
    // exdiff |= hi(c0) ^ hi(c3), one v_bitop3_b32 per term (bits 20..30 count)
    exdiff = __builtin_amdgcn_bitop3_b32(exdiff, hi32(c0), hi32(c3), 0xF6);
    // Tie the check to its partial sums: otherwise the scheduler first runs the chains to the end and keeps all
    // partial sums alive.  A scheduling barrier, not an empty asm statement with the sums as operands: the hazard
    // recognizer treats an inline asm that names registers a double-precision instruction has just written as a
    // reader of them and puts a wait state in front -- one s_nop per term, 80 of the ~1000 issue slots of a forward
    // step (round 4, seen in the ISA).
    // (The backward pass, whose terms are recomputed here four at a time, keeps the asm statement: with the barrier
    //  alone its chain block spills 47 register pairs.)
    if constexpr (REG_TERM)
      __builtin_amdgcn_sched_barrier(0);
    else
      asm volatile("" : "+v"(exdiff), "+v"(c1), "+v"(c2), "+v"(thB), "+v"(nthB));  // (c0, c3: through exdiff)
  });
  const unsigned long long tk2 = RL_CLK();
  const int e_out = expo_field(c0);
  // exit unit = entry unit of the next lane = ulp of the binade of Q
  const int e_next = expo_field(Q);
  // An exit offset (c - Q) / ulp is asked for only where c lies in Q's binade (every other lane is invalid or walked
  // from its exact entry): there it is the difference of the two bit patterns -- one integer subtraction of the low
  // words instead of a subtraction, a multiplication and a quarter-rate conversion in double precision, six times
  // per sum (round 4).
  const unsigned q_lo = (unsigned)__double_as_longlong(Q);
  auto exit_offset = [&](double c) -> int { return (int)((unsigned)__double_as_longlong(c) - q_lo); };

  // ---- classification
  const bool same_seq = (exdiff >> 20) == 0;
  const int sh = e_out - e_in;
  bool invalid = !entry_ok || !same_seq;
  // the exit must sit in the binade the next lane (or the caller) measures in
  if (!zero_entry && e_out != e_next) invalid = true;
  if (zero_entry && expo_field(c0) != e_next) invalid = true;
  // a run that jumps two or more binades (a term much larger than the prefix)
  // does not fit the mod-4 argument: the walk redoes it from its exact entry
  const bool jump = !zero_entry && !invalid && sh >= 2;
  // ... unless the two bracketing runs END on the same value: addition is
  // monotone in its start, so every run started inside the bracket ends there
  // too, the true one included -- the exit is known outright and nothing to
  // the left of this lane matters any more (the usual case: the big term
  // swamps the 2^15 ulp of the bracket)
  const bool constant = jump && __double_as_longlong(c0) == __double_as_longlong(c3);
  const bool special = jump && !constant;

  // offsets are in units of the exit ulp.  Exit offsets of the four runs
  // (|A_h| < 2^15) and entry offsets B_h = (r_h - P)/ulp_in of their starts:
  int A0 = 0;
  if (constant) A0 = exit_offset(c0);
  // exact entry: the exit is c0 itself; offset 0 wherever the approximate prefix Q is that same sum (lane 0,
  // all-zero prefixes), a few ulp for lane 1
  if (zero_entry && __double_as_longlong(c0) != __double_as_longlong(Q)) A0 = exit_offset(c0);
  // The lane's map is delta -> A_h + ((delta - B_h) >> sh), h = (p0 + delta) & 3, B_h = (r_h - P)/ulp_in the entry
  // offsets of the four starts; with U_h = A_h - (B_h >> sh) (walk_run_offset) it is (delta >> sh) + U_h.  A lane that
  // stays in its binade (sh = 0) and whose four U_h agree (no tie) is the translation delta -> delta + U_0.  So is an
  // exact-entry lane: delta is 0 on entry (nothing but exact lanes before it) and A0 on exit.  Every other valid lane
  // is a head, which the walk visits: a tie lane, a lane that crosses one binade (sh = 1; with or without a tie, the
  // hop (delta >> 1) + U_h covers both), a multi-binade run and a `constant` lane.
  const bool table = !invalid && !jump && !zero_entry;  // sh is 0 or 1
  int U0 = A0, U1 = 0, U2 = 0, U3 = 0;  // (a `constant` lane: its A0 in the table's low field, where the walk starts)
  bool translation = zero_entry;
  if (table) {
    U0 = walk_run_offset(exit_offset(c0), 0, p0, sh);
    U1 = walk_run_offset(exit_offset(c1), 1, p0, sh);
    U2 = walk_run_offset(exit_offset(c2), 2, p0, sh);
    U3 = walk_run_offset(exit_offset(c3), 3, p0, sh);
    translation = sh == 0 && U0 == U1 && U1 == U2 && U2 == U3;
  }
  // the hop table of a head with one (walk_table_pack); the fields of every other lane are never read, but for the
  // low field of a `constant` lane
  const WalkTable wt = walk_table_pack_runs(U0, U1, U2, U3);
  // A U_h beyond int16 (never seen: |U_h| is bounded by the error of Q - P, (1) above): the lane has no table and is
  // redone from its exact entry value like a multi-binade run, which is right for every lane that is not invalid.
  // (the flag is read for heads only: !wt.ok needs no `table && !translation` beside it)
  const bool redo = special || !wt.ok;
  const int t01 = wt.lo, t23 = wt.hi;
  // a register of its own, read for heads only (sh: read for table lanes only, where it is 0 or 1)
  const int meta = walk_meta(p0, sh, redo);

  // the caller's unit: the total is returned as Q_63 + delta * ulp(Q_63); Q_63
  // must not be within the bracket width of a power of two
  const double Qt = rd_lane_f64(Q, 63);
  {
    const long long qb = __double_as_longlong(Qt) & ~3ll;
    const int ea = expo_field(__longlong_as_double(qb - G4)), eb = expo_field(__longlong_as_double(qb + 3 + G4));
    if (ea != eb || ea <= 64) invalid = true;
  }
  // ---- C. compose the translations with one integer add-scan (walk_enter: a head adds nothing and nothing else
  // rides in the scanned register), then walk the heads
  const unsigned TS = wave_scan_u32(translation ? (unsigned)U0 : 0u);
  RL_STAT(0, 1);
  if (__ballot(invalid) != 0ull) {
    RL_STAT(1, 1);
    return sum_exact_fallback<S>(term);  // irregular step: literal serial sum
  }
  const unsigned long long tk3 = RL_CLK();
  unsigned long long todo = __ballot(!translation);
  RL_STAT(2, __builtin_popcountll(todo));
  {
    const unsigned long long sp = __ballot(special || (table && !translation && !wt.ok));
    (void)sp;
    RL_STAT(3, __builtin_popcountll(sp));
  }
  // the walk's state: the exact offset less the scan value (walk_enter, walk_leave).  Lane 0 enters at exactly 0 (its
  // local sum is exact, Q_0 == L_0)
  int rel = 0;
  {  // start behind the last lane whose exit is known outright
    const unsigned long long cm = __ballot(constant);
    if (cm) {
      const int qc = 63 - __builtin_clzll(cm);
      rel = walk_leave((int)(short)__builtin_amdgcn_readlane(t01, qc),  // its A0
                       (unsigned)__builtin_amdgcn_readlane((int)TS, qc));
      todo &= ~((2ull << qc) - 1ull);
    }
  }
  while (todo) {
    const int q = __builtin_ctzll(todo);
    asm("s_bitset0_b64 %0, %1" : "+s"(todo) : "s"(q));  // todo &= ~(1 << q), one instruction instead of three
    // Everything read from the lanes is independent of the offset and comes first: the head's hop table, its meta
    // and its scan value; the offset's own path is then one add in front of the hop (walk_enter), the hop
    // (walk_head_hop) and one subtraction behind it (walk_leave).  Lane 0 enters at exactly +0.0 and is never walked.
    const int tlo = __builtin_amdgcn_readlane(t01, q), thi = __builtin_amdgcn_readlane(t23, q);
    const int m = __builtin_amdgcn_readlane(meta, q);
    const unsigned Tq = (unsigned)__builtin_amdgcn_readlane((int)TS, q);
    const int din = walk_enter(rel, Tq);
    // The hop first and for every head, the rerun after it as the exception: with the two as the arms of one branch
    // the compiler routes both through a flag and three more branches per head.  (What the hop makes of a lane that
    // is redone is not used.)
    int dout = walk_head_hop(tlo, thi, m, din);  // a tie or a crossing lane: sh is 0 or 1
    if (m & WALK_META_REDO) {
      // multi-binade run: redo it from the exact entry value
      const double Pq = rd_lane_f64(P, q);
      const double uq = pow2_field(expo_field(Pq) - 52);
      double t = Pq + (double)din * uq;  // exact
      double thC = term.th, nthC = term.nth;
      term.for_each(thC, nthC, [&](int, double x) {
        t += x;
        if constexpr (!REG_TERM) asm volatile("" : "+v"(thC), "+v"(nthC));  // (not t: a wait state per term, see the chain pass)
      });
      const double v = rd_lane_f64(t, q);
      // (the true exit lies between the bracketing runs, which end in Q's binade -- else the lane were invalid)
      dout = (int)((unsigned)__double_as_longlong(v) - (unsigned)__builtin_amdgcn_readlane((int)q_lo, q));
    }
    rel = walk_leave(dout, Tq);
  }
  // the translations behind the last head
  const int delta = walk_enter(rel, (unsigned)__builtin_amdgcn_readlane((int)TS, 63));
  {
    const unsigned long long tk4 = RL_CLK();
    (void)tk0; (void)tk1; (void)tk2; (void)tk3; (void)tk4;
    RL_STAT(4, tk1 - tk0);  // scan
    RL_STAT(5, tk2 - tk1);  // four runs
    RL_STAT(6, tk3 - tk2);  // classification + translation scan
    RL_STAT(7, tk4 - tk3);  // walk
  }
  return Qt + (double)delta * pow2_field(expo_field(Qt) - 52);
}

// Targets of two waves (N > 5120) keep the sum they had: the tie-free lanes, crossing lanes among them, composed as
// maps delta -> ((delta + K) >> s) + C by a segmented scan over three registers, the walk over the tie lanes and
// the multi-binade lanes with the composite of lane q - 1 read in front of each, and the waves meeting in LDS at
// workgroup barriers.  A run of the whole GPU suite with the one-wave sum above in both places stopped in the test
// that paints N = 10,000 from two host threads at once; nothing in the sum explains that (DESIGN_NOTES 17), and until
// something does the two-wave kernels are, instruction for instruction, what they were.
template <int S, int WAVES, typename T>
RL_DEV double sum_exact_fast_segmented(const T &term, double L, WaveLink<WAVES> &lk) {
  constexpr bool REG_TERM = T::REG;
  constexpr int G4 = WALK_G4;  // half-width of the bracket [r_0, r_3] in ulps

  const unsigned long long tk0 = RL_CLK();
  // ---- A. approximate prefix from the lanes' local serial sums
  double Q = wave_scan_f64(L);                // ~ sum over lanes <= l (of this wave)
  double P = dpp_f64<DPP_WAVE_SHR1>(Q);       // ~ entry value of this lane (lane 0: +0.0)
  if constexpr (WAVES > 1) {
    // wave 1 continues where wave 0 ends: shift its prefixes by wave 0's (approximate) total
    const int lane = threadIdx.x & 63;
    const unsigned ph = lk.phase & 1u;
    if (lane == 63) lk.s->tot[ph][lk.w] = Q;
    lk.barrier();
    if (lk.w == 1) {
      const double before = lk.s->tot[ph][0];
      Q = before + Q;
      P = dpp_f64<DPP_WAVE_SHR1>(Q);
      if (lane == 0) P = before;
    }
  }
  const long long pb = __double_as_longlong(P);
  // Lanes whose entry value is known exactly need no bracket: nothing but zeros before the lane (entry
  // +0.0; lane 0 always), and lane 1 of the first wave, whose entry is lane 0's local sum -- a serial sum
  // from +0.0, i.e. the true prefix.  Their four runs start AT the entry, so the run is the true one whatever
  // it crosses (lane 1 is where two-binade jumps are most frequent), and the lane's map is the constant
  // exit offset.
  const bool zero_entry = pb == 0 || ((threadIdx.x & 63) == 1 && lk.w == 0);

  const unsigned long long tk1 = RL_CLK();
  // ---- B. four runs from r_h = h (mod 4 ulp), r_0 / r_3 bracketing the true entry
  const long long base = pb & ~3ll;
  const int p0 = (int)(pb & 3);
  double c0 = __longlong_as_double(base - G4);
  double c1 = __longlong_as_double(base + 1);
  double c2 = __longlong_as_double(base + 2);
  double c3 = __longlong_as_double(base + 3 + G4);
  if (zero_entry) { c0 = P; c1 = P; c2 = P; c3 = P; }
  const double r0 = c0, r3 = c3;
  const int e_in = expo_field(r0);
  const bool entry_ok = zero_entry || (e_in == expo_field(r3) && e_in > 64);
  int exdiff = 0;  // OR over the terms of (high word of c0) xor (high word of c3)
  double thB = term.th, nthB = term.nth;
  term.for_each(thB, nthB, [&](int, double x) {
    c0 += x;
    c1 += x;
    c2 += x;
    c3 += x;
    // exponent fields of the two bracketing runs must agree after every term:
    // exdiff |= hi(c0) ^ hi(c3), one v_bitop3_b32 per term (bits 20..30 count)
    exdiff = __builtin_amdgcn_bitop3_b32(exdiff, hi32(c0), hi32(c3), 0xF6);
    // Tie the check to its partial sums: otherwise the scheduler first runs the chains to the end and keeps all
    // partial sums alive.  A scheduling barrier, not an empty asm statement with the sums as operands: the hazard
    // recognizer treats an inline asm that names registers a double-precision instruction has just written as a
    // reader of them and puts a wait state in front -- one s_nop per term, 80 of the ~1000 issue slots of a forward
    // step (round 4, seen in the ISA).
    // (The backward pass, whose terms are recomputed here four at a time, keeps the asm statement: with the barrier
    //  alone its chain block spills 47 register pairs.)
    if constexpr (REG_TERM)
      __builtin_amdgcn_sched_barrier(0);
    else
      asm volatile("" : "+v"(exdiff), "+v"(c1), "+v"(c2), "+v"(thB), "+v"(nthB));  // (c0, c3: through exdiff)
  });
  const unsigned long long tk2 = RL_CLK();
  const int e_out = expo_field(c0);
  // exit unit = entry unit of the next lane = ulp of the binade of Q
  const int e_next = expo_field(Q);
  // An exit offset (c - Q) / ulp is asked for only where c lies in Q's binade (every other lane is invalid or walked
  // from its exact entry): there it is the difference of the two bit patterns -- one integer subtraction of the low
  // words instead of a subtraction, a multiplication and a quarter-rate conversion in double precision, six times
  // per sum (round 4).
  const unsigned q_lo = (unsigned)__double_as_longlong(Q);
  auto exit_offset = [&](double c) -> int { return (int)((unsigned)__double_as_longlong(c) - q_lo); };

  // ---- classification
  const bool same_seq = (exdiff >> 20) == 0;
  const int sh = e_out - e_in;
  bool invalid = !entry_ok || !same_seq;
  // the exit must sit in the binade the next lane (or the caller) measures in
  if (!zero_entry && e_out != e_next) invalid = true;
  if (zero_entry && expo_field(c0) != e_next) invalid = true;
  // a run that jumps two or more binades (a term much larger than the prefix)
  // does not fit the mod-4 argument: the walk redoes it from its exact entry
  const bool jump = !zero_entry && !invalid && sh >= 2;
  // ... unless the two bracketing runs END on the same value: addition is
  // monotone in its start, so every run started inside the bracket ends there
  // too, the true one included -- the exit is known outright and nothing to
  // the left of this lane matters any more (the usual case: the big term
  // swamps the 2^15 ulp of the bracket)
  const bool constant = jump && __double_as_longlong(c0) == __double_as_longlong(c3);
  const bool special = jump && !constant;

  // offsets are in units of the exit ulp.  Exit offsets of the four runs
  // (|A_h| < 2^15) and entry offsets B_h = (r_h - P)/ulp_in of their starts:
  int A0 = 0;
  if (constant) A0 = exit_offset(c0);
  // exact entry: the exit is c0 itself; offset 0 wherever the approximate prefix Q is that same sum (lane 0,
  // all-zero prefixes), a few ulp for lane 1
  if (zero_entry && __double_as_longlong(c0) != __double_as_longlong(Q)) A0 = exit_offset(c0);
  // Is the lane's map delta -> A_h + ((delta - B_h) >> sh), h = (p0 + delta) & 3, B_h = (r_h - P)/ulp_in the entry
  // offsets of the four starts, of the tie-free form ((delta + K) >> sh) + C ?   (K in {0,1} when sh = 1)
  // With U_h = A_h - (B_h >> sh) (walk_run_offset):  K = 0 iff the four U_h agree, C = U_0;  K = 1 (sh = 1 only) iff the
  // four A_h - ((B_h + 1) >> 1) = U_h - (B_h & 1) agree, and B_h & 1 = (h + p0) & 1:  U_0 = U_2, U_1 = U_3 and
  // U_0 - U_1 = 2 (p0 & 1) - 1,  C = U_0 - (p0 & 1).
  int mK = 0, mC = zero_entry ? A0 : 0;  // exact entry: delta is 0 on entry (nothing but exact lanes before), A0 on exit
  bool affine = zero_entry;
  const bool table = !invalid && !jump && !zero_entry;  // sh is 0 or 1
  int U0 = A0, U1 = 0, U2 = 0, U3 = 0;  // (a `constant` lane: its A0 in the table's low field, where the walk starts)
  if (table) {
    U0 = walk_run_offset(exit_offset(c0), 0, p0, sh);
    U1 = walk_run_offset(exit_offset(c1), 1, p0, sh);
    U2 = walk_run_offset(exit_offset(c2), 2, p0, sh);
    U3 = walk_run_offset(exit_offset(c3), 3, p0, sh);
    const int e = p0 & 1;
    const bool k0 = U0 == U1 && U1 == U2 && U2 == U3;
    const bool k1 = sh != 0 && U0 == U2 && U1 == U3 && U0 - U1 == 2 * e - 1;
    affine = k0 || k1;
    mK = k0 ? 0 : 1;
    mC = k0 ? U0 : U0 - e;
  }
  const int mS = (affine && !zero_entry) ? sh : 0;
  if (!affine) { mK = 0; mC = 0; }
  // the hop table of a tie lane (walk_table_pack); the fields of every other lane are never read, but for the low
  // field of a `constant` lane
  const WalkTable wt = walk_table_pack_runs(U0, U1, U2, U3);
  // A U_h beyond int16 (never seen: |U_h| is bounded by the error of Q - P, (1) above): the lane has no table and is
  // redone from its exact entry value like a multi-binade run, which is right for every lane that is not invalid.
  // (the flag is read for walked lanes only: !wt.ok needs no `table && !affine` beside it)
  const bool redo = special || !wt.ok;
  const int t01 = wt.lo, t23 = wt.hi;
  const int meta = (p0 << 4) | (sh << 2) | (redo ? 1 : 0);  // (sh: read for tie lanes only, where it is 0 or 1)

  // the caller's unit: the total is returned as Q_63 + delta * ulp(Q_63); Q_63
  // must not be within the bracket width of a power of two
  const double Qt = rd_lane_f64(Q, 63);
  {
    const long long qb = __double_as_longlong(Qt) & ~3ll;
    const int ea = expo_field(__longlong_as_double(qb - G4)), eb = expo_field(__longlong_as_double(qb + 3 + G4));
    if (ea != eb || ea <= 64) invalid = true;
  }
  // ---- C. compose the tie-free lanes with a segmented scan (segments end at
  // the lanes that need the walk), then walk those lanes
  // bit 6: segment head; a head carries its meta in the bits above, which no step of the scan reads
  int sK = mK, sC = mC, sS = affine ? mS : (64 | (meta << 8));
  auto combine = [&](int pK, int pC, int pS) {
    // (pK,pC,pS) = composite of the lanes further left; no-op if a head lies in between
    if (!(sS & 64)) {
      const int ps = pS & 63;
      sK = pK + ((pC + sK) << ps);
      sS = (ps + (sS & 63)) | (pS & 64);
      // sC unchanged
    }
  };
#define RL_SCAN_STEP(CTRL, RM)                                              \
  {                                                                         \
    const int pK = __builtin_amdgcn_update_dpp(0, sK, CTRL, RM, 0xf, true); \
    const int pC = __builtin_amdgcn_update_dpp(0, sC, CTRL, RM, 0xf, true); \
    const int pS = __builtin_amdgcn_update_dpp(0, sS, CTRL, RM, 0xf, true); \
    combine(pK, pC, pS);                                                    \
  }
  RL_SCAN_STEP(DPP_ROW_SHR + 1, 0xf)
  RL_SCAN_STEP(DPP_ROW_SHR + 2, 0xf)
  RL_SCAN_STEP(DPP_ROW_SHR + 4, 0xf)
  RL_SCAN_STEP(DPP_ROW_SHR + 8, 0xf)
  RL_SCAN_STEP(DPP_ROW_BCAST15, 0xa)
  RL_SCAN_STEP(DPP_ROW_BCAST31, 0xc)
#undef RL_SCAN_STEP
  // lanes not selected by a step read (0,0,0) = the identity map: harmless
  RL_STAT(0, 1);
  bool fallback = __ballot(invalid || (sS & 63) > 20) != 0ull;
  if constexpr (WAVES > 1) {  // the waves agree on the path
    if ((threadIdx.x & 63) == 0) lk.s->bad[lk.w] = fallback;
    lk.barrier();
    fallback = lk.s->bad[0] | lk.s->bad[1];
  }
  if (fallback) {
    RL_STAT(1, 1);
    return sum_exact_fallback_linked<S, WAVES>(term, lk);  // irregular step: literal serial sum
  }
  const unsigned long long tk3 = RL_CLK();
  unsigned long long todo = __ballot(!affine);
  RL_STAT(2, __builtin_popcountll(todo));
  {
    const unsigned long long sp = __ballot(special || (table && !affine && !wt.ok));
    (void)sp;
    RL_STAT(3, __builtin_popcountll(sp));
  }
  int delta = 0;  // lane 0 enters at exactly 0 (its local sum is exact, Q_0 == L_0)
  if constexpr (WAVES > 1) {
    // wave 1 walks after wave 0 and enters at wave 0's exact exit offset (same unit: the entry
    // value of its lane 0 IS wave 0's Q_63)
    if (lk.w == 1) {
      lk.barrier();
      delta = lk.s->delta;
    }
  }
  {  // start behind the last lane whose exit is known outright
    const unsigned long long cm = __ballot(constant);
    if (cm) {
      const int qc = 63 - __builtin_clzll(cm);
      delta = (int)(short)__builtin_amdgcn_readlane(t01, qc);  // its A0
      todo &= ~((2ull << qc) - 1ull);
    }
  }
  while (todo) {
    const int q = __builtin_ctzll(todo);
    todo &= todo - 1;
    // tie-free lanes since the previous walked lane (composite sits in lane q-1).  Only wave 1 can walk its lane 0
    // (virtual lane 64 enters at wave 0's total, and its run can hold a tie or a two-binade jump): nothing of this
    // wave lies before it, and delta is already its entry offset -- lane q-1 = -1 would read lane 63 (the lane select
    // keeps 6 bits), the composite of this wave's trailing lanes.  Lane 0 of wave 0 enters at exactly +0.0 and is
    // never walked.
    // Everything read from the lanes is independent of delta and comes first: the lane's hop table and meta, the
    // composite in front of it; delta's own path is then the composite map and the hop (walk_table_hop).
    const int tlo = __builtin_amdgcn_readlane(t01, q), thi = __builtin_amdgcn_readlane(t23, q);
    const int m = __builtin_amdgcn_readlane(sS, q) >> 8;
    if (WAVES == 1 || q > 0) {
      const int K = __builtin_amdgcn_readlane(sK, q - 1), C = __builtin_amdgcn_readlane(sC, q - 1);
      const int sft = __builtin_amdgcn_readlane(sS, q - 1) & 63;
      delta = ((delta + K) >> sft) + C;
    }
    if (m & 1) {
      // multi-binade run: redo it from the exact entry value
      const double Pq = rd_lane_f64(P, q);
      const double uq = pow2_field(expo_field(Pq) - 52);
      double t = Pq + (double)delta * uq;  // exact
      double thC = term.th, nthC = term.nth;
      term.for_each(thC, nthC, [&](int, double x) {
        t += x;
        if constexpr (!REG_TERM) asm volatile("" : "+v"(thC), "+v"(nthC));  // (not t: a wait state per term, see the chain pass)
      });
      const double v = rd_lane_f64(t, q);
      // (the true exit lies between the bracketing runs, which end in Q's binade -- else the lane were invalid)
      delta = (int)((unsigned)__double_as_longlong(v) - (unsigned)__builtin_amdgcn_readlane((int)q_lo, q));
    } else {
      delta = walk_table_hop(tlo, thi, m & 48, (m >> 2) & 1, delta);  // a tie lane: sh is 0 or 1
    }
  }
  {  // trailing tie-free lanes (lane 63 holds their composite; identity if it was walked)
    const int K = __builtin_amdgcn_readlane(sK, 63), C = __builtin_amdgcn_readlane(sC, 63);
    const int sft = __builtin_amdgcn_readlane(sS, 63) & 63;
    delta = ((delta + K) >> sft) + C;
  }
  {
    const unsigned long long tk4 = RL_CLK();
    (void)tk0; (void)tk1; (void)tk2; (void)tk3; (void)tk4;
    RL_STAT(4, tk1 - tk0);  // scan
    RL_STAT(5, tk2 - tk1);  // four runs
    RL_STAT(6, tk3 - tk2);  // classification + map scan
    RL_STAT(7, tk4 - tk3);  // walk
  }
  if constexpr (WAVES > 1) {
    const int lane = threadIdx.x & 63;
    if (lk.w == 0) {
      if (lane == 0) lk.s->delta = delta;
      lk.barrier();  // wave 1 starts its walk
      lk.barrier();  // ... and has finished it
    } else {
      if (lane == 0) lk.s->result = Qt + (double)delta * pow2_field(expo_field(Qt) - 52);
      lk.barrier();
    }
    const double r = lk.s->result;
    lk.barrier();  // read by everyone before the next sum's hand-over may overwrite it
    return r;
  }
  return Qt + (double)delta * pow2_field(expo_field(Qt) - 52);
}

// L = the lane's local serial sum of its terms (see sum_exact_fast)
template <int MODE, int S, int WAVES, typename T>
RL_DEV double wave_sum(const T &term, double L, WaveLink<WAVES> &lk) {
  if constexpr (MODE == 0) {
    return lanes_total(L, lk);
  } else {
    lk.phase++;
    if constexpr (MODE == 1 && WAVES == 1)
      return sum_exact_fast<S>(term, L);
    else if constexpr (MODE == 1)
      return sum_exact_fast_segmented<S, WAVES>(term, L, lk);
    else
      return sum_exact_fallback_linked<S, WAVES>(term, lk);
  }
}
// one wave per target (K2, the test hook)
template <int MODE, int S, typename T>
RL_DEV double wave_sum(const T &term, double L) {
  WaveLink<1> lk;
  return wave_sum<MODE, S, 1>(term, L, lk);
}

template <int S, typename T>
RL_DEV double local_sum(const T &term) {
  double L = 0.0, th = term.th, nth = term.nth;
  term.for_each(th, nth, [&](int, double x) { L += x; });
  return L;
}

}  // namespace rl
