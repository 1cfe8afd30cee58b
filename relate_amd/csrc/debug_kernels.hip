// debug_kernels.hip -- test hook: the wavefront sums of paint_device.h /
// exact_sum.h applied to caller-supplied arrays, so that tests can drive
// sum_exact_fast with adversarial inputs (ties, terms spanning many binades,
// totals next to powers of two) and compare with a literal left-to-right sum.
//
// The hook runs at the kernels' real geometry: an array of n terms gets
// target_waves(n) waves (two for n > 5120, meeting in LDS through one
// WaveLink), and a workgroup sums several arrays back to back on that WaveLink,
// as a step loop of K1 does.  The terms are the registers themselves (RegTerm,
// the forward passes) or (mismatch ? th : nth) * x under the EXEC masks of a
// lane-mask panel (MaskTerm, the backward passes), or those terms computed once
// into the wave's LDS stash and read back from it by every pass of the sum
// (StashTerm, K1's exact backward pass), or split three ways as that pass splits
// them: the first KS through the stash, the last R held in registers from the
// loop that computed them, the rest recomputed.
//
// This translation unit alone is compiled with the path counters of exact_sum.h
// (RL_STATS); the Makefile has no -fgpu-rdc, so the paint and repaint objects
// stay free of them.
#define RL_STATS 1
#include "paint_device.h"
#include "exact_sum.h"
#include "launch.h"
#include "common.h"

#include <vector>

namespace rl {

constexpr int SUM_STATS = 8;  // exact_sum.h RL_STAT: sums, fallbacks, walked lanes, reruns, then 4 cycle counts

enum { TERM_REG = 0, TERM_MASK = 1, TERM_STASH = 2, TERM_REGSTASH = 3 };

template <int S, int MODE, int WAVES, int KIND>
__global__ void __launch_bounds__(64 * WAVES) sum_kernel(const double *__restrict__ x, int n, int rows_per_group,
                                                         const unsigned long long *__restrict__ masks, double th,
                                                         double nth, double *__restrict__ out,
                                                         unsigned long long *__restrict__ stats) {
  __shared__ WaveLinkStorage link;
  __shared__ unsigned long long lstats[SUM_STATS];
  // the stash of each wave, as in paint_kernel (only the stashing kind has one)
  constexpr bool STASHING = KIND == TERM_STASH || KIND == TERM_REGSTASH;
  constexpr int STASH = STASHING ? stash_bytes(S) : 16;
  constexpr int R = KIND == TERM_REGSTASH ? reg_stash_terms(S) : 0;  // (the stashing kind: LDS and recomputed alone)
  __shared__ __attribute__((aligned(16))) char stash[WAVES][STASH];
  WaveLink<WAVES> lk = make_wave_link<WAVES>(&link);
  if (threadIdx.x < SUM_STATS) lstats[threadIdx.x] = 0;
  __syncthreads();
  // the kernels' layout over n terms (make_layout(n, WAVES), PaintLane::init)
  const int q = n / (64 * WAVES), rem = n % (64 * WAVES), vl = 64 * lk.w + (threadIdx.x & 63);
  const int start = vl * q + (vl < rem ? vl : rem), len = q + (vl < rem ? 1 : 0);
  for (int r = 0; r < rows_per_group; r++) {
    const size_t row = (size_t)blockIdx.x * rows_per_group + r;
    const double *xb = x + row * n;
    double a[S];
#pragma unroll
    for (int i = 0; i < S; i++) a[i] = (i < len) ? xb[start + i] : 0.0;
    double sum;
    if constexpr (STASHING) {
      // as K1's update loop: every weighted term once, its first KS into the stash, its last R into registers of
      // their own, the lane's local sum alongside
      const MaskRow mrow = (MaskRow)(masks + (row * WAVES + lk.w) * S);
      const StashPtr sp = stash_of(stash[lk.w]);
      double L = 0.0, xr[R > 0 ? R : 1];
      for_each_chunk<S, 4>(mrow, [&](int j0, const u64x4 &m) {
        double w[4];
        weighted4(w, a[j0], a[j0 + 1], a[j0 + 2], a[j0 + 3], m, th, nth);
        if (j0 < stash_terms(S)) stash_put4(sp, j0 / 4, w);
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
          L += w[jj];
          hold_term<S, R>(xr, j0 + jj, w[jj]);
        }
      });
      const StashTerm<S, S, R> t{mrow, a, th, nth, lstats, sp, xr};
      sum = wave_sum<MODE, S, WAVES>(t, L, lk);
    } else if constexpr (KIND == TERM_MASK) {
      const MaskTerm<S> t{(MaskRow)(masks + (row * WAVES + lk.w) * S), a, th, nth, lstats};
      sum = wave_sum<MODE, S, WAVES>(t, local_sum<S>(t), lk);
    } else {
      const RegTerm<S> t{a, 0.0, 0.0, lstats};
      sum = wave_sum<MODE, S, WAVES>(t, local_sum<S>(t), lk);
    }
    if (threadIdx.x == 0) out[row] = sum;
  }
  __syncthreads();
  if (threadIdx.x < SUM_STATS && lstats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], lstats[threadIdx.x]);
}

template <int S, int MODE, int WAVES>
static hipError_t launch_sum_t(const double *x, int n, int groups, int rows_per_group, const unsigned long long *masks,
                               double th, double nth, double *out, unsigned long long *stats, int kind) {
  if constexpr (MODE == 1) {  // (the stash exists for the exact order alone)
    if (kind == TERM_STASH) {
      hipLaunchKernelGGL((sum_kernel<S, MODE, WAVES, TERM_STASH>), dim3(groups), dim3(64 * WAVES), 0, nullptr, x, n,
                         rows_per_group, masks, th, nth, out, stats);
      return hipGetLastError();
    }
    if (kind == TERM_REGSTASH) {
      hipLaunchKernelGGL((sum_kernel<S, MODE, WAVES, TERM_REGSTASH>), dim3(groups), dim3(64 * WAVES), 0, nullptr, x,
                         n, rows_per_group, masks, th, nth, out, stats);
      return hipGetLastError();
    }
  }
  if (masks)
    hipLaunchKernelGGL((sum_kernel<S, MODE, WAVES, TERM_MASK>), dim3(groups), dim3(64 * WAVES), 0, nullptr, x, n,
                       rows_per_group, masks, th, nth, out, stats);
  else
    hipLaunchKernelGGL((sum_kernel<S, MODE, WAVES, TERM_REG>), dim3(groups), dim3(64 * WAVES), 0, nullptr, x, n,
                       rows_per_group, masks, th, nth, out, stats);
  return hipGetLastError();
}

template <int MODE>
static hipError_t launch_sum(int S, int waves, const double *x, int n, int groups, int rows_per_group,
                             const unsigned long long *masks, double th, double nth, double *out,
                             unsigned long long *stats, int kind) {
  return dispatch_tile(S, waves, [&](auto s, auto, auto w) {
    return launch_sum_t<s(), MODE, w()>(x, n, groups, rows_per_group, masks, th, nth, out, stats, kind);
  });
}

}  // namespace rl

extern "C" int rl_debug_wave_sum_ex(const double *x, int n, int batch, int rows_per_group, int sum_mode,
                                    const uint8_t *mismatch, double th, double nth, double *out,
                                    unsigned long long *stats8) {
  using namespace rl;
  if (!x || !out) {
    set_error("rl_debug_wave_sum_ex: null x or out");
    return RL_EINVAL;
  }
  const bool stash = (sum_mode & RL_DEBUG_SUM_STASH) != 0, regstash = (sum_mode & RL_DEBUG_SUM_REGSTASH) != 0;
  sum_mode &= ~(RL_DEBUG_SUM_STASH | RL_DEBUG_SUM_REGSTASH);
  if (stash && regstash) {
    set_error("rl_debug_wave_sum_ex: RL_DEBUG_SUM_STASH and RL_DEBUG_SUM_REGSTASH exclude each other");
    return RL_EINVAL;
  }
  if ((stash || regstash) && (sum_mode != RL_SUM_EXACT || !mismatch)) {
    set_error("rl_debug_wave_sum_ex: %s needs RL_SUM_EXACT and a mismatch array",
              stash ? "RL_DEBUG_SUM_STASH" : "RL_DEBUG_SUM_REGSTASH");
    return RL_EINVAL;
  }
  const int kind = stash ? TERM_STASH : regstash ? TERM_REGSTASH : mismatch ? TERM_MASK : TERM_REG;
  if (n < 1 || n > 2 * 80 * 64) {
    set_error("rl_debug_wave_sum_ex: n=%d outside 1..%d", n, 2 * 80 * 64);
    return RL_EINVAL;
  }
  if (rows_per_group < 1 || batch < 1 || batch % rows_per_group) {
    set_error("rl_debug_wave_sum_ex: batch=%d must be a positive multiple of rows_per_group=%d", batch,
              rows_per_group);
    return RL_EINVAL;
  }
  const int waves = target_waves(n);
  const Layout lay = make_layout(n, waves);
  const int S = choose_S(lay);  // (two waves: 48, 64 or 80, launch.h tile_has_two_waves)
  if (!S) {
    set_error("rl_debug_wave_sum_ex: no register tile for n=%d", n);
    return RL_EINVAL;
  }
  // the lane-mask panel of the mismatches (launch_lane_masks' format): per row, `waves` consecutive runs of S words;
  // bit l of word j of wave w = register j of virtual lane 64w + l holds a mismatch
  std::vector<unsigned long long> masks;
  if (mismatch) {
    masks.assign((size_t)batch * waves * S, 0ull);
    for (size_t b = 0; b < (size_t)batch; b++)
      for (int vl = 0; vl < 64 * waves; vl++) {
        const int start = vl * lay.q + (vl < lay.rem ? vl : lay.rem), len = lay.q + (vl < lay.rem ? 1 : 0);
        unsigned long long *words = &masks[(b * waves + vl / 64) * S];
        for (int j = 0; j < len; j++)
          if (mismatch[b * n + start + j]) words[j] |= 1ull << (vl & 63);
      }
  }
  DevBuf dx, dout, dmask, dstats;
  int rc;
  if ((rc = dx.alloc(sizeof(double) * (size_t)n * batch))) return rc;
  if ((rc = dout.alloc(sizeof(double) * batch))) return rc;
  if ((rc = dstats.alloc(sizeof(unsigned long long) * SUM_STATS))) return rc;
  if (mismatch && (rc = dmask.alloc(sizeof(unsigned long long) * masks.size()))) return rc;
  RL_HIP(hipMemcpy(dx.p, x, sizeof(double) * (size_t)n * batch, hipMemcpyHostToDevice));
  RL_HIP(hipMemset(dstats.p, 0, sizeof(unsigned long long) * SUM_STATS));
  if (mismatch)
    RL_HIP(hipMemcpy(dmask.p, masks.data(), sizeof(unsigned long long) * masks.size(), hipMemcpyHostToDevice));
  const unsigned long long *dm = mismatch ? dmask.as<unsigned long long>() : nullptr;
  const int groups = batch / rows_per_group;
  hipError_t e;
  switch (kernel_mode(sum_mode)) {
#define RL_ARGS S, waves, dx.as<double>(), n, groups, rows_per_group, dm, th, nth, dout.as<double>(), \
                dstats.as<unsigned long long>(), kind
    case 0: e = launch_sum<0>(RL_ARGS); break;
    case 1: e = launch_sum<1>(RL_ARGS); break;
    default: e = launch_sum<2>(RL_ARGS); break;
#undef RL_ARGS
  }
  RL_HIP(e);
  RL_HIP(hipDeviceSynchronize());
  RL_HIP(hipMemcpy(out, dout.p, sizeof(double) * batch, hipMemcpyDeviceToHost));
  if (stats8) RL_HIP(hipMemcpy(stats8, dstats.p, sizeof(unsigned long long) * SUM_STATS, hipMemcpyDeviceToHost));
  return RL_OK;
}

extern "C" int rl_debug_wave_sum(const double *x, int n, int batch, int sum_mode, double *out) {
  return rl_debug_wave_sum_ex(x, n, batch, 1, sum_mode, nullptr, 0.0, 0.0, out, nullptr);
}

// what the memory cache hands out (common.h DevBuf): the block's bytes as they come, then a fill of the caller's
extern "C" int rl_debug_alloc_peek(size_t bytes, int fill, unsigned char *out, size_t *got) {
  using namespace rl;
  if (!out || !got || fill > 255) {
    set_error("rl_debug_alloc_peek: null out or got, or fill=%d above 255", fill);
    return RL_EINVAL;
  }
  *got = 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    set_error("no usable HIP device");
    return RL_ENODEVICE;
  }
  DevBuf d;
  int rc;
  if ((rc = d.alloc(bytes))) return rc;
  if (d.bytes > bytes + bytes / 8 + 4096) {
    set_error("rl_debug_alloc_peek: a block of %zu bytes for %zu asked for: more than `out` has to hold", d.bytes, bytes);
    return RL_ENOMEM;
  }
  RL_HIP(hipMemcpy(out, d.p, d.bytes, hipMemcpyDeviceToHost));
  *got = d.bytes;
  if (fill >= 0) {
    RL_HIP(hipMemset(d.p, fill, d.bytes));
    RL_HIP(hipStreamSynchronize(nullptr));
  }
  return RL_OK;
}

// host only: how K1's exact backward pass splits the S weighted terms of tile S (exact_sum.h) -- the first *ks through
// LDS, the last *r in registers, the rest recomputed
extern "C" int rl_debug_term_split(int S, int *ks, int *r) {
  using namespace rl;
  const hipError_t e = dispatch_tile(S, 1, [&](auto s, auto, auto) {
    *ks = stash_terms(s());
    *r = reg_stash_terms(s());
    return hipSuccess;
  });
  if (e != hipSuccess) {
    set_error("rl_debug_term_split: no register tile S=%d", S);
    return RL_EINVAL;
  }
  return RL_OK;
}

// host only: the walk's hop over a tie lane (exact_sum.h), the packed table against the literal form, for every entry
// offset delta_lo .. delta_hi
extern "C" int rl_debug_walk_table(const int *A4, int p0, int sh, int delta_lo, int delta_hi, int *packable,
                                   int *out_table, int *out_reference) {
  using namespace rl;
  if (!A4 || !packable || !out_table || !out_reference) {
    set_error("rl_debug_walk_table: null argument");
    return RL_EINVAL;
  }
  if (p0 < 0 || p0 > 3 || sh < 0 || sh > 1 || delta_hi < delta_lo) {
    set_error("rl_debug_walk_table: p0=%d outside 0..3, sh=%d outside 0..1 or delta_hi=%d < delta_lo=%d", p0, sh,
              delta_hi, delta_lo);
    return RL_EINVAL;
  }
  const WalkTable t = walk_table_pack(A4[0], A4[1], A4[2], A4[3], p0, sh);
  *packable = t.ok ? 1 : 0;
  for (long long d = delta_lo; d <= delta_hi; d++) {
    out_reference[d - delta_lo] = walk_hop_reference(A4[0], A4[1], A4[2], A4[3], p0, sh, (int)d);
    out_table[d - delta_lo] = t.ok ? walk_table_hop(t.lo, t.hi, 16 * p0, sh, (int)d) : 0;
  }
  return RL_OK;
}

// host only: the walk over one wave's lanes (exact_sum.h) for per-lane records {kind, U_0, U_1, U_2, U_3, p0, sh} --
// lane by lane in the literal form, and as the kernels do it: the add-scan of the translations, then the heads
extern "C" int rl_debug_walk_lanes(const int *records, int lanes, int entry_delta, int *out_literal, int *out_scan) {
  using namespace rl;
  if (!records || !out_literal || !out_scan) {
    set_error("rl_debug_walk_lanes: null argument");
    return RL_EINVAL;
  }
  if (lanes < 1 || lanes > 64) {
    set_error("rl_debug_walk_lanes: lanes=%d outside 1..64", lanes);
    return RL_EINVAL;
  }
  for (int l = 0; l < lanes; l++) {
    const int *r = records + 7 * l;
    if (r[0] < RL_WALK_TRANSLATION || r[0] > RL_WALK_CONSTANT) {
      set_error("rl_debug_walk_lanes: lane %d: kind=%d outside 0..2", l, r[0]);
      return RL_EINVAL;
    }
    if (r[0] == RL_WALK_TABLE &&
        (r[5] < 0 || r[5] > 3 || r[6] < 0 || r[6] > 1 || !walk_table_pack_runs(r[1], r[2], r[3], r[4]).ok)) {
      set_error("rl_debug_walk_lanes: lane %d: p0=%d outside 0..3, sh=%d outside 0..1 or a U_h that is no int16", l,
                r[5], r[6]);
      return RL_EINVAL;
    }
    if (r[0] == RL_WALK_CONSTANT && (short)r[1] != r[1]) {
      set_error("rl_debug_walk_lanes: lane %d: the exit offset %d of a constant lane is no int16", l, r[1]);
      return RL_EINVAL;
    }
  }
  // the literal form: one lane after the other, a table lane as A_h + ((delta - B_h) >> sh), A_h = U_h + (B_h >> sh)
  int delta = entry_delta;
  for (int l = 0; l < lanes; l++) {
    const int *r = records + 7 * l;
    if (r[0] == RL_WALK_TRANSLATION) {
      delta = (int)((unsigned)delta + (unsigned)r[1]);
    } else if (r[0] == RL_WALK_CONSTANT) {
      delta = r[1];
    } else {
      int A[4];
      for (int h = 0; h < 4; h++) A[h] = r[1 + h] - walk_run_offset(0, h, r[5], r[6]);  // U_h + (B_h >> sh)
      delta = walk_hop_reference(A[0], A[1], A[2], A[3], r[5], r[6], delta);
    }
  }
  *out_literal = delta;
  // as sum_exact_fast: T = inclusive scan of (head ? 0 : C); start behind the last constant lane; per head
  // walk_enter, the hop through the packed table and the meta word (walk_head_hop), walk_leave; the trailing
  // translations
  unsigned T[64], run = 0;
  unsigned long long todo = 0;
  int qc = -1;
  for (int l = 0; l < lanes; l++) {
    const int *r = records + 7 * l;
    if (r[0] == RL_WALK_TRANSLATION)
      run += (unsigned)r[1];
    else
      todo |= 1ull << l;
    if (r[0] == RL_WALK_CONSTANT) qc = l;
    T[l] = run;
  }
  int rel = entry_delta;
  if (qc >= 0) {
    rel = walk_leave((int)(short)walk_table_pack_runs(records[7 * qc + 1], 0, 0, 0).lo, T[qc]);
    todo &= ~((2ull << qc) - 1ull);
  }
  while (todo) {
    const int q = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int *r = records + 7 * q;
    const WalkTable t = walk_table_pack_runs(r[1], r[2], r[3], r[4]);
    const int m = walk_meta(r[5], r[6], false);
    delta = walk_enter(rel, T[q]);
    delta = walk_head_hop(t.lo, t.hi, m, delta);
    rel = walk_leave(delta, T[q]);
  }
  *out_scan = walk_enter(rel, T[lanes - 1]);
  return RL_OK;
}
