// launch.h -- host-visible launchers of the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_types.h"

namespace rl {

// Register-tile sizes the kernels are instantiated for: S doubles per lane,
// with the last TAIL registers carrying a per-lane validity test.
#ifdef RL_ONLY_S
#define RL_FOR_EACH_S(X) X(RL_ONLY_S, 16)
#else
#define RL_FOR_EACH_S(X) \
  X(8, 8) X(16, 8) X(32, 16) X(48, 16) X(64, 16) X(80, 16)
#endif

// smallest instantiated S with S >= q + (rem > 0); 0 if N is too large
inline int choose_S(const Layout &lay) {
  const int need = lay.q + (lay.rem > 0 ? 1 : 0);
#define RL_FITS(s, t) \
  if (s >= need) return s;
  RL_FOR_EACH_S(RL_FITS)
#undef RL_FITS
  return 0;
}

// The tile as K1's FP64 kernels take it for a layout (paint_kernels.hip): which of a tile's instantiations runs.
//   tail   registers S - tail .. S - 1 take the backward pass's per-lane validity masks.  The tile list's value
//          (loose: 8 or 16) while q < S - 4; else 4, the backward chunk: one chunk of validity masks per step
//   live   registers 0 .. live - 1 hold a donor in some lane: S, or S - 1 when need = q + (rem > 0) is S - 1.  The
//          kernels leave a dead register out of every pass, so it costs neither instructions nor VGPRs
//   ftail  registers S - ftail .. live - 1 take the forward pass's validity compare (one v_cmp each)
//   variant  the instantiation: 0 loose (tail, S, tail) -- every layout of the tile may run it, and it is the only
//          kernel of the tile before the fit --, 1 tight (4, S, 1) for need = S, 2 tight (4, S, 4) for q >= S - 4 with
//          need <= S - 2, 3 tight minus one (4, S - 1, 2) for need = S - 1
// (q = S with rem = 0 runs variant 1: its one compare cannot fail.)
struct TileFit {
  int tail, live, ftail, variant;
};
inline TileFit tile_fit(const Layout &lay, int S, bool fit = true) {
  const int need = lay.q + (lay.rem > 0 ? 1 : 0);
  if (!fit || lay.q < S - 4) {
    int t = 0;
#define RL_TAIL_OF(s, tl) \
  if (s == S) t = tl;
    RL_FOR_EACH_S(RL_TAIL_OF)
#undef RL_TAIL_OF
    return {t, S, t, 0};
  }
  if (need == S) return {4, S, 1, 1};
  if (need == S - 1) return {4, S - 1, 2, 3};
  return {4, S, 4, 2};
}
// Two tiles of the `lanes` order keep their loose variant alone: fitted, the kernel of the merged launch comes out
// of the register allocator with 68 B of scratch per lane (S = 32 with one wave, S = 64 with two; the sensitivity
// DESIGN_NOTES.md 13 describes).  launch_paint_mode asks before it follows tile_fit, and the variants are not built.
constexpr bool tile_fit_built(int mode, int S, int waves) {
  return !(mode == 0 && ((S == 32 && waves == 1) || (S == 64 && waves == 2)));
}

// The segmented twins of the merged launch (paint_kernels.hip at -DRL_SEG) exist for the `lanes` and `exact` orders,
// for every tile, variant and wave count whose twin keeps the unsegmented kernel's scratch (none) and waves per SIMD
// (tools/kernel_resources.sh, profiles/paint_segments_kernel_resources.txt).  One does not and stays unsegmented:
// the loose variant of S = 8 in the `lanes` order comes out with 68 B of scratch per lane (its fitted variants do not).
constexpr bool paint_segments_built(int mode, int S, int waves, int variant) {
  return (mode == 0 || mode == 1) && !(mode == 0 && S == 8 && variant == 0);
}
// segments per backward / forward pass where the rule segments at all (context.cpp paint_segments_rule): the
// smallest setting that passed the A/B rule at C3 (profiles/paint_segments_ab.json)
constexpr int PAINT_SEGMENTS_AUTO_BACKWARD = 1, PAINT_SEGMENTS_AUTO_FORWARD = 8;

// the layout of all kernels: all N donors, the target keeps a slot that is pinned to +0.0;
// cut into 64*waves balanced runs (target_waves)
inline Layout make_layout(int N, int waves = 1) {
  Layout l;
  l.N = N;
  l.P = N;
  l.q = N / (64 * waves);
  l.rem = N % (64 * waves);
  return l;
}
// K1 and K2 give a target to a workgroup of two waves once one wave would need more than 80
// registers per lane (two waves per SIMD need the kernels to stay within 256 VGPRs)
inline int target_waves(int N) { return N > 80 * 64 ? 2 : 1; }
// ... which leaves 41 .. 80 registers per lane (q = N / 128 >= 40 and choose_S rounds q + 1 up to a tile of
// RL_FOR_EACH_S): the two-wave kernels exist for the tiles from 48 on.
// (RL_ONLY_S is an experiment switch of the kernel files alone, tools/build_paint_variant.sh: there the tile list is
//  the one tile and no two-wave kernel is built.  The host files are compiled without it, so choose_S keeps the full
//  list in a variant library and a tile the variant lacks comes back as hipErrorInvalidValue.)
constexpr bool tile_has_two_waves(int S) {
#ifdef RL_ONLY_S
  return false;
#else
  return S >= 48;
#endif
}
// The run-time (S, waves) as compile-time (S, TAIL, WAVES): f(integral_constant S, TAIL, WAVES) of the instantiated
// tile, hipErrorInvalidValue for any other.  The one switch over the tiles.
template <typename F>
hipError_t dispatch_tile(int S, int waves, F &&f) {
  switch (S) {
#define RL_CASE(s, t)                                                                                    \
  case s:                                                                                                \
    if (waves == 1) return f(std::integral_constant<int, s>{}, std::integral_constant<int, t>{},         \
                             std::integral_constant<int, 1>{});                                          \
    if constexpr (tile_has_two_waves(s))                                                                 \
      if (waves == 2) return f(std::integral_constant<int, s>{}, std::integral_constant<int, t>{},       \
                               std::integral_constant<int, 2>{});                                        \
    break;
    RL_FOR_EACH_S(RL_CASE)
#undef RL_CASE
  }
  return hipErrorInvalidValue;
}
// K1's launch of one direction (dir = 0 forward, 1 backward: nloc workgroups) or of both (2: 2 * nloc workgroups);
// kernel_of(integral_constant DIR) is the kernel
template <typename K>
hipError_t launch_paint_dir(K kernel_of, const PaintParams &p, int waves, int dir, hipStream_t stream) {
  const dim3 grid(dir == 2 ? 2 * p.nloc : p.nloc), block(64 * waves);
  if (dir == 2)
    hipLaunchKernelGGL(kernel_of(std::integral_constant<int, 2>{}), grid, block, 0, stream, p);
  else if (dir == 1)
    hipLaunchKernelGGL(kernel_of(std::integral_constant<int, 1>{}), grid, block, 0, stream, p);
  else
    hipLaunchKernelGGL(kernel_of(std::integral_constant<int, 0>{}), grid, block, 0, stream, p);
  return hipGetLastError();
}
// the segmented merged launch: (nb + nf) * nloc workgroups that draw their work by ticket; the control block (ticket
// counter, error word, flags) is zeroed on the stream in front of every launch
template <typename K>
hipError_t launch_paint_segments(K kernel, const PaintParams &p, int waves, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(p.seg.ctl, 0, paint_seg_ctl_bytes(p.nloc), stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)(p.seg.nb + p.seg.nf) * (unsigned)p.nloc), block(64 * waves);
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_lane_masks(const uint32_t *bits, int row_words, int L, const Layout &lay, int S, int waves,
                             unsigned long long *masks, hipStream_t stream);

// kernel summation modes (template parameter MODE of the kernels)
//   0 = lanes (RL_SUM_LANES), 1 = exact, parallel (RL_SUM_EXACT), 2 = exact, literal serial (RL_SUM_EXACT_SERIAL),
//   3 = lanes on a packed-FP32 state (RL_SUM_LANES32; K1 only, paint32_kernels.hip -- K2 then runs its `lanes` kernels)
// dir: 0 forward pass, 1 backward pass, 2 both in one launch of 2 * nloc workgroups
// fit: K1's FP64 kernels run the tile's instantiation that tile_fit picks for p.lay (1, rl_set_paint_fit's default) or
// always the loose one (0)
template <int MODE>
hipError_t launch_paint_mode(const PaintParams &p, int S, int waves, int dir, hipStream_t stream, int fit);
// ... each of whose variants is a translation unit of its own (paint_kernels.hip at -DRL_FIT=VARIANT, so that the
// build compiles them side by side), with its own launcher
template <int MODE, int VARIANT>
hipError_t launch_paint_variant(const PaintParams &p, int S, int waves, int dir, hipStream_t stream);
template <int MODE, int VARIANT>
hipError_t launch_paint_seg_variant(const PaintParams &p, int S, int waves, hipStream_t stream);
template <int MODE>
hipError_t launch_repaint_mode(const RepaintParams &p, int S, int waves, hipStream_t stream);
template <> hipError_t launch_paint_mode<0>(const PaintParams &, int, int, int, hipStream_t, int);
template <> hipError_t launch_paint_mode<1>(const PaintParams &, int, int, int, hipStream_t, int);
template <> hipError_t launch_paint_mode<2>(const PaintParams &, int, int, int, hipStream_t, int);
template <> hipError_t launch_paint_mode<3>(const PaintParams &, int, int, int, hipStream_t, int);
#define RL_DECLARE_VARIANTS(m)                                                                          \
  template <> hipError_t launch_paint_variant<m, 0>(const PaintParams &, int, int, int, hipStream_t); \
  template <> hipError_t launch_paint_variant<m, 1>(const PaintParams &, int, int, int, hipStream_t); \
  template <> hipError_t launch_paint_variant<m, 2>(const PaintParams &, int, int, int, hipStream_t); \
  template <> hipError_t launch_paint_variant<m, 3>(const PaintParams &, int, int, int, hipStream_t);
RL_DECLARE_VARIANTS(0) RL_DECLARE_VARIANTS(1) RL_DECLARE_VARIANTS(2)
#undef RL_DECLARE_VARIANTS
#define RL_DECLARE_SEG_VARIANTS(m)                                                                \
  template <> hipError_t launch_paint_seg_variant<m, 0>(const PaintParams &, int, int, hipStream_t); \
  template <> hipError_t launch_paint_seg_variant<m, 1>(const PaintParams &, int, int, hipStream_t); \
  template <> hipError_t launch_paint_seg_variant<m, 2>(const PaintParams &, int, int, hipStream_t); \
  template <> hipError_t launch_paint_seg_variant<m, 3>(const PaintParams &, int, int, hipStream_t);
RL_DECLARE_SEG_VARIANTS(0) RL_DECLARE_SEG_VARIANTS(1)
#undef RL_DECLARE_SEG_VARIANTS
template <> hipError_t launch_repaint_mode<0>(const RepaintParams &, int, int, hipStream_t);
template <> hipError_t launch_repaint_mode<1>(const RepaintParams &, int, int, hipStream_t);
template <> hipError_t launch_repaint_mode<2>(const RepaintParams &, int, int, hipStream_t);

inline int kernel_mode(int sum_mode) { return sum_mode == 0 ? 1 : (sum_mode == 1 || sum_mode == 3 ? 0 : 2); }
inline hipError_t launch_paint(const PaintParams &p, int S, int waves, int dir, hipStream_t stream, int fit = 1) {
  if (p.sum_mode == 3) return launch_paint_mode<3>(p, S, waves, dir, stream, fit);  // RL_SUM_LANES32 (one variant)
  switch (kernel_mode(p.sum_mode)) {
    case 0: return launch_paint_mode<0>(p, S, waves, dir, stream, fit);
    case 1: return launch_paint_mode<1>(p, S, waves, dir, stream, fit);
    default: return launch_paint_mode<2>(p, S, waves, dir, stream, fit);
  }
}
// K2: the forward kernel (checkpoint rows + side records of every target), then the backward kernel, one workgroup
// per target each
inline hipError_t launch_repaint(const RepaintParams &p, int S, int waves, hipStream_t stream) {
  switch (kernel_mode(p.sum_mode)) {
    case 0: return launch_repaint_mode<0>(p, S, waves, stream);
    case 1: return launch_repaint_mode<1>(p, S, waves, stream);
    default: return launch_repaint_mode<2>(p, S, waves, stream);
  }
}
// the paint file's run-length quantisation of `rows` stones of N floats, in place (panel_kernels.hip)
hipError_t launch_quantise(float *stones, int rows, int N, hipStream_t stream);
hipError_t launch_matrix(const MatrixParams &p, const Layout &lay, int S, int waves, hipStream_t stream);

}  // namespace rl
