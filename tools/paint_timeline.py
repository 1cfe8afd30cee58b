#!/usr/bin/env python3
"""Resident workgroups over time of the merged Paint launch, from an experiment build (-DRL_STATS) that stamps every
workgroup's start and end with the device's 100 MHz wall clock (rl_debug_timeline):

    make -C relate_amd/csrc ../variants/librelate_amd_stats.so OBJDIR=../../build/obj_stats \\
         LIB=../variants/librelate_amd_stats.so EXTRA=-DRL_STATS
    RELATE_AMD_LIB=$PWD/relate_amd/variants/librelate_amd_stats.so RELATE_AMD_TEST_TIMELINE=1 \\
         python tools/paint_timeline.py [N L] [b,f ...]

For every segment setting (default: 1,1 = the unsegmented kernels, and the automatic rule's): the launch's span, the
slot-time the workgroups held (sum of their durations), the idle slot-time span x slots - held, and the number of
resident workgroups at tenths of the span.  slots = CUs x 4 x waves per SIMD of the tile / waves per target."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from relate_amd import api  # noqa: E402

WAVES_PER_SIMD = {8: 7, 16: 5, 32: 4, 48: 3, 64: 2, 80: 2}  # device_types.h tile_waves_per_simd


def timeline(ctx):
    n = C.c_longlong(0)
    api._check(api.lib().rl_debug_timeline(C.c_void_p(ctx._h), None, C.c_longlong(0), C.byref(n)))
    t = np.zeros((n.value, 2), np.uint64)
    api._check(api.lib().rl_debug_timeline(C.c_void_p(ctx._h), api._p(t), C.c_longlong(n.value), C.byref(n)))
    return t.astype(np.int64)


def report(name, t, ms, slots):
    t0, t1 = t[:, 0].min(), t[:, 1].max()
    span = (t1 - t0) * 1e-5  # ms
    held = (t[:, 1] - t[:, 0]).sum() * 1e-5
    print("%-8s kernel %.1f ms, %d workgroups, span %.1f ms, held %.0f slot-ms, idle %.0f slot-ms of %.0f (%.1f %%)"
          % (name, ms, len(t), span, held, span * slots - held, span * slots, 100 * (1 - held / (span * slots))))
    starts, ends = np.sort(t[:, 0]), np.sort(t[:, 1])
    at = [t0 + (t1 - t0) * i // 20 for i in range(1, 20)]
    res = [int(np.searchsorted(starts, x, "right") - np.searchsorted(ends, x, "right")) for x in at]
    print("         resident at 5 %% .. 95 %% of the span: %s" % " ".join(str(r) for r in res))
    last = (t1 - np.percentile(t[:, 1], [50, 90, 99])) * 1e-5
    print("         half / 90 %% / 99 %% of the workgroups had ended %.1f / %.1f / %.1f ms before the last" % tuple(last))


def main():
    args = sys.argv[1:]
    N, L = (int(args[0]), int(args[1])) if len(args) >= 2 and "," not in args[0] else (5000, 100000)
    settings = [tuple(int(x) for x in a.split(",")) for a in args if "," in a] or [(1, 1), (0, 0)]
    bits, r, rpos, wb = bench.make_chunk(N, L, seed=1, memory_gb=20.0)
    ctx = api.Context(0)
    ctx.set_chunk_bits(N, bits, r, rpos, wb)
    slots = 256 * 4 * WAVES_PER_SIMD[ctx.tile] // ctx.waves
    print("N = %d, L = %d, tile %d, %d waves per target, %d slots" % (N, L, ctx.tile, ctx.waves, slots))
    ctx.paint(api.RL_SUM_EXACT)
    for s in settings:
        ctx.set_paint_segments(*s)
        ms = ctx.paint(api.RL_SUM_EXACT)
        report("%d,%d" % ctx.paint_launched_segments(), timeline(ctx), ms, slots)
    ctx.close()


if __name__ == "__main__":
    main()
