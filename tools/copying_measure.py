"""CopyingMatrix on one MI355X: the reduce kernel (copying_kernels.hip) against the host twin on one thread and
against the RePaint launch of the same window, written to profiles/copying_matrix.json.

    python tools/copying_measure.py all [N ...]        # default N = 1000 5000 10000
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/copying_measure.py kernels N   # the launches alone

Per N: a random chunk of two windows, painted on the device; window 0 opened whole (one RePaint launch, its HIP-event
time), then rl_window_copying into a device-side matrix: one warm-up, the median of five (HIP events around the
launches).  Bytes model: 4 B per element of every posterior row with a weight (stride S * 64 * waves floats) plus C
read and written once, 16 B per element, as a share of the 8 TB/s HBM peak.  The host twin reduces `sample` targets'
rows (rl_window_get_topology) on one thread, scaled to all targets."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rlutil  # noqa: E402
from relate_amd import api  # noqa: E402

HBM_PEAK = 8.0e12
L, WB = 120, [0, 60, 120]


def chunk(N):
    rng = np.random.RandomState(N)
    seq = (rng.rand(L, N) < 0.15).astype(np.uint8) + ord("0")
    bp = 1000 + np.cumsum(rng.randint(1, 200, L)).astype(np.int32)
    rpos = np.concatenate([bp, [bp[-1] + 100]]).astype(np.float64) * 1e-8
    r = np.maximum(np.diff(rpos), 1e-10) * 2500
    return rlutil.Chunk(seq, r, rpos, np.array(WB, np.int32), bp)


def measure(N, reps=5, sample=8, host=True):
    ch = chunk(N)
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    win = ctx.open_window(0, None, None, api.RL_SUM_EXACT)
    rows = sum(win.rows(n) for n in range(N))
    Cm = np.zeros((N, N), np.float64)
    times = []
    for _ in range(reps + 1):  # (the first is the warm-up)
        t0 = time.perf_counter()
        win.copying(Cm)
        times.append((win.copying_ms, time.perf_counter() - t0))
    kernel_ms = float(np.median([t[0] for t in times[1:]]))
    out = dict(N=N, L=L, window_snps=WB[1], posterior_rows=rows, tile=ctx.tile, waves=ctx.waves,
               repaint_launch_ms=win.repaint_ms, reduce_kernel_ms=kernel_ms, reduce_kernel_ms_all=[t[0] for t in times],
               call_s_median=float(np.median([t[1] for t in times[1:]])))
    stride = ctx.tile * 64 * ctx.waves
    model = 4.0 * rows * stride + 16.0 * N * N
    out["bytes_model"] = model
    out["share_of_hbm_peak"] = model / (kernel_ms * 1e-3) / HBM_PEAK
    out["reduce_over_repaint"] = kernel_ms / win.repaint_ms
    if host:
        o = rlutil.oracle()
        import copying_cases as cc
        t_host, rows_host = 0.0, 0
        for n in np.linspace(0, N - 1, sample).astype(int):
            top, _ = win.topology(int(n))
            bb, be = cc.plan_bounds(o, ch, int(n))
            wt = api.copying_weights_host(cc.row_sites(ch, int(n), bb[0], be[0]), ch.rpos, WB[0], WB[1])
            t0 = time.perf_counter()
            api.copying_rows_host(top, wt)
            t_host += time.perf_counter() - t0
            rows_host += top.shape[0]
        out["host_twin_s_projected"] = t_host * rows / rows_host
        out["device_speedup_over_host_twin"] = out["host_twin_s_projected"] / (kernel_ms * 1e-3)
    win.close()
    ctx.close()
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    Ns = [int(x) for x in sys.argv[2:]] or [1000, 5000, 10000]
    if what == "kernels":
        for N in Ns:
            print(json.dumps(measure(N, reps=5, host=False)))
    else:
        res = dict(tool="tools/copying_measure.py all", hbm_peak_bytes_per_s=HBM_PEAK, cases=[measure(N) for N in Ns])
        with open(os.path.join(ROOT, "profiles", "copying_matrix.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
