#!/usr/bin/env python3
"""Measurements of `--mode OptimizeParameters` on the GPU at config #2's shape (profiles/opt_*.json).

    python tools/opt_measure.py wall OUT.json [N L memory_GB reps]
        one chunk (synthetic block-coalescent panel, the chunk files written as MakeChunks would), one grid point
        (theta 0.001, factor 1) through rl_stage_optimize_parameters: `reps` runs in one process, the first is the
        warm-up; wall-clock by the host clock around the call (it returns after the last tree is out), trees per
        second.  The JSON is rewritten after every run.
    rocprofv3 --kernel-trace --stats -d DIR -o opt -- python tools/opt_measure.py kernels [N L memory_GB sections]
        the run to profile, in a process of its own: the first `sections` sections of the same chunk through
        rl_optimize_section (cancel_rowmin_kernel once per tree), then 200 trees of a device rl_builder from uploaded
        matrices of the same N (rowmin_penalty_kernel: one read of N^2 floats, the yardstick).
    python tools/opt_measure.py summary RESULTS.db OUT.json [N]
        per-kernel calls and average time from the rocprofv3 database, and cancel_rowmin_kernel's time per tree against
        N^2 x 8 B at the rate rowmin_penalty_kernel reaches (N^2 x 4 B over its average time) in the same run.
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chunk(N, L, mem):
    import rlutil
    budget = mem * 1e9 / 4.0 - (2.0 * N * N + 3.0 * N)
    return rlutil.synth_chunk(N, L, seed=1, budget=budget)


def args(i, default):
    return type(default)(sys.argv[i]) if len(sys.argv) > i else default


def wall():
    from relate_amd import api
    out_fn = sys.argv[2]
    N, L, mem, reps = args(3, 1000), args(4, 100000), args(5, 5.0), args(6, 3)
    ch = chunk(N, L, mem)
    res = {"what": "rl_stage_optimize_parameters, one chunk, one grid point (theta 0.001, factor 1)", "N": N, "L": L,
           "sections": int(ch.W), "trees_per_run": L, "runs": []}
    with tempfile.TemporaryDirectory() as work:
        ch.write(os.path.join(work, "out"))
        for rep in range(reps):
            t0 = time.time()
            counts = api.optimize_parameters(os.path.join(work, "out"), 0, [0.001], [1.0])
            sec = time.time() - t0
            res["runs"].append({"run": rep, "warm_up": rep == 0, "seconds": sec, "trees_per_second": L / sec,
                                "count": int(counts[0, 0])})
            json.dump(res, open(out_fn, "w"), indent=1)
            print(json.dumps(res["runs"][-1]), flush=True)


def kernels():
    import numpy as np
    from relate_amd import api
    N, L, mem, sections = args(2, 1000), args(3, 100000), args(4, 5.0), args(5, 1)
    ch = chunk(N, L, mem)
    ctx = api.Context(0)
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    t0 = time.time()
    counts = [ctx.optimize_section(s, 0.001, 1.0) for s in range(min(sections, ctx.W))]
    print("sections", counts, "%.1f s" % (time.time() - t0), flush=True)
    ctx.close()
    rng = np.random.default_rng(3)
    b = api.Builder(N, 0.001, device=0)
    for _ in range(200):
        d = (rng.random((N, N), dtype=np.float32) * np.float32(30.0)).astype(np.float32)
        np.fill_diagonal(d, 0.0)
        b.build(d)
    b.close()


def summary():
    import sqlite3
    db, out_fn, N = sys.argv[2], sys.argv[3], args(4, 1000)
    c = sqlite3.connect(db)
    rows = {name: (calls, total / calls) for name, calls, total in
            c.execute("select name,total_calls,total_duration from top_kernels")}  # (total_duration: microseconds)
    pick = lambda key: next(((k, v) for k, v in rows.items() if key in k), (None, (0, float("nan"))))
    res = {"what": "rocprofv3 --kernel-trace --stats, tools/opt_measure.py kernels, one run", "N": N, "kernels_us_per_call": {}}
    for key in ("cancel_rowmin_kernel", "rowmin_penalty_kernel", "matrix_kernel", "weave_kernel", "stage_args_kernel"):
        name, (calls, us) = pick(key)
        res["kernels_us_per_call"][key] = {"calls": calls, "average_us": us}
    _, (_, t_pen) = pick("rowmin_penalty_kernel")
    _, (_, t_can) = pick("cancel_rowmin_kernel")
    rate = 4.0 * N * N / (t_pen * 1e-6) / 1e9
    floor = 8.0 * N * N / (rate * 1e9) * 1e6
    res["rowmin_penalty_kernel_GB_per_s (N^2 x 4 B read)"] = rate
    res["cancel_rowmin_kernel_floor_us (N^2 x 8 B at that rate)"] = floor
    res["cancel_rowmin_kernel_over_floor"] = t_can / floor
    json.dump(res, open(out_fn, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    {"wall": wall, "kernels": kernels, "summary": summary}[sys.argv[1]]()
