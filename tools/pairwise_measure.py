#!/usr/bin/env python3
"""Measurements of rl_pairwise_trees (PairwiseCoalescence) on the GPU against the host implementation on the same
input (profiles/pairwise_coalescence.json).

    python tools/pairwise_measure.py all OUT.json [trees reps]
        for N = 1000, 5000 and 10,000 and both metrics: `trees` (256) random trees with random weights and branch
        lengths, each (N, metric) in child processes of its own under a time limit:
          - `timing N metric`: the device call (upload of the trees in batches, the kernels, the matrix back; host
            clock around the call, which ends in a device synchronise) once as warm-up and `reps` (5) times, then the
            host implementation (one thread) on the same input -- `reps` times at N = 1000, once above (a run is
            N^2 x trees updates); the two must return the same bits;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N metric`: two device calls in a process of its own, for
            the kernels' time without the copies.
        The bytes model: every tree reads and writes every off-diagonal accumulator once, 16 B per ordered pair and
        tree (the per-tree arrays, 12 N bytes -- 6 N for size -- are read by every workgroup, from L2).  The JSON is
        rewritten after every (N, metric).
    python tools/pairwise_measure.py timing N metric OUT.json [trees reps]
    python tools/pairwise_measure.py kernels N metric [trees]

The device == host assert of `timing` is a guard of the measurement (random trees, the host twin shares the device's
design).  What decides whether the device is right at these sizes is tests/test_pairwise_gpu.py:
test_device_equals_the_reference_across_the_lds_switches and ..._at_the_documented_maximum (N = 10,240, caterpillars
too, against the independent numpy reference of tests/pairwise_cases.py).
"""
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from compare_measure import random_trees  # noqa: E402

SIZES = (1000, 5000, 10000)
METRICS = ("size", "time")
HBM_PEAK = 8e12  # bytes per second, the MI355X's specification


def args(i, default):
    return type(default)(sys.argv[i]) if len(sys.argv) > i else default


def case(N, trees):
    rng = np.random.default_rng(N)
    return random_trees(N, trees, 3 * N), rng.integers(1, 2000, trees), rng.random((trees, 2 * N - 1)) * 1000.0 + 0.1


def timing():
    from relate_amd import api
    N, metric, out_fn, trees, reps = int(sys.argv[2]), sys.argv[3], sys.argv[4], args(5, 256), args(6, 5)
    P, w, bl = case(N, trees)
    bl = bl if metric == "time" else None
    dev, host, s_dev, s_host = [], [], None, None
    for rep in range(reps + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        s_dev, W = api.pairwise_trees(P, w, bl, metric, device=0)
        if rep:
            dev.append(time.perf_counter() - t0)
    for rep in range(reps if N <= 1000 else 1):
        t0 = time.perf_counter()
        s_host, _ = api.pairwise_trees(P, w, bl, metric)
        host.append(time.perf_counter() - t0)
    assert np.array_equal(s_dev.view(np.uint64), s_host.view(np.uint64)), "device and host disagree"
    off = ~np.eye(N, dtype=bool)
    json.dump({"N": N, "metric": metric, "trees": trees, "snps": int(W), "device_call_seconds": dev,
               "host_one_thread_seconds": host, "sums_equal_bit_for_bit": True,
               "mean_of_the_mean_matrix": float((s_host[off] / float(W)).mean())}, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    N, metric, trees = int(sys.argv[2]), sys.argv[3], args(4, 256)
    P, w, bl = case(N, trees)
    for _ in range(2):
        api.pairwise_trees(P, w, bl if metric == "time" else None, metric, device=0)


def everything():
    out_fn, trees, reps = sys.argv[2], args(3, 256), args(4, 5)
    res = {"what": "rl_pairwise_trees: %d random trees; device call = upload in batches + pairwise_prepare_kernel + "
                   "pairwise_accumulate_kernel + download of S, host = relate_amd/csrc/pairwise.cpp on one thread; "
                   "kernel times from rocprofv3 --kernel-trace --stats in a run of its own (2 calls), per call" % trees,
           "rows": []}
    me = os.path.abspath(__file__)
    for N in SIZES:
        for metric in METRICS:
            with tempfile.TemporaryDirectory() as tmp:
                part = os.path.join(tmp, "timing.json")
                subprocess.run(["timeout", "-k", "10", "900", sys.executable, me, "timing", str(N), metric, part,
                                str(trees), str(reps)], check=True)
                row = json.load(open(part))
                subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o",
                                "pwc", "--", sys.executable, me, "kernels", str(N), metric, str(trees)], check=True,
                               stdout=subprocess.DEVNULL)
                db = glob.glob(os.path.join(tmp, "**", "*results.db"), recursive=True)[0]
                stats = list(sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels"))
            per_call = {}
            for key in ("pairwise_prepare_kernel", "pairwise_accumulate_kernel"):
                rows = [r for r in stats if key in r[0]]
                assert len(rows) == 1, stats
                # (total_duration: microseconds, as tools/rocprof_summary.py reads it; two calls were traced)
                per_call[key] = {"launches_per_call": rows[0][1] // 2, "seconds_per_call": rows[0][2] / 2 * 1e-6}
            acc_s = per_call["pairwise_accumulate_kernel"]["seconds_per_call"]
            model = 16.0 * N * (N - 1) * trees
            dev, host = float(np.median(row["device_call_seconds"])), float(np.median(row["host_one_thread_seconds"]))
            row.update({"kernels": per_call, "device_call_seconds_median": dev, "host_seconds_median": host,
                        "host_over_device_call": host / dev,
                        "host_over_kernels": host / (acc_s + per_call["pairwise_prepare_kernel"]["seconds_per_call"]),
                        "accumulator_bytes_model": model, "per_tree_array_bytes": (12 if metric == "time" else 6) * N,
                        "accumulate_kernel_TB_per_s_of_the_model": model / acc_s / 1e12,
                        "share_of_HBM_peak_8_TB_per_s": model / acc_s / HBM_PEAK,
                        "pair_updates_per_second_device_call": float(N) * (N - 1) * trees / dev,
                        "pair_updates_per_second_host": float(N) * (N - 1) * trees / host})
            res["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
            json.dump(res, open(out_fn, "w"), indent=1)
            print(json.dumps({k: row[k] for k in ("N", "metric", "device_call_seconds_median", "host_seconds_median",
                                                  "host_over_device_call", "share_of_HBM_peak_8_TB_per_s")}), flush=True)


if __name__ == "__main__":
    {"all": everything, "timing": timing, "kernels": kernels}[sys.argv[1]]()
