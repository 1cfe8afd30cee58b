#!/usr/bin/env python3
"""Measurements of rl_compare_trees (CompareTopology) on the GPU against the host implementation on the same input
(profiles/compare_topology.json).

    python tools/compare_measure.py all OUT.json [pairs trees reps]
        for N = 1000, 5000 and 10,000: `pairs` (4096) pairs drawn from `trees` (256) random trees per side, each N in
        child processes of its own under a time limit:
          - `timing N`: the device call (upload of the trees, the kernel, the distances back; host clock around the
            call, which ends in a device synchronise) once as warm-up and `reps` (5) times, then the host
            implementation (one thread) `reps` times on the same input; the two must return the same integers;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N`: three device calls in a process of its own, for the
            kernel's time without the copies.
        The yardstick is the host implementation; the bytes a pair must read are 2 x (2N-1) x 4.  The JSON is
        rewritten after every N.
    python tools/compare_measure.py timing N OUT.json [pairs trees reps]
    python tools/compare_measure.py kernels N [pairs trees]
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

SIZES = (1000, 5000, 10000)


def args(i, default):
    return type(default)(sys.argv[i]) if len(sys.argv) > i else default


def random_trees(N, count, seed):
    """random joins (the next label goes to the parent of two clusters drawn at random) -> int32 [count][2N-1]"""
    rng = np.random.default_rng(seed)
    out = np.full((count, 2 * N - 1), -1, np.int32)
    for t in range(count):
        u = rng.random((N - 1, 2))
        live, parent = list(range(N)), out[t]
        for k in range(N - 1):
            n = len(live)
            i = int(u[k, 0] * n)
            live[i], live[-1] = live[-1], live[i]
            a = live.pop()
            j = int(u[k, 1] * (n - 1))
            b = live[j]
            live[j] = N + k
            parent[a] = parent[b] = N + k
    return out


def case(N, pairs, trees):
    A, B = random_trees(N, trees, 2 * N), random_trees(N, trees, 2 * N + 1)
    P = np.random.default_rng(N).integers(0, trees, (pairs, 2)).astype(np.int32)
    return A, B, P


def timing():
    from relate_amd import api
    N, out_fn, pairs, trees, reps = int(sys.argv[2]), sys.argv[3], args(4, 4096), args(5, 256), args(6, 5)
    A, B, P = case(N, pairs, trees)
    dev, host, d_dev, d_host = [], [], None, None
    for rep in range(reps + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        d_dev = api.compare_trees(A, B, P, device=0)
        if rep:
            dev.append(time.perf_counter() - t0)
    for rep in range(reps):
        t0 = time.perf_counter()
        d_host = api.compare_trees(A, B, P)
        host.append(time.perf_counter() - t0)
    assert np.array_equal(d_dev, d_host), "device and host disagree"
    res = {"N": N, "pairs": pairs, "distinct_trees_per_side": trees, "device_call_seconds": dev,
           "host_one_thread_seconds": host, "distances_equal": True,
           "mean_distance_over_full": float(d_host.mean() / (2 * (N - 2)))}
    json.dump(res, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    N, pairs, trees = int(sys.argv[2]), args(3, 4096), args(4, 256)
    A, B, P = case(N, pairs, trees)
    for _ in range(3):
        api.compare_trees(A, B, P, device=0)


def median(v):
    return float(np.median(v))


def everything():
    out_fn, pairs, trees, reps = sys.argv[2], args(3, 4096), args(4, 256), args(5, 5)
    res = {"what": "rl_compare_trees: %d pairs from %d random trees per side; device call = upload + "
                   "clade_distance_kernel + download, host = relate_amd/csrc/compare.cpp on one thread; kernel time "
                   "from rocprofv3 --kernel-trace --stats in a run of its own (3 launches)" % (pairs, trees),
           "sizes": []}
    me = os.path.abspath(__file__)
    for N in SIZES:
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "timing.json")
            subprocess.run(["timeout", "-k", "10", "600", sys.executable, me, "timing", str(N), part, str(pairs),
                            str(trees), str(reps)], check=True)
            row = json.load(open(part))
            subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "cmp",
                            "--", sys.executable, me, "kernels", str(N), str(pairs), str(trees)], check=True,
                           stdout=subprocess.DEVNULL)
            db = glob.glob(os.path.join(tmp, "**", "*results.db"), recursive=True)[0]
            rows = [r for r in sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels")
                    if "clade_distance_kernel" in r[0]]
            assert len(rows) == 1 and rows[0][1] == 3, rows
            kernel_s = rows[0][2] / rows[0][1] * 1e-6  # (total_duration: microseconds, as tools/rocprof_summary.py reads it)
        bytes_pair = 2 * (2 * N - 1) * 4
        dev, host = median(row["device_call_seconds"]), median(row["host_one_thread_seconds"])
        row.update({"kernel": rows[0][0], "kernel_seconds_per_launch": kernel_s,
                    "kernel_microseconds_per_pair": kernel_s / pairs * 1e6,
                    "device_call_seconds_median": dev, "host_seconds_median": host,
                    "device_call_microseconds_per_pair": dev / pairs * 1e6,
                    "host_microseconds_per_pair": host / pairs * 1e6,
                    "host_over_device_call": host / dev, "host_over_kernel": host / kernel_s,
                    "bytes_a_pair_must_read": bytes_pair,
                    "kernel_GB_per_s_of_those_bytes": bytes_pair * pairs / kernel_s / 1e9})
        res["sizes"].append(row)
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        json.dump(res, open(out_fn, "w"), indent=1)
        print(json.dumps({k: row[k] for k in ("N", "kernel_microseconds_per_pair", "device_call_microseconds_per_pair",
                                              "host_microseconds_per_pair", "host_over_device_call",
                                              "host_over_kernel")}), flush=True)


if __name__ == "__main__":
    {"all": everything, "timing": timing, "kernels": kernels}[sys.argv[1]]()
