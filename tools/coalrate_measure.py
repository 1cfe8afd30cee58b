#!/usr/bin/env python3
"""Measurements of rl_coalrate_trees (CoalescentRateForSection) on the GPU against the host implementation on the same
input (profiles/coalescence_rates.json).

    python tools/coalrate_measure.py all OUT.json [trees reps]
        for N = 1000 and 5000 with the default 31 epochs: `trees` (64) random dated trees (branch lengths exp of a
        uniform, so that the node times spread over the epochs) with random factors, each N in child processes of its
        own under a time limit:
          - `timing N`: the device call (upload of the trees in batches, the kernels, D back; host clock around the
            call, which ends in a device synchronise) once as warm-up and `reps` (5) times, then the host
            implementation (one thread) on the same input, once; the two must return the same bits;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N`: two device calls in a process of its own, for the
            kernels' time without the copies.
        The bytes model: every read-modify-write of an accumulator is 8 B; a pair i < j whose MRCA falls in epoch es
        costs one for its count (es < E-1) and min(es, E-2) + 1 for its opportunities -- counted exactly from the
        trees, and quoted next to the issue's round figure N^2/2 (mean es + 2) 8 B.  The JSON is rewritten after
        every N.
    python tools/coalrate_measure.py reference OUT.json [trees]
        where the reference's sources are (no GPU needed): its RelateCoalescentRate, built into a temporary directory
        by tools/make_golden_coalrate.py's recipe, and the host twin (rl_coalrate_anc, device -1) on the same text
        .anc / .mut at N = 1000, on the same machine; merged into OUT.json under "reference_binary".
No number is asserted anywhere.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (1000, 5000)
HBM_PEAK = 8e12  # bytes per second, the MI355X's specification
PAIRWISE_SHARE = 0.53  # pairwise_accumulate_kernel at N = 5000: the same access pattern


def args(i, default):
    return type(default)(sys.argv[i]) if len(sys.argv) > i else default


def case(N, trees):
    import coalrate_cases as cc
    rng = np.random.default_rng(N)
    parents = np.stack([cc.random_tree(N, rng) for _ in range(trees)])
    bl = np.stack([cc.dated_lengths(N, rng) for _ in range(trees)])
    return parents, bl, rng.uniform(1.0, 20000.0, trees).astype(np.float32)


def traffic(parents, bl, ep):
    """-> (read-modify-writes of the whole input, mean epoch index over pairs and trees)"""
    N, E = (parents.shape[1] + 1) // 2, len(ep)
    rmw = es_sum = 0
    for parent, b in zip(parents, bl):
        kids = np.argsort(parent, kind="stable")[1:].reshape(N - 1, 2)
        size, t = np.ones(2 * N - 1, np.int64), np.zeros(2 * N - 1, np.float32)
        for m in range(N, 2 * N - 1):
            a, c = kids[m - N]
            size[m] = size[a] + size[c]
            t[m] = np.float32(np.float64(t[a]) + b[a])
            es = int(np.searchsorted(ep[1:], t[m], side="right"))
            pairs = int(size[a] * size[c])
            rmw += pairs * ((es < E - 1) + min(es, E - 2) + 1)
            es_sum += pairs * es
    return rmw, es_sum / (len(parents) * N * (N - 1) / 2)


def timing():
    from relate_amd import api
    import coalrate_cases as cc
    N, out_fn, trees, reps = int(sys.argv[2]), sys.argv[3], args(4, 64), args(5, 5)
    P, bl, f = case(N, trees)
    ep = api.coalrate_epochs()
    dev = []
    for rep in range(reps + 1):  # the first is the warm-up
        t0 = time.perf_counter()
        d_dev = api.coalrate_trees(P, bl, f, ep, device=0)
        if rep:
            dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    d_host = api.coalrate_trees(P, bl, f, ep)
    host = [time.perf_counter() - t0]
    assert cc.same_bits(d_dev, d_host), "device and host disagree"
    rmw, mean_es = traffic(P, bl, ep)
    json.dump({"N": N, "epochs": len(ep), "trees": trees, "device_call_seconds": dev, "host_one_thread_seconds": host,
               "planes_equal_bit_for_bit": True, "read_modify_writes": rmw, "mean_epoch_index": mean_es,
               "batch_trees": api.coalrate_batch_trees(N)}, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    N, trees = int(sys.argv[2]), args(3, 64)
    P, bl, f = case(N, trees)
    for _ in range(2):
        api.coalrate_trees(P, bl, f, api.coalrate_epochs(), device=0)


def everything():
    out_fn, trees, reps = sys.argv[2], args(3, 64), args(4, 5)
    res = {"what": "rl_coalrate_trees: %d random dated trees, 31 default epochs; device call = upload in batches + "
                   "coalrate_prepare_kernel + coalrate_accumulate_kernel + download of D, host = "
                   "relate_amd/csrc/coalrate.cpp on one thread; kernel times from rocprofv3 --kernel-trace --stats in a "
                   "run of its own (2 calls), per call" % trees,
           "rows": []}
    me = os.path.abspath(__file__)
    for N in SIZES:
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "timing.json")
            subprocess.run(["timeout", "-k", "10", "900", sys.executable, me, "timing", str(N), part, str(trees),
                            str(reps)], check=True)
            row = json.load(open(part))
            subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o",
                            "cr", "--", sys.executable, me, "kernels", str(N), str(trees)], check=True,
                           stdout=subprocess.DEVNULL)
            db = glob.glob(os.path.join(tmp, "**", "*results.db"), recursive=True)[0]
            stats = list(sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels"))
        per_call = {}
        for key in ("coalrate_prepare_kernel", "coalrate_accumulate_kernel"):
            rows = [r for r in stats if key in r[0]]
            assert len(rows) == 1, stats
            # (total_duration: microseconds, as tools/rocprof_summary.py reads it; two calls were traced)
            per_call[key] = {"launches_per_call": rows[0][1] // 2, "seconds_per_call": rows[0][2] / 2 * 1e-6}
        acc_s = per_call["coalrate_accumulate_kernel"]["seconds_per_call"]
        model = 8.0 * row["read_modify_writes"]
        dev, host = float(np.median(row["device_call_seconds"])), float(np.median(row["host_one_thread_seconds"]))
        share = model / acc_s / HBM_PEAK
        row.update({"kernels": per_call, "device_call_seconds_median": dev, "host_seconds_median": host,
                    "host_over_device_call": host / dev,
                    "host_over_kernels": host / (acc_s + per_call["coalrate_prepare_kernel"]["seconds_per_call"]),
                    "accumulator_bytes_model": model,
                    "round_figure_bytes_model": N * N / 2.0 * (row["mean_epoch_index"] + 2.0) * 8.0 * trees,
                    "accumulate_kernel_TB_per_s_of_the_model": model / acc_s / 1e12,
                    "share_of_HBM_peak_8_TB_per_s": share,
                    "share_over_pairwise_accumulate_share_0.53": share / PAIRWISE_SHARE})
        res["rows"].append(row)
        os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
        json.dump(res, open(out_fn, "w"), indent=1)
        print(json.dumps({k: row[k] for k in ("N", "device_call_seconds_median", "host_seconds_median", "kernels",
                                              "mean_epoch_index", "share_of_HBM_peak_8_TB_per_s")}), flush=True)


def reference():
    from relate_amd import api
    import coalrate_cases as cc
    import make_golden_coalrate as mg
    out_fn, trees, N = sys.argv[2], args(3, 64), 1000
    P, bl, _ = case(N, trees)
    rng = np.random.default_rng(1)
    rows, pos = [], 100
    for t in range(trees):
        dist = int(rng.integers(1, 20000))
        rows.append((pos, dist, t))
        pos += dist
    res = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    with tempfile.TemporaryDirectory() as work:
        exe = mg.build_reference(work)
        open(os.path.join(work, "m.anc"), "wb").write(cc.anc_text(N, [(t, P[t], bl[t]) for t in range(trees)]))
        open(os.path.join(work, "m.mut"), "wb").write(cc.mut_text(rows))
        ref, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            subprocess.run([exe, "--mode", "CoalescentRateForSection", "-i", "m", "-o", "ref"], cwd=work, check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            ref.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            D = api.coalrate_anc(os.path.join(work, "m.anc"), os.path.join(work, "m.mut"), api.coalrate_epochs())
            host.append(time.perf_counter() - t0)
        same = cc.bin_bytes(api.coalrate_epochs(), D) == open(os.path.join(work, "ref.bin"), "rb").read()
    res["reference_binary"] = {"N": N, "trees": trees, "what": "RelateCoalescentRate --mode CoalescentRateForSection "
                               "(process start, reading the text files and writing the .bin included) and "
                               "rl_coalrate_anc on the host, one thread, same files, same machine, three runs each",
                               "reference_seconds": ref, "host_twin_seconds": host, "bin_equal_byte_for_byte": bool(same)}
    json.dump(res, open(out_fn, "w"), indent=1)
    print(json.dumps(res["reference_binary"]))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    {"all": everything, "timing": timing, "kernels": kernels, "reference": reference}[sys.argv[1]]()
