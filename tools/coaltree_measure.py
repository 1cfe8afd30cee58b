#!/usr/bin/env python3
"""Measurements of CoalRateForTree (rl_coaltree_trees, `Relate --mode CoalRateForTree`) on the GPU against the host
twin on the same input (profiles/coaltree.json).

    python tools/coaltree_measure.py all OUT.json [reps]
        for N = 1000, 5000 and 10,240: 2500, 2200 and 2100 dated trees (eight random topologies, every tree with
        branch lengths of its own), the reference's blocks of 1000 -- three blocks each --, each N in a child process
        of its own under a time limit:
          - the device call (upload of the trees in batches, both kernels per batch, the accumulators back; host
            clock around the call, which ends in a blocking copy) once as warm-up and `reps` (3) times, then the host
            twin (one thread) on the same input `reps` times; medians; the two must return the same bits.  The
            warm-up call minus the median is what the process pays once for the device (start-up, code load):
            `trees_to_break_even` is that over the host's gain per tree;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N`: two device calls in a process of its own, for the
            two kernels' times without the copies;
          - 256, 64 and 32 of the trees as a text .anc / .mut through `Relate --mode CoalRateForTree` on the device
            and on the host: the process's wall clock, reading the text included.
        The JSON is rewritten after every N.
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
CLI = os.path.join(ROOT, "relate_amd", "Relate")

SIZES = {1000: 2500, 5000: 2200, 10240: 2100}  # N -> trees
TEXT_TREES = {1000: 256, 5000: 64, 10240: 32}  # N -> trees of the run through the text files
KERNELS = ("coaltree_terms_kernel", "coaltree_chains_kernel")


def case(N, trees):
    import coaltree_cases as ct
    rng = np.random.default_rng(N)
    base = np.stack([ct.random_tree(N, rng) for _ in range(8)])
    parents = base[np.arange(trees) % len(base)]
    bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
    factors = (rng.integers(1, 20000, trees).astype(np.float32) / np.float32(2))
    return parents, bl, factors


def same_bits(a, b):
    return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def timing():
    from relate_amd import api
    import coaltree_cases as ct
    N, out_fn, reps = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    trees = SIZES[N]
    parents, bl, factors = case(N, trees)
    ep = ct.default_epochs()
    dev, host = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got = api.coaltree_trees(parents, bl, factors, ep, device=0)
        dev.append(time.perf_counter() - t0)
    for _ in range(reps):
        t0 = time.perf_counter()
        want = api.coaltree_trees(parents, bl, factors, ep)
        host.append(time.perf_counter() - t0)
    call, twin = float(np.median(dev[1:])), float(np.median(host))
    once = dev[0] - call
    row = dict(N=N, trees=trees, blocks=len(got[0]), epochs=len(ep), batch_trees=api.coaltree_batch_trees(N),
               tree_bytes_up=(2 * N - 1) * 12 + 4, bytes_kept_on_device_per_tree=(N - 1) * 8 + len(ep) * 16,
               first_device_call_seconds=dev[0], device_call_seconds=dev[1:], device_call_median=call,
               device_seconds_per_tree=call / trees, host_twin_seconds=host, host_twin_median=twin,
               host_seconds_per_tree=twin / trees, host_over_device=twin / call,
               once_per_process_seconds=once, trees_to_break_even=once / ((twin - call) / trees) if twin > call else None,
               same_bits=same_bits(got[0], want[0]) and same_bits(got[1], want[1]))
    json.dump(row, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    import coaltree_cases as ct
    N = int(sys.argv[2])
    parents, bl, factors = case(N, SIZES[N])
    for _ in range(2):
        api.coaltree_trees(parents, bl, factors, ct.default_epochs(), device=0)


def mode_run(prefix, device):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, "--mode", "CoalRateForTree", "-i", os.path.basename(prefix), "-o",
                        "o%d" % device, "--device", str(device)], cwd=os.path.dirname(prefix), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    return (dict(process_wall_seconds=time.perf_counter() - t0) if p.returncode == 0 else dict(failed=p.returncode)), p.returncode


def died(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def all_sizes():
    import coalrate_cases as cc
    import coaltree_cases as ct
    out_fn, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    doc.setdefault("what", "tools/coaltree_measure.py: CoalRateForTree on one MI355X against the host twin, same inputs")
    stop = False
    for N in SIZES:
        with tempfile.TemporaryDirectory() as work:
            part = os.path.join(work, "part.json")
            p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "timing", str(N), part, str(reps)])
            if p.returncode != 0:
                doc["N%d" % N] = dict(failed=p.returncode)
                json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
                if died(p.returncode):
                    break  # nothing more is started on the device
                continue
            row = json.load(open(part))
            p = subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(work, "trace"), "-o", "ct",
                                "--", sys.executable, os.path.abspath(__file__), "kernels", str(N)], stdout=subprocess.DEVNULL)
            stop = died(p.returncode)
            if p.returncode == 0:
                db = glob.glob(os.path.join(work, "trace", "**", "*results.db"), recursive=True)[0]
                stats = list(sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels"))
                row["kernels"] = {}
                for k in KERNELS:  # (total_duration: microseconds, as tools/mutrate_measure.py reads it; two calls were traced)
                    mine = [r for r in stats if k in r[0]]
                    secs = sum(r[2] for r in mine) / 2 * 1e-6
                    row["kernels"][k] = dict(launches_per_call=sum(r[1] for r in mine) // 2, seconds_per_call=secs,
                                             seconds_per_tree=secs / row["trees"])
                both = sum(v["seconds_per_call"] for v in row["kernels"].values())
                row["kernels"]["share_of_the_chains"] = row["kernels"][KERNELS[1]]["seconds_per_call"] / both
                row["kernels"]["host_over_both_kernels"] = row["host_twin_median"] / both
            if not stop:
                n = TEXT_TREES[N]
                parents, bl, _ = case(N, n)
                prefix = os.path.join(work, "n%d" % N)
                open(prefix + ".anc", "wb").write(cc.anc_text(N, [(10 * k, q, b) for k, (q, b) in enumerate(zip(parents, bl))]))
                open(prefix + ".mut", "wb").write(cc.mut_text(ct.mut_rows(n, np.random.default_rng(N + 1))))
                row["mode_end_to_end"] = dict(trees=n, anc_bytes=os.path.getsize(prefix + ".anc"))
                for name, device in (("device", 0), ("host", -1)):
                    row["mode_end_to_end"][name], rc = mode_run(prefix, device)
                    stop = died(rc)
                    if stop:
                        break
                if not stop:
                    row["mode_end_to_end"]["same_bytes"] = open(os.path.join(work, "o0.coal"), "rb").read() == \
                        open(os.path.join(work, "o-1.coal"), "rb").read()
            doc["N%d" % N] = row
        json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
        if stop:
            break


if __name__ == "__main__":
    {"all": all_sizes, "timing": timing, "kernels": kernels}[sys.argv[1]]()
