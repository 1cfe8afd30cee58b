#!/usr/bin/env python3
"""Measurements of SubTreesForSubpopulation (rl_subtrees_trees, `Relate --mode SubTreesForSubpopulation`) on the GPU
against the host twin on the same input (profiles/subtrees.json).

    python tools/subtrees_measure.py all OUT.json [reps]
        for N = 1000, 5000 and 10,240: 1000, 200 and 100 dated trees (eight random topologies, every tree with branch
        lengths of its own) with a tenth, a half and all but one of the leaves as the subset, and 44 caterpillars with
        their two lowest leaves as the subset (one chain of N-2 steps on one lane: the worst case); each N in a child
        process of its own under a time limit:
          - the device call (upload of the trees in batches, the kernel per batch, the five outputs back; host clock
            around the call, which ends in a blocking copy) once as warm-up and `reps` (3) times, then the host twin
            (one thread) on the same input `reps` times; medians; the two must return the same bits.  The first
            subset's warm-up call minus its median is what the process pays once for the device (start-up, code
            load): `trees_to_break_even` is that over the host's gain per tree, where the host is slower at all;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N WHICH`: two device calls in a process of its own per
            subset, for the kernel's time without the copies;
          - 256, 64 and 32 of the trees as a text .anc / .mut with a .poplabels of two groups, one of interest (half
            the leaves), through `Relate --mode SubTreesForSubpopulation` under RELATE_AMD_TIMING=1 on the device and
            on the host: the process's wall clock and the split the mode prints.
        The JSON is rewritten after every N.
No number is asserted anywhere.
"""
import glob
import json
import os
import re
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

SIZES = {1000: 1000, 5000: 200, 10240: 100}    # N -> trees
TEXT_TREES = {1000: 256, 5000: 64, 10240: 32}  # N -> trees of the run through the text files
WORST_TREES = 44
SUBSETS = ("tenth", "half", "all_but_one", "caterpillar_two_lowest")
KERNEL = "subtrees_kernel"


def case(N, which):
    import subtrees_cases as sc
    rng = np.random.default_rng(N)
    if which == "caterpillar_two_lowest":
        parents = np.repeat(sc.caterpillar(N)[None], WORST_TREES, 0)
        subset = np.array([0, 1], np.int32)
    else:
        base = np.stack([sc.random_tree(N, rng) for _ in range(8)])
        parents = base[np.arange(SIZES[N]) % len(base)]
        M = {"tenth": N // 10, "half": N // 2, "all_but_one": N - 1}[which]
        subset = np.sort(np.random.default_rng(M).choice(N, M, replace=False)).astype(np.int32)
    bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
    return parents, bl, subset


def timing():
    from relate_amd import api
    import subtrees_cases as sc
    N, out_fn, reps = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    rows = {}
    for which in SUBSETS:
        parents, bl, subset = case(N, which)
        trees = len(parents)
        dev, host = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            got = api.subtrees_trees(parents, bl, subset, device=0)
            dev.append(time.perf_counter() - t0)
        for _ in range(reps):
            t0 = time.perf_counter()
            want = api.subtrees_trees(parents, bl, subset)
            host.append(time.perf_counter() - t0)
        call, twin = float(np.median(dev[1:])), float(np.median(host))
        row = dict(N=N, M=len(subset), trees=trees, batch_trees=api.subtrees_batch_trees(N),
                   tree_bytes_up=(2 * N - 1) * 12, tree_bytes_down=(2 * N - 1) * 8 + (2 * len(subset) - 1) * 16,
                   first_device_call_seconds=dev[0], device_call_seconds=dev[1:], device_call_median=call,
                   device_seconds_per_tree=call / trees, host_twin_seconds=host, host_twin_median=twin,
                   host_seconds_per_tree=twin / trees, host_over_device=twin / call, same_bits=not sc.same(got, want))
        if which == SUBSETS[0]:
            once = dev[0] - call
            row["once_per_process_seconds"] = once
            row["trees_to_break_even"] = once / ((twin - call) / trees) if twin > call else None
        rows[which] = row
    json.dump(rows, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    parents, bl, subset = case(int(sys.argv[2]), sys.argv[3])
    for _ in range(2):
        api.subtrees_trees(parents, bl, subset, device=0)


def text_case(N, n, work):
    """n of the `half` case's trees as files: two groups of diploid samples in turn, group A of interest; three SNPs
    per tree on leaf branches"""
    import coalrate_cases as cc
    import subtrees_cases as sc
    parents, bl, _ = case(N, "half")
    rng = np.random.default_rng(N + 1)
    lines, pos = [], 100
    for t in range(n):
        for _ in range(3):
            dist = int(rng.integers(1, 9000))
            lines.append("%d;%d;%d;rs%d;%d;%d;0;0;0;10;A/C;" % (len(lines), pos, dist, len(lines), t, int(rng.integers(N))))
            pos += dist
    prefix = os.path.join(work, "n%d" % N)
    open(prefix + ".anc", "wb").write(cc.anc_text(N, [(3 * k, q, b) for k, (q, b) in enumerate(zip(parents[:n], bl[:n]))]))
    open(prefix + ".mut", "wb").write(sc.mut_text(lines))
    open(prefix + ".poplabels", "wb").write(sc.poplabels_text(["AB"[k % 2] for k in range(N // 2)], "NA"))
    return prefix


def mode_run(prefix, device):
    base = os.path.basename(prefix)
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, "--mode", "SubTreesForSubpopulation", "--anc", base + ".anc", "--mut",
                        base + ".mut", "--poplabels", base + ".poplabels", "--pop_of_interest", "A", "-o", "o%d" % device,
                        "--device", str(device)], cwd=os.path.dirname(prefix), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, RELATE_AMD_TIMING="1"))
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        return dict(failed=p.returncode), p.returncode
    split = re.search(r"parsing ([\d.]+) s, subtrees \(\w+\) ([\d.]+) s, mutations mapped ([\d.]+) s, branches associated ([\d.]+) s, "
                      r"files written ([\d.]+) s", p.stderr.decode())
    names = ("parsing", "subtrees", "mutations_mapped", "branches_associated", "files_written")
    return dict(process_wall_seconds=wall, split_seconds=dict(zip(names, (float(x) for x in split.groups()))),
                summary=p.stdout.decode().strip()), 0


def died(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def all_sizes():
    out_fn, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    doc.setdefault("what", "tools/subtrees_measure.py: SubTreesForSubpopulation on one MI355X against the host twin, same inputs")
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
            rows = json.load(open(part))
            for which in SUBSETS:
                trace = os.path.join(work, "trace_" + which)
                p = subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "st",
                                    "--", sys.executable, os.path.abspath(__file__), "kernels", str(N), which], stdout=subprocess.DEVNULL)
                stop = died(p.returncode)
                if stop:
                    break
                if p.returncode == 0:
                    db = glob.glob(os.path.join(trace, "**", "*results.db"), recursive=True)[0]
                    stats = list(sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels"))
                    mine = [r for r in stats if KERNEL in r[0]]  # (total_duration: microseconds; two calls were traced)
                    secs = sum(r[2] for r in mine) / 2 * 1e-6
                    rows[which]["kernel"] = dict(launches_per_call=sum(r[1] for r in mine) // 2, seconds_per_call=secs,
                                                 seconds_per_tree=secs / rows[which]["trees"],
                                                 host_over_kernel=rows[which]["host_twin_median"] / secs if secs else None)
            if not stop:
                n = TEXT_TREES[N]
                prefix = text_case(N, n, work)
                rows["mode_end_to_end"] = dict(trees=n, anc_bytes=os.path.getsize(prefix + ".anc"))
                for name, device in (("device", 0), ("host", -1)):
                    rows["mode_end_to_end"][name], rc = mode_run(prefix, device)
                    stop = died(rc)
                    if stop:
                        break
                if not stop and "failed" not in rows["mode_end_to_end"]["device"] and "failed" not in rows["mode_end_to_end"]["host"]:
                    rows["mode_end_to_end"]["same_bytes"] = all(
                        open(os.path.join(work, "o0." + e), "rb").read() == open(os.path.join(work, "o-1." + e), "rb").read()
                        for e in ("anc", "mut", "poplabels"))
            doc["N%d" % N] = rows
        json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
        if stop:
            break


if __name__ == "__main__":
    {"all": all_sizes, "timing": timing, "kernels": kernels}[sys.argv[1]]()
