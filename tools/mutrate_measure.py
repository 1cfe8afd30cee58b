#!/usr/bin/env python3
"""Measurements of AvgMutationRate (rl_mutrate_trees, rl_mutrate_anc) on the GPU against the host twin on the same
input (profiles/mutrate_through_time.json).

    python tools/mutrate_measure.py all OUT.json [reps]
        for N = 1000, 5000 and 10,240: random dated trees (frequency_cases.clock_lengths) -- 256, 64 and 32 trees --,
        each N in a child process of its own under a time limit:
          - the device call (upload of the trees in batches, the kernel, E doubles per tree back; host clock around
            the call, which ends in a blocking copy) once as warm-up and `reps` (5) times, then the host twin (one
            thread) on the same input, once; the two must return the same bits.  Three sets of boundaries:
              spread    31 boundaries over the trees' times: the lanes share the intervals unevenly, as in the mode
              one_lane  0 and one boundary above every root: ONE lane adds all N-1 intervals one by one -- the worst the
                        one-lane-per-epoch walk can do
              no_walk   0 and one boundary below every node time: the first interval crosses it and nothing is
                        walked -- what the kernel costs without the walk (the passes and the sort)
          - rocprofv3 --kernel-trace --stats -- ... `kernels N`: two device calls per set of boundaries in a process
            of its own, for the kernel's time without the copies;
          - the same trees as a text .anc / .mut (5 SNPs per tree) through `Relate --mode AvgMutationRate` with
            RELATE_AMD_TIMING=1 on the device and on the host: the split of the mode into reading the text, the trees'
            lengths and the SNP loop.
        The JSON is rewritten after every N.
    python tools/mutrate_measure.py reference OUT.json
        where the reference's sources are (no GPU needed): its RelateMutationRate --mode Avg, built into a temporary
        directory by tools/make_golden_mutrate.py's recipe, and the host twin's mode on the same text files at N =
        1000, on the same machine; merged into OUT.json under "reference_binary".
No number is asserted anywhere.
"""
import glob
import json
import os
import platform
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

SIZES = {1000: 256, 5000: 64, 10240: 32}  # N -> trees
SNPS_PER_TREE = 5
BINS = "1.2,5.4,0.15"  # --bins of the mode's runs: 31 boundaries over the times of clock_lengths with 28 years per generation


def case(N, trees):
    import mutrate_cases as mc
    rng = np.random.default_rng(N)
    parents = np.stack([mc.random_tree(N, rng) for _ in range(trees)])
    bl = np.stack([mc.clock_lengths(p, rng) for p in parents])
    return parents, bl


def boundaries():
    return dict(spread=np.concatenate(([0.0], np.exp(np.linspace(2.5, 12.5, 30)))), one_lane=np.array([0.0, 1e30]),
                no_walk=np.array([0.0, 1e-3]))


def write_text(work, N, parents, bl):
    import coalrate_cases as cc
    import mutrate_cases as mc
    prefix = os.path.join(work, "n%d" % N)
    rng = np.random.default_rng(N + 1)
    trees = [(10 * k, p, b) for k, (p, b) in enumerate(zip(parents, bl))]
    open(prefix + ".anc", "wb").write(cc.anc_text(N, trees))
    open(prefix + ".mut", "wb").write(mc.mut_text(mc.branch_rows(N, trees, rng, per_tree=SNPS_PER_TREE, big_dist_at=-1)))
    return prefix


def model(N):
    """bytes of LDS a workgroup holds and the compare-exchanges of its sort network"""
    ni = N - 1
    P = 1
    while P < ni:
        P *= 2
    stages = (P.bit_length() - 1) * P.bit_length() // 2
    return dict(lds_bytes=8 * ni, sort_slots=P, sort_stages=stages, compare_exchange_slots=stages * P // 2,
                tree_bytes_up=(2 * N - 1) * 12, serial_adds_of_one_lane_at_most=ni)


def mode_split(prefix, device):
    """`Relate --mode AvgMutationRate` with RELATE_AMD_TIMING=1 -> wall clock and the library's own split"""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, "--mode", "AvgMutationRate", "-i", os.path.basename(prefix), "-o",
                        "o%d" % device, "--device", str(device), "--bins", BINS], cwd=os.path.dirname(prefix),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, RELATE_AMD_TIMING="1"))
    wall = time.perf_counter() - t0
    m = re.search(r"\[mutrate\] .*: ([0-9.]+) s; SNP loop \((\d+) mapped\): ([0-9.]+) s; reading the text and the rest: ([0-9.]+) s", p.stderr.decode())
    if p.returncode != 0 or not m:
        return dict(failed=p.returncode), p.returncode
    return dict(process_wall_seconds=wall, trees_seconds=float(m.group(1)), mapped_snps=int(m.group(2)),
                snp_loop_seconds=float(m.group(3)), text_and_rest_seconds=float(m.group(4))), 0


def timing():
    from relate_amd import api
    N, out_fn, reps = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    trees = SIZES[N]
    parents, bl = case(N, trees)
    row = dict(N=N, trees=trees, model=model(N))
    for name, ep in boundaries().items():
        dev = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            got = api.mutrate_trees(parents, bl, ep, device=0)
            dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = api.mutrate_trees(parents, bl, ep)
        host = time.perf_counter() - t0
        call = float(np.median(dev[1:]))
        row[name] = dict(epochs=len(ep), device_call_seconds=dev[1:], device_call_median=call, device_seconds_per_tree=call / trees,
                         host_twin_seconds=host, host_seconds_per_tree=host / trees, host_over_device=host / call,
                         same_bits=bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))))
    json.dump(row, open(out_fn, "w"))


def kernels():
    from relate_amd import api
    N, name = int(sys.argv[2]), sys.argv[3]
    parents, bl = case(N, SIZES[N])
    for _ in range(2):
        api.mutrate_trees(parents, bl, boundaries()[name], device=0)


def died(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def all_sizes():
    out_fn, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    doc.setdefault("what", "tools/mutrate_measure.py: AvgMutationRate on one MI355X against the host twin, same inputs")
    stop = False
    for N in SIZES:
        with tempfile.TemporaryDirectory() as work:
            part = os.path.join(work, "part.json")
            p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "timing", str(N), part, str(reps)])
            if p.returncode != 0:
                doc["N%d" % N] = dict(failed=p.returncode)
                json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
                if died(p.returncode):
                    break  # nothing more is started on the device
                continue
            row = json.load(open(part))
            for name in boundaries():
                p = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(work, name), "-o", "mr",
                                    "--", sys.executable, os.path.abspath(__file__), "kernels", str(N), name], stdout=subprocess.DEVNULL)
                if p.returncode == 0:
                    db = glob.glob(os.path.join(work, name, "**", "*results.db"), recursive=True)[0]
                    stats = [r for r in sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels")
                             if "mutrate_kernel" in r[0]]
                    # (total_duration: microseconds, as tools/frequency_measure.py reads it; two calls were traced)
                    secs = sum(r[2] for r in stats) / 2 * 1e-6
                    row[name]["kernel"] = dict(launches_per_call=sum(r[1] for r in stats) // 2, seconds_per_call=secs,
                                               seconds_per_tree=secs / row["trees"],
                                               host_over_kernel=row[name]["host_twin_seconds"] / secs)
                stop = died(p.returncode)
                if stop:
                    break
            if not stop:
                prefix = write_text(work, N, *case(N, SIZES[N]))
                row["mode_end_to_end"] = dict(anc_bytes=os.path.getsize(prefix + ".anc"))
                for name, device in (("device", 0), ("host", -1)):
                    row["mode_end_to_end"][name], rc = mode_split(prefix, device)
                    stop = died(rc)
                    if stop:
                        break
                if not stop:
                    row["mode_end_to_end"]["same_bytes"] = open(os.path.join(work, "o0_avg.rate"), "rb").read() == \
                        open(os.path.join(work, "o-1_avg.rate"), "rb").read()
            doc["N%d" % N] = row
        json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
        if stop:
            break


def reference():
    import make_golden_mutrate as mg
    out_fn = sys.argv[2]
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    N = 1000
    with tempfile.TemporaryDirectory() as work:
        exes = mg.build_reference(work)
        prefix = write_text(work, N, *case(N, SIZES[N]))
        t0 = time.perf_counter()
        subprocess.run([exes[0], "--mode", "Avg", "-i", prefix, "-o", prefix + "_ref", "--bins", BINS], check=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        ref = time.perf_counter() - t0
        host, _ = mode_split(prefix, -1)
        same = open(prefix + "_ref_avg.rate", "rb").read() == open(os.path.join(work, "o-1_avg.rate"), "rb").read()
    doc["reference_binary"] = dict(N=N, trees=SIZES[N], snps_per_tree=SNPS_PER_TREE,
                                   machine="%s, %d CPUs, no GPU" % (platform.processor() or platform.machine(), os.cpu_count()),
                                   reference_mode_seconds=ref, host_twin_mode=host, same_bytes=bool(same),
                                   note="both on this CPU machine, one thread each; not comparable with the MI355X machine's numbers")
    json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    {"all": all_sizes, "timing": timing, "kernels": kernels, "reference": reference}[sys.argv[1]]()
