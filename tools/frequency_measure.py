#!/usr/bin/env python3
"""Measurements of Frequency (rl_frequency_trees, rl_frequency_anc) on the GPU against the host walk on the same input
(profiles/frequency_through_time.json).

    python tools/frequency_measure.py all OUT.json [reps]
        for N = 1000, 5000 and 10,240 with the default 31 epochs: random dated trees (frequency_cases.clock_lengths: tie-free float times at any N)
        with 5 SNPs per tree on random branches -- 256, 64 and 32 trees --, each N in a child process of its own under a
        time limit:
          - the device call (upload of the trees in batches, the kernel, the rows back; host clock around the call,
            which ends in a blocking copy) once as warm-up and `reps` (5) times, then the host walk (one thread) on the
            same input, once; the two must return the same integers;
          - rocprofv3 --kernel-trace --stats -- ... `kernels N`: two device calls in a process of its own, for the
            kernel's time without the copies (launches = batches);
          - the same trees as a text .anc / .mut through rl_frequency_anc on the device and on the host: the wall clock
            of the mode end to end; what it takes beyond the call on arrays is reading the text and writing the rows.
        The JSON is rewritten after every N.
    python tools/frequency_measure.py reference OUT.json
        where the reference's sources are (no GPU needed): its RelateSelection --mode Frequency, built into a temporary
        directory by tools/make_golden_selection.py's recipe, and the host walk (rl_frequency_anc, device -1) on the
        same text files at N = 1000, on the same machine; merged into OUT.json under "reference_binary".
No number is asserted anywhere.
"""
import glob
import json
import os
import platform
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {1000: 256, 5000: 64, 10240: 32}  # N -> trees
SNPS_PER_TREE = 5


def case(N, trees):
    import frequency_cases as fc
    rng = np.random.default_rng(N)
    parents = np.stack([fc.random_tree(N, rng) for _ in range(trees)])
    bl = np.stack([fc.clock_lengths(p, rng) for p in parents])  # tie-free: no tree goes back to the host walk
    st = np.repeat(np.arange(trees), SNPS_PER_TREE).astype(np.int32)
    sb = rng.integers(0, 2 * N - 2, len(st)).astype(np.int32)
    return parents, bl, st, sb


def write_text(work, N, parents, bl, st, sb):
    import coalrate_cases as cc
    import frequency_cases as fc
    prefix = os.path.join(work, "n%d" % N)
    open(prefix + ".anc", "wb").write(cc.anc_text(N, [(10 * k, p, b) for k, (p, b) in enumerate(zip(parents, bl))]))
    open(prefix + ".mut", "wb").write(fc.mut_text([(100 + 10 * k, 10, int(t), [int(b)], 0, 0.0) for k, (t, b) in enumerate(zip(st, sb))]))
    return prefix


def model(N, E=31):
    """bytes of LDS a workgroup holds and the compare-exchanges of its sort"""
    ni = N - 1
    P = 1
    while P < ni:
        P *= 2
    stages = (P.bit_length() - 1) * P.bit_length() // 2
    return dict(lds_bytes=12 * ni + 4 * ((ni + 31) // 32), sort_slots=P, sort_stages=stages, compare_exchanges=stages * P // 2,
                tree_bytes_up=(2 * N - 1) * 12, row_bytes_back=(2 * E + 2) * 4)


def timing():
    from relate_amd import api
    N, out_fn, reps = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    trees = SIZES[N]
    parents, bl, st, sb = case(N, trees)
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.5, 12.5, 30)))).astype(np.float32)  # 31 boundaries over the trees' times
    dev = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got = api.frequency_trees(parents, bl, st, sb, ep, device=0)
        dev.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = api.frequency_trees(parents, bl, st, sb, ep)
    host = time.perf_counter() - t0
    same = all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == 0
    files = {}
    with tempfile.TemporaryDirectory() as work:
        prefix = write_text(work, N, parents, bl, st, sb)
        for name, device in (("device", 0), ("host", None)):
            t0 = time.perf_counter()
            api.frequency_anc(prefix + ".anc", prefix + ".mut", ep, prefix + ".freq", prefix + ".lin", device)
            files[name] = time.perf_counter() - t0
        files["anc_bytes"] = os.path.getsize(prefix + ".anc")
    call = float(np.median(dev[1:]))
    json.dump(dict(N=N, trees=trees, snps=len(st), epochs=len(ep), device_call_seconds=dev[1:], device_call_median=call,
                   device_seconds_per_tree=call / trees, device_seconds_per_snp=call / len(st), host_walk_seconds=host,
                   host_seconds_per_tree=host / trees, host_over_device=host / call, same_integers=bool(same),
                   mode_end_to_end_seconds=files,
                   text_share_of_the_device_mode=max(0.0, 1.0 - call / files["device"]), model=model(N)),
              open(out_fn, "w"))


def kernels():
    from relate_amd import api
    N = int(sys.argv[2])
    parents, bl, st, sb = case(N, SIZES[N])
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.5, 12.5, 30)))).astype(np.float32)
    for _ in range(2):
        api.frequency_trees(parents, bl, st, sb, ep, device=0)


def all_sizes():
    out_fn, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    doc.setdefault("what", "tools/frequency_measure.py: Frequency on one MI355X against the host walk, same inputs")
    for N in SIZES:
        with tempfile.TemporaryDirectory() as work:
            part = os.path.join(work, "part.json")
            p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "timing", str(N), part, str(reps)])
            if p.returncode != 0:
                doc["N%d" % N] = dict(failed=p.returncode)
                json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
                if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                    break  # nothing more is started on the device
                continue
            row = json.load(open(part))
            p = subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", "fq", "--",
                                sys.executable, os.path.abspath(__file__), "kernels", str(N)], stdout=subprocess.DEVNULL)
            if p.returncode == 0:
                db = glob.glob(os.path.join(work, "**", "*results.db"), recursive=True)[0]
                stats = [r for r in sqlite3.connect(db).execute("select name,total_calls,total_duration from top_kernels")
                         if "frequency_kernel" in r[0]]
                # (total_duration: microseconds, as tools/coalrate_measure.py reads it; two calls were traced)
                secs = sum(r[2] for r in stats) / 2 * 1e-6
                row["kernel"] = dict(launches_per_call=sum(r[1] for r in stats) // 2, seconds_per_call=secs,
                                     seconds_per_tree=secs / row["trees"], seconds_per_snp=secs / row["snps"],
                                     host_over_kernel=row["host_walk_seconds"] / secs)
            doc["N%d" % N] = row
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
                break
        json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)


def reference():
    import make_golden_selection as mg
    from relate_amd import api
    out_fn = sys.argv[2]
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    N = 1000
    parents, bl, st, sb = case(N, SIZES[N])
    with tempfile.TemporaryDirectory() as work:
        exe = mg.build_reference(work)
        prefix = write_text(work, N, parents, bl, st, sb)
        t0 = time.perf_counter()
        subprocess.run([exe, "--mode", "Frequency", "-i", prefix, "-o", prefix + "_ref", "--bins", "1.2,5.4,0.15"], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        ref = time.perf_counter() - t0
        t0 = time.perf_counter()
        api.frequency_anc(prefix + ".anc", prefix + ".mut", api.coalrate_epochs(28.0, "1.2,5.4,0.15"), prefix + ".freq", prefix + ".lin")
        host = time.perf_counter() - t0
        same = all(open(prefix + e, "rb").read() == open(prefix + "_ref" + e, "rb").read() for e in (".freq", ".lin"))
    doc["reference_binary"] = dict(N=N, trees=SIZES[N], snps=len(st), machine="%s, %d CPUs, no GPU" % (platform.processor() or platform.machine(), os.cpu_count()),
                                   reference_mode_seconds=ref, host_walk_mode_seconds=host, same_bytes=bool(same),
                                   note="both on this CPU machine, one thread each; not comparable with the MI355X machine's numbers")
    json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    {"all": all_sizes, "timing": timing, "kernels": kernels, "reference": reference}[sys.argv[1]]()
