#!/usr/bin/env python3
"""Measurements of MutationRateWithContext (rl_mutctx_trees, rl_mutctx_anc) on the GPU against the host twin on the
same input (profiles/mutctx.json).

    python tools/mutctx_measure.py all OUT.json [reps] [largest L]
        for L = 10^4, 10^5 and 10^6 qualifying SNPs on 64 random dated trees at N = 1000 (one batch), E = 31, each L
        in a child process of its own under a time limit:
          - rl_mutctx_trees on the device once as warm-up and `reps` (3) times -- the host's clock around the call,
            and the library's own split of it: the tree arrays up with the per-tree kernel | the SNPs' trees and
            counts up (384 bytes per SNP) | the chains kernel alone (the device idle on both sides of each) --, then
            the host twin (one thread) on the same input, once; the two must return the same bits.  The rows of counts
            are as the mode makes them: about 20 bases between two midpoints, so most of the 96 entries are 0;
          - the same trees as a text .anc with a .mut of L SNPs, an ancestor and a mask through `Relate --mode
            MutationRateWithContext` with RELATE_AMD_TIMING=1 on the device and with --device -1: the split of the
            mode into counting the bases, the trees and SNPs, and reading the .anc.
        The JSON is rewritten after every L.
No number is asserted anywhere.
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
N, TREES = 1000, 64
BINS = "1.2,5.4,0.15"  # 31 boundaries over the times of clock_lengths with 28 years per generation


def trees_of():
    import mutrate_cases as mc
    rng = np.random.default_rng(N)
    parents = np.stack([mc.random_tree(N, rng) for _ in range(TREES)])
    bl = np.stack([mc.clock_lengths(p, rng) for p in parents])
    return parents, bl


def snps_of(L):
    rng = np.random.default_rng(L)
    tree = (np.arange(L, dtype=np.int64) * TREES // L).astype(np.int32)
    counts = np.zeros((L, 96), np.uint32)
    for _ in range(12):  # twelve of the 96 categories hold a few bases each
        counts[np.arange(L), rng.integers(0, 96, L)] += rng.integers(1, 4, L).astype(np.uint32)
    return tree, counts


def timing():
    from relate_amd import api
    L, out_fn, reps = int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    parents, bl = trees_of()
    tree, counts = snps_of(L)
    ep = api.mutrate_epochs(28.0, BINS)
    dev, parts = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got, _, seconds = api.mutctx_trees(parents, bl, tree, counts, ep, device=0, details=True)
        dev.append(time.perf_counter() - t0)
        parts.append(seconds.tolist())
    t0 = time.perf_counter()
    want = api.mutctx_trees(parents, bl, tree, counts, ep)
    host = time.perf_counter() - t0
    call = float(np.median(dev[1:]))
    split = np.median(np.array(parts[1:]), axis=0)
    row = dict(L=L, N=N, trees=TREES, epochs=len(ep), multiply_adds=L * len(ep) * 96, count_bytes_up=L * 384,
               device_call_seconds=dev[1:], device_call_median=call,
               trees_and_per_tree_kernel_seconds=float(split[0]), count_copies_seconds=float(split[1]),
               chains_kernel_seconds=float(split[2]), copies_share_of_call=float(split[1] / call),
               chains_share_of_call=float(split[2] / call), host_twin_seconds=host, host_over_device_call=host / call,
               host_over_chains_kernel=host / float(split[2]),
               same_bits=bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))))
    json.dump(row, open(out_fn, "w"))


def write_text(work, L):
    """the trees as a text .anc, a .mut of L qualifying SNPs on random branches, an ancestor and a mask"""
    import coalrate_cases as cc
    import mutctx_cases as xc
    from frequency_cases import MUT_HEAD, max_times
    parents, bl = trees_of()
    rng = np.random.default_rng(L + 1)
    prefix = os.path.join(work, "l%d" % L)
    open(prefix + ".anc", "wb").write(cc.anc_text(N, [(10 * k, p, b) for k, (p, b) in enumerate(zip(parents, bl))]))
    pos = 1100 + np.cumsum(rng.integers(5, 36, L))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(pos[-1]) + 4)]
    mask = np.full(len(seq) + 100, ord("P"), np.uint8)
    for at in rng.integers(0, len(mask), 200):
        mask[at:at + int(rng.integers(1, 400))] = ord("N")
    tree = np.arange(L, dtype=np.int64) * TREES // L
    branch = rng.integers(0, 2 * N - 2, L)
    times = np.stack([max_times(p, b) for p, b in zip(parents, bl)])
    a0, a1 = times[tree, branch], times[tree, parents[tree, branch]]
    other = rng.integers(0, 3, L)  # an index into the three other bases
    alphabet = {65: "A", 67: "C", 71: "G", 84: "T"}
    rot = {65: "CGT", 67: "GTA", 71: "TAC", 84: "ACG"}
    with open(prefix + ".mut", "w") as f:
        f.write(MUT_HEAD)
        for k in range(L):
            x = int(seq[pos[k]])
            f.write("%d;%d;%d;.;%d;%d;0;0;%s;%s;%s/%s;%s;%s;\n" % (
                k, pos[k], pos[k + 1] - pos[k] if k + 1 < L else 1, tree[k], branch[k], repr(float(a0[k])), repr(float(a1[k])),
                alphabet[x], rot[x][int(other[k])], alphabet[int(seq[pos[k] - 1])], alphabet[int(seq[pos[k] + 1])]))
    open(prefix + "_ancestor.fa", "wb").write(xc.fasta_text("ancestor", seq.tobytes().decode()))
    open(prefix + "_mask.fa", "wb").write(xc.fasta_text("mask", mask.tobytes().decode()))
    return prefix


def mode_split(prefix, device):
    """`Relate --mode MutationRateWithContext` with RELATE_AMD_TIMING=1 -> wall clock and the library's own split"""
    base = os.path.basename(prefix)
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "420", CLI, "--mode", "MutationRateWithContext", "-i", base, "-o", "o%d" % device,
                        "--device", str(device), "--bins", BINS, "--mask", base + "_mask.fa", "--ancestor", base + "_ancestor.fa"],
                       cwd=os.path.dirname(prefix), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, RELATE_AMD_TIMING="1"))
    wall = time.perf_counter() - t0
    m = re.search(r"\[mutctx\] counting bases and reading the \.mut: ([0-9.]+) s; (\d+) trees of N=\d+ and (\d+) qualifying SNPs on [a-z ]+: "
                  r"([0-9.]+) s \(trees ([0-9.]+) s, counts up ([0-9.]+) s, chains ([0-9.]+) s\); reading the \.anc, the numerator and "
                  r"the rest: ([0-9.]+) s", p.stderr.decode())
    if p.returncode != 0 or not m:
        return dict(failed=p.returncode, stderr=p.stderr.decode()[-300:]), p.returncode
    return dict(process_wall_seconds=wall, counting_bases_and_mut_seconds=float(m.group(1)), trees=int(m.group(2)),
                qualifying_snps=int(m.group(3)), trees_and_snps_seconds=float(m.group(4)), trees_seconds=float(m.group(5)),
                count_copies_seconds=float(m.group(6)), chains_kernel_seconds=float(m.group(7)),
                anc_numerator_and_rest_seconds=float(m.group(8))), 0


def died(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def all_sizes():
    out_fn, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    largest = int(sys.argv[4]) if len(sys.argv) > 4 else 10 ** 6
    doc = json.load(open(out_fn)) if os.path.exists(out_fn) else {}
    doc.setdefault("what", "tools/mutctx_measure.py: MutationRateWithContext on one MI355X against the host twin, same inputs")
    for L in (10 ** 4, 10 ** 5, 10 ** 6):
        if L > largest:
            break
        stop = False
        with tempfile.TemporaryDirectory() as work:
            part = os.path.join(work, "part.json")
            p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "timing", str(L), part, str(reps)])
            if p.returncode != 0:
                doc["L%d" % L] = dict(failed=p.returncode)
                json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
                if died(p.returncode):
                    break  # nothing more is started on the device
                continue
            row = json.load(open(part))
            doc["L%d" % L] = row
            json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
            prefix = write_text(work, L)
            row["mode_end_to_end"] = dict(mut_bytes=os.path.getsize(prefix + ".mut"), ancestor_bytes=os.path.getsize(prefix + "_ancestor.fa"))
            for name, device in (("device", 0), ("host", -1)):
                row["mode_end_to_end"][name], rc = mode_split(prefix, device)
                stop = died(rc)
                if stop:
                    break
            if not stop and "failed" not in row["mode_end_to_end"]["host"] and "failed" not in row["mode_end_to_end"]["device"]:
                row["mode_end_to_end"]["same_bytes"] = all(
                    open(os.path.join(work, "o0" + ext), "rb").read() == open(os.path.join(work, "o-1" + ext), "rb").read()
                    for ext in ("_mut.bin", "_opp.bin"))
        json.dump(doc, open(out_fn, "w"), indent=1, sort_keys=True)
        if stop:
            break


if __name__ == "__main__":
    {"all": all_sizes, "timing": timing}[sys.argv[1]]()
