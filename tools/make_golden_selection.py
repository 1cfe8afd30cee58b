#!/usr/bin/env python3
"""tests/golden/selection_ref.npz: what the reference's RelateSelection writes in --mode Frequency and --mode Selection
for the cases of tests/frequency_cases.py (needs the reference's sources, REF=/root/reference by default).

The reference program is compiled from its sources where they lie, with the flags of oracle/Makefile's `ref` rule
(asserts live), into a temporary directory outside the tree; nothing of it is kept.

  a       case a of tests/golden/coalrate_ref.npz (a real dated tree sequence, N = 8, 355 trees, 3000 SNPs): .freq,
          .lin and .sele in full
  b       case b of coalrate_ref.npz (N = 24, six synthetic trees, every SNP on leaf 0), default epochs
  b_bins  the same with --bins 2,6,0.5
  s       the 40 random dated trees of coalrate_ref.npz's case c (N = 300) with a .mut of this tool: three SNPs per
          tree on random branches, tree 7 without SNPs, and rows the filter drops (two branches, flipped, the root, -1,
          an age above the root); the .mut rows as arrays, the three files in full
  tie     N = 16, 12 trees whose branch lengths come from {0, 100, 200, 400}: equal node times, internal nodes at
          time 0.  The reference's walk asserts on some such inputs (its asserts are live), and its Selection sizes
          its table of log(k!) by the lineages the FIRST row has at the boundary 0, which a row of a tree with an
          internal node at time 0 can exceed -- a read outside the table, not an answer.  The tool goes through the
          seeds from 1 and keeps the first on which the reference finishes both modes with every row inside the
          table; the seeds it dropped are in `tie/dropped_seeds`.  The trees and rows as arrays, the three files in
          full.

Every case is checked here to be tie-free (a, b, s) or not (tie), and the tie-free ones against the closed form of
frequency_cases.py before anything is written."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coalrate_cases as cc  # noqa: E402
import frequency_cases as fc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
RI = os.path.join(REF, "include")
REF_SRCS = ["filesystem.cpp", "plot.cpp", "data.cpp", "sample.cpp", "fast_painting.cpp", "anc.cpp", "mutations.cpp",
            "tree_builder.cpp", "branch_length_estimator.cpp", "anc_builder.cpp", "tree_comparer.cpp",
            "gzstream/gzstream.cpp"]  # oracle/Makefile REF_SRCS


def build_reference(work):
    """RelateSelection as include/evaluate/CMakeLists.txt lists it, flags of oracle/Makefile's ref rule"""
    exe = os.path.join(work, "RelateSelection")
    inc = ["-I" + os.path.join(RI, d) for d in ("src", "src/gzstream", "pipeline", "evaluate/selection")]
    srcs = [os.path.join(RI, "evaluate", "selection", "RelateSelection.cpp")] + [os.path.join(RI, "src", s) for s in REF_SRCS]
    objs, procs = [], []
    for k, s in enumerate(srcs):
        o = os.path.join(work, "o%d.o" % k)
        objs.append(o)
        procs.append(subprocess.Popen(["g++", "-O3", "-std=c++14", "-w"] + inc + ["-c", s, "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("the reference's RelateSelection does not compile here")
    subprocess.check_call(["g++", "-O3", "-std=c++14", "-w"] + objs + ["-lz", "-o", exe])
    return exe


def u8(b):
    return np.frombuffer(b, np.uint8)


def frequency_and_selection(exe, work, prefix, out, bins=None):
    """-> (.freq, .lin, .sele) of the reference, or None if it does not finish"""
    for args in (["--mode", "Frequency", "-i", prefix, "-o", out] + (["--bins", bins] if bins else []),
                 ["--mode", "Selection", "-i", out, "-o", out]):
        p = subprocess.run([exe] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if p.returncode != 0:
            return None
    return tuple(open(os.path.join(work, out + ext), "rb").read() for ext in (".freq", ".lin", ".sele"))


def inside_table(lin):
    """no row has more lineages than the first row has at the boundary 0 (Selection's N)"""
    rows = [[int(x) for x in ln.split()[2:]] for ln in lin.decode().split("\n")[1:-1]]
    return all(max(r) <= rows[0][-3] for r in rows)


def keep(z, key, files):
    z[key + "/freq"], z[key + "/lin"], z[key + "/sele"] = (u8(f) for f in files)


def main():
    co = cc.fixture()
    z = {}
    with tempfile.TemporaryDirectory() as work:
        exe = build_reference(work)
        ep = cc.default_epochs()
        # ---- a, b, b_bins: the inputs are coalrate_ref.npz's
        for tag in "ab":
            open(os.path.join(work, tag + ".anc"), "wb").write(co[tag + "/anc"].tobytes())
            open(os.path.join(work, tag + ".mut"), "wb").write(co[tag + "/mut"].tobytes())
            N, parents, bl = cc.parse_anc_text(co[tag + "/anc"].tobytes())
            assert all(fc.tie_free(p, b) for p, b in zip(parents, bl)), tag
            keep(z, tag, frequency_and_selection(exe, work, tag, tag + "_out"))
        keep(z, "b_bins", frequency_and_selection(exe, work, "b", "b_bins", bins=fc.BINS))
        # ---- s
        N, trees = fc.case_s_rows(co)
        assert all(fc.tie_free(p, b) for _, p, b in trees)
        rows = fc.random_rows(N, trees, np.random.default_rng(7), per_tree=3, skip=(7,))
        open(os.path.join(work, "s.anc"), "wb").write(cc.anc_text(N, trees))
        open(os.path.join(work, "s.mut"), "wb").write(fc.mut_text(rows))
        files = frequency_and_selection(exe, work, "s", "s_out")
        want = fc.files_by_closed_form(N, trees, rows, ep)
        assert files[:2] == want, "the closed form and the reference differ on case s"
        keep(z, "s", files)
        z["s/rows"], z["s/ages"] = fc.rows_as_arrays(rows)
        # ---- tie
        dropped = []
        for seed in range(1, 200):
            N, trees = 16, fc.tie_trees(16, 12, seed)
            assert not all(fc.tie_free(p, b) for _, p, b in trees)
            rows = fc.random_rows(N, trees, np.random.default_rng(1000 + seed), per_tree=4, filtered=False)
            open(os.path.join(work, "tie.anc"), "wb").write(cc.anc_text(N, trees))
            open(os.path.join(work, "tie.mut"), "wb").write(fc.mut_text(rows))
            files = frequency_and_selection(exe, work, "tie", "tie_out")
            if files is not None and inside_table(files[1]):
                break
            dropped.append(seed)
        else:
            raise SystemExit("the reference finished on no tie case")
        keep(z, "tie", files)
        z["tie/parents"] = np.stack([t[1] for t in trees]).astype(np.int16)
        z["tie/bl"] = np.stack([t[2] for t in trees]).astype(np.float32)
        z["tie/pos"] = np.array([t[0] for t in trees], np.int32)
        z["tie/rows"], z["tie/ages"] = fc.rows_as_arrays(rows)
        z["tie/seed"], z["tie/dropped_seeds"] = np.array([seed], np.int32), np.array(dropped, np.int32)
    np.savez_compressed(fc.FIXTURE, **z)
    print("%s: %d bytes (coalrate_ref.npz: %d)" % (fc.FIXTURE, os.path.getsize(fc.FIXTURE), os.path.getsize(cc.FIXTURE)))
    for k in sorted(z):
        print("  %-18s %s" % (k, z[k].shape))


if __name__ == "__main__":
    main()
