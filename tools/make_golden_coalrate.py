#!/usr/bin/env python3
"""tests/golden/coalrate_ref.npz: what the reference's RelateCoalescentRate writes for the three cases of
tests/coalrate_cases.py (needs /root/reference and oracle/_ref/Relate, `make -C oracle ref`).

The reference program is compiled from its sources where they lie, with the flags of oracle/Makefile's `ref` rule,
into a temporary directory outside the tree; nothing of it is kept.

  a  a real dated tree sequence: `Relate --mode All` of the reference on the first 3000 SNPs of
     tests/golden/example_data (N = 8) with a uniform 1 cM/Mb map; its .anc / .mut text, and the reference's .bin and
     .coal (without and with --poplabels) in full
  b  coalrate_cases.case_b (N = 24, synthetic): .anc / .mut text, .bin for the default epochs and for --bins 2,6,0.5,
     .coal without and with --poplabels (haploid labels, three groups)
  c  coalrate_cases.case_c (N = 300, 40 random trees): the inputs as arrays, the md5 of the text files written from
     them, the md5 of every plane of the .bin
"""
import gzip
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coalrate_cases as cc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
RI = os.path.join(REF, "include")
REF_RELATE = os.path.join(ROOT, "oracle", "_ref", "Relate")
REF_SRCS = ["filesystem.cpp", "plot.cpp", "data.cpp", "sample.cpp", "fast_painting.cpp", "anc.cpp", "mutations.cpp",
            "tree_builder.cpp", "branch_length_estimator.cpp", "anc_builder.cpp", "tree_comparer.cpp",
            "gzstream/gzstream.cpp"]  # oracle/Makefile REF_SRCS


def build_reference(work):
    """RelateCoalescentRate as include/evaluate/CMakeLists.txt:1-2 lists it, flags of oracle/Makefile's ref rule"""
    exe = os.path.join(work, "RelateCoalescentRate")
    inc = ["-I" + os.path.join(RI, d) for d in ("src", "src/gzstream", "pipeline", "evaluate/coalescent_rate")]
    cr = os.path.join(RI, "evaluate", "coalescent_rate")
    srcs = [os.path.join(cr, "coal_tree.cpp"), os.path.join(cr, "RelateCoalescentRate.cpp")] + \
           [os.path.join(RI, "src", s) for s in REF_SRCS]
    objs = []
    procs = []
    for k, s in enumerate(srcs):
        o = os.path.join(work, "o%d.o" % k)
        objs.append(o)
        procs.append(subprocess.Popen(["g++", "-O3", "-std=c++14", "-w"] + inc + ["-c", s, "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("the reference's RelateCoalescentRate does not compile here")
    subprocess.check_call(["g++", "-O3", "-std=c++14", "-w"] + objs + ["-lz", "-o", exe])
    return exe


def run(exe, args, cwd):
    subprocess.run([exe] + args, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def section_and_finalize(exe, work, prefix, out, poplabels, bins=None):
    """-> (.bin, .coal, .coal with --poplabels) of the reference"""
    run(exe, ["--mode", "CoalescentRateForSection", "-i", prefix, "-o", out] + (["--bins", bins] if bins else []), work)
    run(exe, ["--mode", "FinalizePopulationSize", "-o", out], work)
    coal = open(os.path.join(work, out + ".coal"), "rb").read()
    run(exe, ["--mode", "FinalizePopulationSize", "-o", out, "--poplabels", poplabels], work)
    return open(os.path.join(work, out + ".bin"), "rb").read(), coal, open(os.path.join(work, out + ".coal"), "rb").read()


def u8(b):
    return np.frombuffer(b, np.uint8)


def main():
    if not os.path.exists(REF_RELATE):
        raise SystemExit("oracle/_ref/Relate is missing: make -C oracle ref")
    z = {}
    with tempfile.TemporaryDirectory() as work:
        exe = build_reference(work)
        # ---- a
        lines = []
        with gzip.open(os.path.join(ROOT, "tests", "golden", "example_data", "example.haps.gz"), "rt") as f:
            for i, line in enumerate(f):
                if i >= 3000:
                    break
                lines.append(line)
        open(os.path.join(work, "ex.haps"), "w").writelines(lines)
        with gzip.open(os.path.join(ROOT, "tests", "golden", "example_data", "example.sample.gz"), "rb") as f:
            open(os.path.join(work, "ex.sample"), "wb").write(f.read())
        first, last = int(lines[0].split()[2]), int(lines[-1].split()[2])
        with open(os.path.join(work, "ex.map"), "w") as f:
            f.write("pos COMBINED_rate Genetic_Map\n")
            for bp in range(max(0, first - 50000), last + 100000, 50000):
                f.write("%d 1.0 %.6f\n" % (bp, bp * 1e-6))
        run(REF_RELATE, ["--mode", "All", "-m", "1.25e-8", "-N", "30000", "--haps", "ex.haps", "--sample", "ex.sample",
                         "--map", "ex.map", "--seed", "1", "-o", "a"], work)
        N = int(open(os.path.join(work, "a.anc")).readline().split()[1])
        with open(os.path.join(work, "a.poplabels"), "w") as f:
            f.write("sample population group sex\n")
            for i in range(N // 2):
                f.write("id%d %s G NA\n" % (i, "POPB" if i % 2 else "POPA"))
        z["a/anc"], z["a/mut"] = u8(open(os.path.join(work, "a.anc"), "rb").read()), u8(open(os.path.join(work, "a.mut"), "rb").read())
        z["a/poplabels"] = u8(open(os.path.join(work, "a.poplabels"), "rb").read())
        b, c, cg = section_and_finalize(exe, work, "a", "a_out", "a.poplabels")
        z["a/bin"], z["a/coal"], z["a/coal_groups"] = u8(b), u8(c), u8(cg)
        # ---- b
        N, trees, rows = cc.case_b()
        open(os.path.join(work, "b.anc"), "wb").write(cc.anc_text(N, trees))
        open(os.path.join(work, "b.mut"), "wb").write(cc.mut_text(rows))
        with open(os.path.join(work, "b.poplabels"), "w") as f:
            f.write("sample population group sex\n")
            for i in range(N):
                f.write("h%d %s G 1\n" % (i, ("ZED", "ALPHA", "MID")[(i * 7) % 3]))
        z["b/anc"], z["b/mut"] = u8(cc.anc_text(N, trees)), u8(cc.mut_text(rows))
        z["b/poplabels"] = u8(open(os.path.join(work, "b.poplabels"), "rb").read())
        b, c, cg = section_and_finalize(exe, work, "b", "b_out", "b.poplabels")
        z["b/bin"], z["b/coal"], z["b/coal_groups"] = u8(b), u8(c), u8(cg)
        b, c, cg = section_and_finalize(exe, work, "b", "b_bins", "b.poplabels", bins=cc.BINS)
        z["b/bin_bins"], z["b/coal_bins"] = u8(b), u8(c)
        # ---- c
        N, trees, rows = cc.case_c()
        anc, mut = cc.anc_text(N, trees), cc.mut_text(rows)
        open(os.path.join(work, "c.anc"), "wb").write(anc)
        open(os.path.join(work, "c.mut"), "wb").write(mut)
        run(exe, ["--mode", "CoalescentRateForSection", "-i", "c", "-o", "c_out"], work)
        ep, D = cc.parse_bin(open(os.path.join(work, "c_out.bin"), "rb").read())
        z["c/parents"] = np.stack([t[1] for t in trees]).astype(np.int16)
        z["c/bl"] = np.stack([t[2] for t in trees]).astype(np.float32)
        assert np.array_equal(z["c/bl"].astype(np.float64), np.stack([t[2] for t in trees]))
        z["c/pos"] = np.array([t[0] for t in trees], np.int32)
        z["c/mut"] = np.array(rows, np.int32)
        z["c/anc_md5"], z["c/mut_md5"] = u8(hashlib.md5(anc).digest()), u8(hashlib.md5(mut).digest())
        z["c/epochs"], z["c/plane_md5"] = ep, cc.plane_md5(D)
    np.savez_compressed(cc.FIXTURE, **z)
    print("%s: %d bytes" % (cc.FIXTURE, os.path.getsize(cc.FIXTURE)))
    for k in sorted(z):
        print("  %-16s %s" % (k, z[k].shape))


if __name__ == "__main__":
    main()
