#!/usr/bin/env python3
"""tests/golden/subtrees_ref.npz: what the reference's RelateExtract writes in --mode SubTreesForSubpopulation for the
cases of tests/subtrees_cases.py, and what its Tree::GetSubTree and Tree::GetCoordinates hold for every tree in full
precision (needs the reference's sources, REF=/root/reference by default).

Two programs are compiled from the reference's sources where they lie, with the flags of oracle/Makefile's `ref` rule
(asserts live), into a temporary directory outside the tree; nothing of either is kept:
  RelateExtract  the reference's program: its .anc, .mut and .poplabels bytes;
  a harness      (HARNESS below, this project's text) that reads the .anc and .mut through the reference's
                 AncMutIterators, the .poplabels through its Sample, calls Tree::GetSubTree and Tree::GetCoordinates
                 on every tree and prints convert_index, number_in_subpop, the subtree's parents, its branch lengths
                 with %a and its coordinates with %a.

  a      the real dated sequence of tests/golden/coalrate_ref.npz (N = 8, 355 trees, its real .mut without the optional
         columns), four diploid samples in four groups, two of them of interest (M = 4)
  one    N = 24, 14 synthetic trees (neighbours an interchange or two apart, or alike but for their lengths), twelve
         diploid samples in three groups, one of interest (M = 8); some SNPs on two branches
  dup    the same, two groups named with a duplicate and out of order (M = 16)
  all    the same, all three groups named: the identity path
  All    the same under `--pop_of_interest All`
  freq   a .mut with the flanking bases and a frequency column per group; two groups of interest
  hap    a haploid .poplabels (24 lines, ploidy 1), one group of interest (M = 8)
  m2     a group of one diploid sample: M = 2
  drop   trees 2, 3 and 9 have SNPs only on branches without a subset leaf below them: dropped
  tail   the last three trees have no SNPs: the walk ends with the .mut

The reference must finish on every case, and subtrees_cases.subtree must equal the harness's arrays on every tree to
the bit, before anything is written.  The reference's own run time per case is printed: a CPU number."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coalrate_cases as cc  # noqa: E402
import subtrees_cases as sc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
RI = os.path.join(REF, "include")
REF_SRCS = ["filesystem.cpp", "plot.cpp", "data.cpp", "sample.cpp", "fast_painting.cpp", "anc.cpp", "mutations.cpp",
            "tree_builder.cpp", "branch_length_estimator.cpp", "anc_builder.cpp", "tree_comparer.cpp",
            "gzstream/gzstream.cpp"]  # oracle/Makefile REF_SRCS
FLAGS = ["-O3", "-std=c++14", "-w"]

HARNESS = r"""
// prints what the reference's Tree::GetSubTree and Tree::GetCoordinates give for every tree of a sequence:
//   harness x.anc x.mut x.poplabels POPS
#include <cstdio>
#include <string>
#include <vector>
#include "gzstream.hpp"
#include "sample.hpp"
#include "anc.hpp"
#include "mutations.hpp"

int main(int argc, char *argv[]) {
  if (argc != 5) return 2;
  AncMutIterators ancmut(argv[1], argv[2]);
  Sample sample;
  sample.Read(argv[3]);
  sample.AssignPopOfInterest(argv[4]);
  MarginalTree mtr;
  Muts::iterator it_mut;
  std::vector<int> convert_index, number_in_subpop;
  std::vector<float> coordinates;
  printf("N %d M %d trees %d\n", ancmut.NumTips(), sample.group_of_interest_size, ancmut.NumTrees());
  while (ancmut.NextTree(mtr, it_mut) >= 0.0) {
    Tree subtree;
    mtr.tree.GetSubTree(sample, subtree, convert_index, number_in_subpop);
    subtree.GetCoordinates(coordinates);
    printf("convert");
    for (int x : convert_index) printf(" %d", x);
    printf("\ncount");
    for (int x : number_in_subpop) printf(" %d", x);
    printf("\nparent");
    for (Node &n : subtree.nodes) printf(" %d", n.parent == NULL ? -1 : (*n.parent).label);
    printf("\nbl");
    for (Node &n : subtree.nodes) printf(" %a", n.branch_length);
    printf("\ntime");
    for (float x : coordinates) printf(" %a", (double)x);
    printf("\n");
  }
  return 0;
}
"""


def build_reference(work):
    """RelateExtract as include/extract/CMakeLists.txt lists it and the harness, flags of oracle/Makefile's ref rule"""
    inc = ["-I" + os.path.join(RI, d) for d in ("src", "src/gzstream", "pipeline", "extract")]
    srcs = [os.path.join(RI, "src", s) for s in REF_SRCS]
    harness_cpp = os.path.join(work, "harness.cpp")
    open(harness_cpp, "w").write(HARNESS)
    units = srcs + [os.path.join(RI, "extract", "RelateExtract.cpp"), harness_cpp]
    objs, procs = [], []
    for k, s in enumerate(units):
        o = os.path.join(work, "o%d.o" % k)
        objs.append(o)
        procs.append(subprocess.Popen(["g++"] + FLAGS + inc + ["-c", s, "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("the reference's RelateExtract (or the harness) does not compile here")
    exes = []
    for name, own in (("RelateExtract", objs[-2]), ("harness", objs[-1])):
        exes.append(os.path.join(work, name))
        subprocess.check_call(["g++"] + FLAGS + objs[:len(srcs)] + [own, "-lz", "-o", exes[-1]])
    return exes


def u8(b):
    return np.frombuffer(b, np.uint8)


def run_case(exes, work, key, case):
    """-> dict(out_anc, out_mut, out_poplabels bytes; the harness's five arrays per tree)"""
    for ext in ("anc", "mut", "poplabels"):
        open(os.path.join(work, key + "." + ext), "wb").write(case[ext])
    files = [key + ".anc", key + ".mut", key + ".poplabels"]
    t0 = time.time()
    p = subprocess.run([exes[0], "--mode", "SubTreesForSubpopulation", "--anc", files[0], "--mut", files[1], "--poplabels", files[2],
                        "--pop_of_interest", case["pops"], "-o", key + "_out"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    seconds = time.time() - t0
    if p.returncode != 0:
        raise SystemExit("case %s: RelateExtract ends with %d: %s" % (key, p.returncode, p.stderr.decode()[-300:].strip()))
    h = subprocess.run([exes[1]] + files + [case["pops"]], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if h.returncode != 0:
        raise SystemExit("case %s: the harness ends with %d: %s" % (key, h.returncode, h.stderr.decode()[-300:].strip()))
    out = {"out_" + ext: u8(open(os.path.join(work, key + "_out." + ext), "rb").read()) for ext in ("anc", "mut", "poplabels")}
    rows = {"convert": [], "count": [], "parent": [], "bl": [], "time": []}
    lines = h.stdout.decode().splitlines()
    head = lines[0].split()
    out["N"], out["M"] = int(head[1]), int(head[3])
    for ln in lines[1:]:
        tag, *vals = ln.split()
        rows[tag].append([float.fromhex(x) for x in vals] if tag in ("bl", "time") else [int(x) for x in vals])
    out["convert_index"], out["number_in_subpop"] = np.array(rows["convert"], np.int32), np.array(rows["count"], np.int32)
    out["sub_parent"], out["sub_bl"] = np.array(rows["parent"], np.int32), np.array(rows["bl"], np.float64)
    out["sub_time"] = np.array(rows["time"], np.float64).astype(np.float32)
    assert np.array_equal(out["sub_time"].astype(np.float64), np.array(rows["time"], np.float64))
    out["seconds"] = seconds
    return out


def main():
    z = {}
    cases = {"a": sc.case_inputs(None, "a")}
    cases.update(sc.synthetic_cases())
    assert tuple(cases) == sc.CASES
    with tempfile.TemporaryDirectory() as work:
        exes = build_reference(work)
        for key, case in cases.items():
            got = run_case(exes, work, key, case)
            N, parents, bl = cc.parse_anc_text(case["anc"])
            names, of_interest, subset = sc.subset_of(case["poplabels"], case["pops"])
            assert N == got["N"] and len(subset) == got["M"], (key, N, len(subset), got["N"], got["M"])
            want = sc.subtrees(parents, bl, subset)
            bad = sc.same(got, want)
            assert not bad, "the restatement and the reference differ on case %s: %s" % (key, bad)
            if key != "a":
                for name in ("anc", "mut", "poplabels"):
                    z[key + "/" + name] = u8(case[name])
                z[key + "/pops"] = np.array(case["pops"])
            for name in ("out_anc", "out_mut", "out_poplabels"):
                z[key + "/" + name] = got[name]
            # the harness's arrays are what subtrees_cases.subtree gives (asserted above): a few trees are kept as
            # the record of it
            for name in sc.OUTPUTS:
                z[key + "/" + name] = got[name][:3]
            kept = int(got["out_anc"].tobytes().split(b"\n")[1].split()[1])
            print("case %-5s N %3d M %3d: %3d of %3d trees kept, %4d SNPs kept; the reference took %.3f s on this host's CPU" % (
                key, N, got["M"], kept, len(parents), got["out_mut"].tobytes().count(b"\n") - 1, got["seconds"]))
    assert int(z["drop/out_anc"].tobytes().split(b"\n")[1].split()[1]) <= 11
    np.savez_compressed(sc.FIXTURE, **z)
    print("%s: %d bytes" % (sc.FIXTURE, os.path.getsize(sc.FIXTURE)))
    for k in sorted(z):
        print("  %-24s %s %s" % (k, z[k].shape, z[k].dtype))


if __name__ == "__main__":
    main()
