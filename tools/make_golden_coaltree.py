#!/usr/bin/env python3
"""tests/golden/coaltree_ref.npz: what the reference's RelateCoalescentRate writes in --mode CoalRateForTree for the
cases of tests/coaltree_cases.py, and what its coal_tree holds in full precision (needs the reference's sources,
REF=/root/reference by default).

Two programs are compiled from the reference's sources where they lie, with the flags of oracle/Makefile's `ref` rule
(asserts live), into a temporary directory outside the tree; nothing of either is kept:
  RelateCoalescentRate  the reference's program: its .coal bytes;
  a harness             (HARNESS below, this project's text) whose main includes the reference's
                        CoalescentRateForSection.cpp by path, is linked with its coal_tree.cpp and calls
                        CoalescenceRateForTree.  The .coal prints six
                        digits, so it cannot hold a sum to the bit; the harness reads the coal_tree that function
                        built, after its Dump, and prints with %a the epoch boundaries and every block's num
                        and denom after the last tree.

  a        case a of tests/golden/coalrate_ref.npz (a real dated tree sequence, N = 8, 355 trees, its real .mut)
  b        case b of coalrate_ref.npz (N = 24, six synthetic trees: a zero-length branch, a node time on a boundary
           of the float epochs, a root past the last boundary; tree 4 without SNPs), default epochs
  b_bins   the same with --bins 2,6,0.5
  tie      N = 16, 12 trees whose branch lengths come from {0, 100, 200, 400}: equal node times, internal nodes at 0
  on       N = 16 under --years_per_gen 8, whose first and last default boundaries (125 and 12,500,000) are float32
           values: node times exactly ON them, one float32 step to either side, a root above the last
  young    --years_per_gen 1e6 --bins 6.5,7.5,0.5 (boundaries 0, 3.16, 10, 31.6, 100): a root inside epoch 0, roots
           above the last boundary
  many     N = 5, 3000 trees: the reference's own blocks of 1000 are crossed and its fourth block stays empty

The reference must finish on every case, and the closed form of coaltree_cases.block_sums must equal the harness's
doubles in every block, before anything is written."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coalrate_cases as cc  # noqa: E402
import coaltree_cases as ct  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
RI = os.path.join(REF, "include")
REF_SRCS = ["filesystem.cpp", "plot.cpp", "data.cpp", "sample.cpp", "fast_painting.cpp", "anc.cpp", "mutations.cpp",
            "tree_builder.cpp", "branch_length_estimator.cpp", "anc_builder.cpp", "tree_comparer.cpp",
            "gzstream/gzstream.cpp"]  # oracle/Makefile REF_SRCS
FLAGS = ["-O3", "-std=c++14", "-w"]

HARNESS = r"""
// prints what the reference's coal_tree holds after CoalescenceRateForTree, in full precision.  SECTION_CPP is the
// path of the reference's CoalescentRateForSection.cpp.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include <sys/resource.h>
#include "gzstream.hpp"
#include "collapsed_matrix.hpp"
#include "plot.hpp"
#include "sample.hpp"
#include "anc.hpp"
#include "mutations.hpp"
#include "anc_builder.hpp"
#include "tree_comparer.hpp"
#include "cxxopts.hpp"

class coal_tree;
static void probe(coal_tree &ct);
static struct Nothing {
} ct;  // (what `ct` names in a function without a coal_tree of that name)
static void probe(Nothing &) {}
// coal_tree.hpp has no include guard, so it comes in once, through CoalescentRateForSection.cpp -- with its members
// open to probe() (every other header that file names is in already; coal_tree.cpp is linked as it is).
// CoalescenceRateForTree's one coal_tree is its local `ct`, and the getrusage after its Dump is the last thing it does
#define private public
#define getrusage(who, usage) getrusage(who, (probe(ct), usage))
#include SECTION_CPP
#undef getrusage
#undef private

static void print(const char *tag, const std::vector<double> &v) {
  printf("%s", tag);
  for (size_t i = 0; i < v.size(); i++) printf(" %a", v[i]);
  printf("\n");
}
static void probe(coal_tree &ct) {
  print("epochs", ct.epochs);
  printf("blocks %d\n", ct.num_blocks);
  for (size_t b = 0; b < ct.num.size(); b++) {
    print("num", ct.num[b]);
    print("denom", ct.denom[b]);
  }
}

int main(int argc, char *argv[]) {
  cxxopts::Options options("harness");
  options.add_options()("help", "")("years_per_gen", "", cxxopts::value<float>())("bins", "", cxxopts::value<std::string>())(
      "dist", "", cxxopts::value<std::string>())("chr", "", cxxopts::value<std::string>())(
      "coal", "", cxxopts::value<std::string>())("i,input", "", cxxopts::value<std::string>())(
      "o,output", "", cxxopts::value<std::string>());
  options.parse(argc, argv);
  CoalescenceRateForTree(options);
  return 0;
}
"""


def build_reference(work):
    """RelateCoalescentRate as include/evaluate/CMakeLists.txt lists it and the harness, flags of oracle/Makefile's ref rule"""
    inc = ["-I" + os.path.join(RI, d) for d in ("src", "src/gzstream", "pipeline", "evaluate/coalescent_rate")]
    cr = os.path.join(RI, "evaluate", "coalescent_rate")
    srcs = [os.path.join(RI, "src", s) for s in REF_SRCS]
    harness_cpp = os.path.join(work, "harness.cpp")
    open(harness_cpp, "w").write(HARNESS)
    units = [(s, []) for s in srcs] + [
        (os.path.join(cr, "coal_tree.cpp"), []), (os.path.join(cr, "RelateCoalescentRate.cpp"), []),
        (harness_cpp, ['-DSECTION_CPP="%s"' % os.path.join(cr, "CoalescentRateForSection.cpp")])]
    objs, procs = [], []
    for k, (s, extra) in enumerate(units):
        o = os.path.join(work, "o%d.o" % k)
        objs.append(o)
        procs.append(subprocess.Popen(["g++"] + FLAGS + inc + extra + ["-c", s, "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("the reference's RelateCoalescentRate (or the harness around it) does not compile here")
    shared = objs[:len(srcs)]
    exes = []
    for name, own in (("RelateCoalescentRate", objs[len(srcs):len(srcs) + 2]), ("harness", [objs[len(srcs)], objs[-1]])):
        exes.append(os.path.join(work, name))
        subprocess.check_call(["g++"] + FLAGS + shared + own + ["-lz", "-o", exes[-1]])
    return exes


def u8(b):
    return np.frombuffer(b, np.uint8)


def run_case(exes, work, prefix, key):
    """-> dict(coal bytes, epochs, num [blocks][E], denom) of the reference"""
    bins, ypg = ct.CASES[key]
    args = ["-i", prefix] + (["--bins", bins] if bins else []) + (["--years_per_gen", ypg] if ypg else [])
    p = subprocess.run([exes[0], "--mode", "CoalRateForTree", "-o", key + "_out"] + args, cwd=work, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise SystemExit("case %s: RelateCoalescentRate ends with %d: %s" % (key, p.returncode, p.stderr.decode()[-300:].strip()))
    h = subprocess.run([exes[1], "-o", key + "_harness"] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if h.returncode != 0:
        raise SystemExit("case %s: the harness ends with %d: %s" % (key, h.returncode, h.stderr.decode()[-300:].strip()))
    out = {"coal": u8(open(os.path.join(work, key + "_out.coal"), "rb").read()), "num": [], "denom": []}
    assert open(os.path.join(work, key + "_harness.coal"), "rb").read() == out["coal"].tobytes(), key
    for ln in h.stdout.decode().splitlines():
        tag, *vals = ln.split()
        if tag == "blocks":
            blocks = int(vals[0])
            continue
        v = np.array([float.fromhex(x) for x in vals], np.float64)
        if tag == "epochs":
            out[tag] = v
        elif tag in ("num", "denom"):
            out[tag].append(v)
    out["num"], out["denom"] = np.stack(out["num"]), np.stack(out["denom"])
    assert len(out["num"]) == len(out["denom"]) == blocks, key
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def main():
    co = cc.fixture()
    z = {}
    with tempfile.TemporaryDirectory() as work:
        exes = build_reference(work)

        def finish(key, prefix, parents, bl, rows):
            got = run_case(exes, work, prefix, key)
            factors = cc.mut_factors(rows, len(parents))
            num, denom = ct.block_sums(parents, bl, factors, got["epochs"])
            assert got["num"].shape == num.shape == (ct.num_blocks(len(parents)), len(got["epochs"])), key
            assert np.array_equal(bits(num), bits(got["num"])) and np.array_equal(bits(denom), bits(got["denom"])), \
                "the closed form and the reference differ on case " + key
            for name in ("coal", "epochs", "num", "denom"):
                z[key + "/" + name] = got[name]
            print("case %-7s %5d trees, %d blocks, %d of %d epochs with a rate" % (
                key, len(parents), len(num), int((got["denom"].sum(0) != 0).sum()), len(got["epochs"])))

        # ---- a, b, b_bins: the inputs are coalrate_ref.npz's
        for tag in "ab":
            anc, mut = co[tag + "/anc"].tobytes(), co[tag + "/mut"].tobytes()
            open(os.path.join(work, tag + ".anc"), "wb").write(anc)
            open(os.path.join(work, tag + ".mut"), "wb").write(mut)
            N, parents, bl = cc.parse_anc_text(anc)
            for key in ("a",) if tag == "a" else ("b", "b_bins"):
                finish(key, tag, parents, bl, cc.parse_mut_text(mut))
        # ---- tie, on, young, many: written here, kept in the fixture
        young_N, young = ct.young_trees()
        on_N, on = ct.on_boundary_trees()
        many_N, many = ct.many_trees()
        for key, N, trees, seed, skip in (("tie", 16, ct.tie_trees(16, 12, 3), 1, ()), ("on", on_N, on, 2, (5,)),
                                          ("young", young_N, young, 3, ()), ("many", many_N, many, 4, (0, 999, 1000, 2500))):
            rows = ct.mut_rows(len(trees), np.random.default_rng(seed), skip)
            open(os.path.join(work, key + ".anc"), "wb").write(cc.anc_text(N, trees))
            open(os.path.join(work, key + ".mut"), "wb").write(cc.mut_text(rows))
            parents, bl = np.stack([t[1] for t in trees]), np.stack([t[2] for t in trees])
            finish(key, key, parents, bl, rows)
            z[key + "/parents"] = parents.astype(np.int16)
            z[key + "/bl"] = bl.astype(np.float32) if np.array_equal(bl.astype(np.float32).astype(np.float64), bl) else bl
            z[key + "/pos"] = np.array([t[0] for t in trees], np.int32)
            z[key + "/mut"] = np.array(rows, np.int32)
        ep = z["young/epochs"]
        roots = [float(ct.max_times(p, b)[-1]) for _, p, b in young]
        assert roots[0] < ep[1] and roots[1] > ep[-1], (roots, ep)
        assert z["on/epochs"][1] == 125.0 and z["on/epochs"][-1] == 12500000.0
        assert len(z["many/num"]) == 4 and not z["many/num"][3].any() and not z["many/denom"][3].any() and z["many/num"][2].any()
    np.savez_compressed(ct.FIXTURE, **z)
    print("%s: %d bytes" % (ct.FIXTURE, os.path.getsize(ct.FIXTURE)))
    for k in sorted(z):
        print("  %-20s %s %s" % (k, z[k].shape, z[k].dtype))


if __name__ == "__main__":
    main()
