#!/usr/bin/env python3
"""tests/golden/mutrate_ref.npz: what the reference's RelateMutationRate writes in --mode Avg for the cases of
tests/mutrate_cases.py, and what its code holds in full precision (needs the reference's sources, REF=/root/reference
by default).

Two programs are compiled from the reference's sources where they lie, with the flags of oracle/Makefile's `ref` rule
(asserts live), into a temporary directory outside the tree; nothing of either is kept:
  RelateMutationRate   the reference's program: its _avg.rate bytes;
  a harness            (HARNESS below, this project's text) whose main includes the reference's AvgMutationRate.cpp by
                       path.  _avg.rate prints six digits, so it cannot hold a sum to the bit; the harness prints with
                       %a the epoch boundaries CalculateAvgMutationRateForChromosome built (caught from inside it: the
                       harness's own assert macro still aborts on a false condition and also hands the local `epochs`
                       to a probe), that function's mutation and opportunity vectors, and for EVERY tree of the .anc
                       the E-1 doubles of GetCoordsAndLineages + GetBranchLengthsInEpoch.

  a        case a of tests/golden/coalrate_ref.npz (a real dated tree sequence, N = 8, 355 trees, its real .mut)
  b        the trees of case b of coalrate_ref.npz (N = 24, six synthetic trees: a node time on a default boundary, one
           past the last) with a .mut of mutrate_cases.branch_rows, default epochs.  (With that fixture's own .mut --
           every SNP on leaf 0 with the ages 0 and 10 -- the reference writes _avg.rate in full and then ends with
           SIGFPE in its terminal plot, all rates but one being 0: it does not finish, so that .mut is not used.)
  b_bins   the same with --bins 2,6,0.5
  s        the 40 random dated trees of coalrate_ref.npz's case c (N = 300) with a .mut of mutrate_cases.branch_rows:
           ages are the branch's real [t(b), t(parent(b))], flipped rows (counted), rows with two branches (not), tree
           7 without SNPs, one dist of 40 Mb
  s_dist   the same through a --dist file that holds positions the .mut does not
  tie      N = 16, 12 trees whose branch lengths come from {0, 100, 200, 400}: equal node times, internal nodes at 0.
           The tool goes through the seeds from 1 and keeps the first on which the reference finishes; the seeds it
           dropped are in `tie/dropped_seeds`
  young    --years_per_gen 1e6 --bins 6.5,7.5,0.5 (boundaries 0, 3.16, 10, 31.6, 100): a root inside epoch 0, roots
           above the last boundary

The reference must finish on every case, and the closed form of mutrate_cases.lengths_in_epochs must equal the
harness's doubles on every tree, before anything is written."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coalrate_cases as cc  # noqa: E402
import frequency_cases as fc  # noqa: E402
import mutrate_cases as mc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
RI = os.path.join(REF, "include")
REF_SRCS = ["filesystem.cpp", "plot.cpp", "data.cpp", "sample.cpp", "fast_painting.cpp", "anc.cpp", "mutations.cpp",
            "tree_builder.cpp", "branch_length_estimator.cpp", "anc_builder.cpp", "tree_comparer.cpp",
            "gzstream/gzstream.cpp"]  # oracle/Makefile REF_SRCS
FLAGS = ["-O3", "-std=c++14", "-w"]

HARNESS = r"""
// prints what the reference's AvgMutationRate.cpp computes, in full precision.  AVG_CPP is that file's path.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "gzstream.hpp"
#include "collapsed_matrix.hpp"
#include "plot.hpp"
#include "sample.hpp"
#include "anc.hpp"
#include "mutations.hpp"
#include "anc_builder.hpp"
#include "tree_comparer.hpp"
#include "cxxopts.hpp"

static std::vector<double> epochs;  // what a function without a local `epochs` hands to the probe: nothing
static std::vector<double> caught;
static void probe(const std::vector<double> &ep) {
  if (caught.empty() && !ep.empty()) caught = ep;
}
#undef assert
#define assert(c)                                                          \
  do {                                                                     \
    probe(epochs);                                                         \
    if (!(c)) {                                                            \
      fprintf(stderr, "%s:%d: assertion `%s` failed\n", __FILE__, __LINE__, #c); \
      abort();                                                             \
    }                                                                      \
  } while (0)
#include AVG_CPP

static void print(const char *tag, const std::vector<double> &v, size_t n) {
  printf("%s", tag);
  for (size_t i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
}

int main(int argc, char *argv[]) {
  cxxopts::Options options("harness");
  options.add_options()("years_per_gen", "", cxxopts::value<float>())("bins", "", cxxopts::value<std::string>())(
      "dist", "", cxxopts::value<std::string>())("i,input", "", cxxopts::value<std::string>());
  options.parse(argc, argv);
  const std::string prefix = options["input"].as<std::string>();
  std::vector<double> mutation(4096, 0.0), opportunity(4096, 0.0);  // (the caller sizes them by its own epochs)
  CalculateAvgMutationRateForChromosome(options, mutation, opportunity);
  if (caught.empty()) {
    fprintf(stderr, "no assert inside CalculateAvgMutationRateForChromosome ran\n");
    return 2;
  }
  const size_t E = caught.size();
  print("epochs", caught, E);
  print("mutation", mutation, E);
  print("opportunity", opportunity, E);
  std::ifstream is(prefix + ".anc");
  std::string line, tag;
  int N = 0, T = 0;
  is >> tag >> N;
  getline(is, line);
  is >> tag >> T;
  getline(is, line);
  Data data(N, 1);
  std::vector<float> coordinates(2 * N - 1);
  std::vector<int> lineages(2 * N - 1);
  std::vector<double> lengths(E);
  for (int t = 0; t < T; t++) {
    getline(is, line);
    MarginalTree mtr;
    mtr.Read(line, N);
    GetCoordsAndLineages(mtr, coordinates, lineages);
    GetBranchLengthsInEpoch(data, caught, coordinates, lineages, lengths);
    print("tree", lengths, E - 1);
  }
  return 0;
}
"""


def build_reference(work):
    """RelateMutationRate as include/evaluate/CMakeLists.txt lists it and the harness, flags of oracle/Makefile's ref rule"""
    inc = ["-I" + os.path.join(RI, d) for d in ("src", "src/gzstream", "pipeline", "evaluate/mutation_rate")]
    srcs = [os.path.join(RI, "src", s) for s in REF_SRCS]
    avg = os.path.join(RI, "evaluate", "mutation_rate", "AvgMutationRate.cpp")
    harness_cpp = os.path.join(work, "harness.cpp")
    open(harness_cpp, "w").write(HARNESS)
    mains = [(os.path.join(RI, "evaluate", "mutation_rate", "RelateMutationRate.cpp"), []),
             (harness_cpp, ['-DAVG_CPP="%s"' % avg])]
    objs, procs = [], []
    for k, (s, extra) in enumerate([(s, []) for s in srcs] + mains):
        o = os.path.join(work, "o%d.o" % k)
        objs.append(o)
        procs.append(subprocess.Popen(["g++"] + FLAGS + inc + extra + ["-c", s, "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("the reference's RelateMutationRate (or the harness around it) does not compile here")
    exes = []
    for name, main_obj in (("RelateMutationRate", objs[-2]), ("harness", objs[-1])):
        exes.append(os.path.join(work, name))
        subprocess.check_call(["g++"] + FLAGS + objs[:-2] + [main_obj, "-lz", "-o", exes[-1]])
    return exes


def u8(b):
    return np.frombuffer(b, np.uint8)


def run_case(exes, work, prefix, key):
    """-> dict(rate bytes, epochs, mutation, opportunity, trees [T][E-1]) of the reference, or None if it does not finish"""
    bins, ypg, with_dist = mc.CASES[key]
    args = ["-i", prefix] + (["--bins", bins] if bins else []) + (["--years_per_gen", ypg] if ypg else []) \
        + (["--dist", prefix + ".dist"] if with_dist else [])
    p = subprocess.run([exes[0], "--mode", "Avg", "-o", key + "_out"] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        print("case %s: RelateMutationRate ends with %d: %s" % (key, p.returncode, p.stderr.decode()[-300:].strip()))
        return None
    h = subprocess.run([exes[1]] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if h.returncode != 0:
        print("case %s: the harness ends with %d: %s" % (key, h.returncode, h.stderr.decode()[-300:].strip()))
        return None
    out = {"rate": u8(open(os.path.join(work, key + "_out_avg.rate"), "rb").read()), "trees": []}
    for ln in h.stdout.decode().splitlines():
        tag, *vals = ln.split()
        v = np.array([float.fromhex(x) for x in vals], np.float64)
        if tag == "tree":
            out["trees"].append(v)
        elif tag in ("epochs", "mutation", "opportunity"):
            out[tag] = v
    out["trees"] = np.stack(out["trees"])
    return out


def check_closed_form(key, trees, got):
    ep = got["epochs"]
    assert len(got["trees"]) == len(trees), key
    for t, (_, parent, bl) in enumerate(trees):
        want = mc.lengths_in_epochs(parent, bl, ep)
        assert want[-1] == 0.0 and np.array_equal(want[:-1].view(np.uint64), got["trees"][t].view(np.uint64)), \
            "the closed form and the reference differ on tree %d of case %s" % (t, key)


def write_inputs(work, prefix, N, trees, rows=None, anc=None, mut=None, dist=None):
    open(os.path.join(work, prefix + ".anc"), "wb").write(anc if anc is not None else cc.anc_text(N, trees))
    open(os.path.join(work, prefix + ".mut"), "wb").write(mut if mut is not None else mc.mut_text(rows))
    if dist is not None:
        open(os.path.join(work, prefix + ".dist"), "wb").write(dist)


def keep(z, key, got):
    for name in ("rate", "epochs", "mutation", "opportunity", "trees"):
        z[key + "/" + name] = got[name]


def main():
    co = cc.fixture()
    z = {}
    with tempfile.TemporaryDirectory() as work:
        exes = build_reference(work)

        def finish(key, prefix, trees):
            got = run_case(exes, work, prefix, key)
            if got is None:
                raise SystemExit("the reference does not finish on case " + key)
            check_closed_form(key, trees, got)
            keep(z, key, got)

        # ---- a: the inputs are coalrate_ref.npz's; b, b_bins: its trees
        for tag in "ab":
            anc = co[tag + "/anc"].tobytes()
            N, parents, bl = cc.parse_anc_text(anc)
            trees = [(0, p, b) for p, b in zip(parents, bl)]
            if tag == "a":
                write_inputs(work, tag, N, trees, anc=anc, mut=co[tag + "/mut"].tobytes())
                finish(tag, tag, trees)
            else:
                rows = mc.branch_rows(N, trees, np.random.default_rng(24), per_tree=5, big_dist_at=-1)
                write_inputs(work, tag, N, trees, rows, anc=anc)
                finish("b", "b", trees)
                finish("b_bins", "b", trees)
                z["b/rows"], z["b/ages"] = mc.rows_as_arrays(rows)
        # ---- s, s_dist
        N, trees = fc.case_s_rows(co)
        rows = mc.branch_rows(N, trees, np.random.default_rng(11), per_tree=3, skip=(7,))
        dist = mc.dist_text(rows, np.random.default_rng(12))
        write_inputs(work, "s", N, trees, rows, dist=dist)
        finish("s", "s", trees)
        finish("s_dist", "s", trees)
        z["s/rows"], z["s/ages"] = mc.rows_as_arrays(rows)
        z["s_dist/dist"] = u8(dist)
        # ---- tie
        dropped = []
        for seed in range(1, 200):
            N, trees = 16, mc.tie_trees(16, 12, seed)
            rows = mc.branch_rows(N, trees, np.random.default_rng(1000 + seed), per_tree=4, big_dist_at=-1)
            write_inputs(work, "tie", N, trees, rows)
            got = run_case(exes, work, "tie", "tie")
            if got is not None:
                break
            dropped.append(seed)
        else:
            raise SystemExit("the reference finished on no tie case")
        check_closed_form("tie", trees, got)
        keep(z, "tie", got)
        z["tie/seed"], z["tie/dropped_seeds"] = np.array([seed], np.int32), np.array(dropped, np.int32)
        # ---- young
        N, young = mc.young_trees()
        young_rows = mc.branch_rows(N, young, np.random.default_rng(16), per_tree=4, big_dist_at=-1)
        write_inputs(work, "young", N, young, young_rows)
        finish("young", "young", young)
        ep = z["young/epochs"]
        roots = [float(mc.max_times(p, b)[-1]) for _, p, b in young]
        assert roots[0] < ep[1] and roots[1] > ep[-1], (roots, ep)
        for key, tr, rw in (("tie", trees, rows), ("young", young, young_rows)):
            z[key + "/parents"] = np.stack([t[1] for t in tr]).astype(np.int16)
            z[key + "/bl"] = np.stack([t[2] for t in tr]).astype(np.float32)
            assert np.array_equal(z[key + "/bl"].astype(np.float64), np.stack([t[2] for t in tr]))
            z[key + "/pos"] = np.array([t[0] for t in tr], np.int32)
            z[key + "/rows"], z[key + "/ages"] = mc.rows_as_arrays(rw)
    np.savez_compressed(mc.FIXTURE, **z)
    print("%s: %d bytes (selection_ref.npz: %d)" % (mc.FIXTURE, os.path.getsize(mc.FIXTURE), os.path.getsize(fc.FIXTURE)))
    for k in sorted(z):
        print("  %-20s %s" % (k, z[k].shape))


if __name__ == "__main__":
    main()
