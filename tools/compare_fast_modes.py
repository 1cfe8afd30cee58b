#!/usr/bin/env python3
"""What the fast summation modes change in the trees: `Relate --mode PaintBuildTopology` of the test fixtures with
--sum_mode exact, lanes and lanes32, then CompareTopology (on the device) of every section's .anc against the exact
mode's, summed over the sections.  Findings for DESIGN.md, not thresholds.

    python tools/compare_fast_modes.py OUT.json [fixture ...]      (default: synth24 synth70 synth40_noisy example8)
        a fixture named synth:N:L:GB is a synthetic block-coalescent chunk of that shape (windows as --memory GB gives
        them), generated from a seed as bench.py's is
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


def chunk_of(name, where):
    """the chunk files of a test fixture, or of synth:N:L:GB, written to `where` -> object with N, L, W"""
    if not name.startswith("synth:"):
        from golden_util import Fixture
        return Fixture(name, where)
    import rlutil
    N, L, mem = name.split(":")[1:]
    N, L, mem = int(N), int(L), float(mem)
    ch = rlutil.synth_chunk(N, L, seed=1, budget=mem * 1e9 / 4.0 - (2.0 * N * N + 3.0 * N))
    ch.write(where)
    return ch


def main():
    from relate_amd import api
    out_fn = sys.argv[1]
    names = sys.argv[2:] or ["synth24", "synth70", "synth40_noisy", "example8"]
    res = {"what": "PaintBuildTopology per summation mode, every section's .anc against --sum_mode exact's "
                   "(rl_compare_anc on the device), sums over the sections", "fixtures": {}}
    for name in names:
        with tempfile.TemporaryDirectory() as tmp:
            for mode in ("exact", "lanes", "lanes32"):
                os.makedirs(os.path.join(tmp, mode, "out"))
                fx = chunk_of(name, os.path.join(tmp, mode, "out"))
                subprocess.run(["timeout", "-k", "10", "900", CLI, "--mode", "PaintBuildTopology", "--chunk_index", "0",
                                "-o", "out", "--sum_mode", mode], cwd=os.path.join(tmp, mode), check=True,
                               stderr=subprocess.DEVNULL)
            row = {"N": fx.N, "L": fx.L, "sections": fx.W, "full_distance": 2 * (fx.N - 2)}
            for mode in ("lanes", "lanes32"):
                snps = same = worst = trees = 0
                weighted = 0.0
                for w in range(fx.W):
                    s = api.compare_anc(os.path.join(tmp, "exact", "out", "chunk_0", "out_%d.anc" % w),
                                        os.path.join(tmp, mode, "out", "chunk_0", "out_%d.anc" % w), device=0)
                    n = s["snp_end"] - s["snp_begin"]
                    snps += n
                    same += s["snps_identical"]
                    weighted += s["mean_normalised"] * n
                    worst = max(worst, s["max_distance"])
                    trees += s["trees_b"] - s["trees_a"]
                row["exact_vs_" + mode] = {"snps": snps, "share_identical": same / snps, "mean_normalised": weighted / snps,
                                           "max_distance": worst, "trees_more_than_exact": trees}
            res["fixtures"][name] = row
            json.dump(res, open(out_fn, "w"), indent=1)
            print(name, json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
