"""CompareTopology on the device (relate_amd/csrc/compare_kernels.hip clade_distance_kernel) against the host
implementation, integer for integer, and end to end on the trees of the exact and the fast summation modes against
the brute-force oracle of compare_cases.py.  Every step that uses the GPU is a child process under a time limit of
its own; after one that was killed, aborted or timed out no further step is started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import compare_cases as cc
from golden_util import Fixture
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")

CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
t0 = time.perf_counter()
out = api.compare_trees(z["A"], z["B"], z["pairs"], device=0)
np.savez(sys.argv[3], out=out, seconds=time.perf_counter() - t0)
"""


def on_device(tmp_path, A, B, pairs, seconds=120):
    A, B = np.atleast_2d(A), np.atleast_2d(B)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, A=A, B=B, pairs=np.asarray(pairs, np.int32).reshape(-1, 2))
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    z = np.load(dst)
    return z["out"], float(z["seconds"])


def paired(n):
    return np.repeat(np.arange(n), 2).reshape(-1, 2)


@pytest.mark.parametrize("N", [2, 3, 4, 8, 64, 65, 257, 1000])
def test_device_equals_host_on_the_cpu_suites_cases(tmp_path, N):
    rng = np.random.default_rng(N)
    trees = [cc.random_tree(N, rng) for _ in range(24)]
    if N >= 4:
        trees += [cc.caterpillar(N), cc.balanced(N), cc.caterpillar(N, rng.permutation(N))]
    if N >= 3:
        trees += [cc.nni(trees[k], rng) for k in range(4)]
    A = np.stack(trees)
    B = np.stack(trees[::-1])
    pairs = [(i, j) for i in range(len(A)) for j in range(0, len(B), 3)] + [(k, len(B) - 1 - k) for k in range(len(A))]
    host = api.compare_trees(A, B, pairs)
    got, _ = on_device(tmp_path, A, B, pairs)
    assert got.dtype == np.int32 and got.tolist() == host.tolist()
    # ... and both equal the definition on a few of them (the CPU suite holds the host to it everywhere)
    for k in range(0, len(pairs), max(1, len(pairs) // 12)):
        assert got[k] == cc.oracle_distance(A[pairs[k][0]], B[pairs[k][1]])
    assert not got[-len(A):].any()  # a tree against itself
    if N >= 3:
        assert got[pairs.index((0, 3))] == 2  # tree 0 against its interchange (the fourth tree from the end)


@pytest.mark.parametrize("N", [5000, 10000])
def test_large_trees_device_equals_host(tmp_path, N):
    """64 pairs at the sizes whose tables fill most of a CU's LDS (14 N bytes), a caterpillar pair among them"""
    rng = np.random.default_rng(N)
    A = [cc.random_tree(N, rng) for _ in range(60)]
    B = [cc.random_tree(N, rng) for _ in range(56)] + A[56:60]  # four pairs of a tree with itself
    A += [cc.caterpillar(N), cc.caterpillar(N), cc.balanced(N), cc.caterpillar(N, rng.permutation(N))]
    B += [cc.caterpillar(N, rng.permutation(N)), cc.balanced(N), cc.caterpillar(N), cc.caterpillar(N)]
    A, B = np.stack(A), np.stack(B)
    assert len(A) == 64 and len(B) == 64
    host = api.compare_trees(A, B)
    got, seconds = on_device(tmp_path, A, B, paired(64), seconds=300)
    assert got.tolist() == host.tolist()
    assert not host[56:60].any() and host[:56].min() > 0 and host.max() <= 2 * (N - 2)
    assert host[61] == host[62]  # caterpillar against balanced, both ways round
    bigtile.record("compare_topology/large_N%d" % N,
                   dict(pairs=64, device_call_seconds=seconds, distances_min_max=[int(host.min()), int(host.max())],
                        caterpillar_pairs=[int(x) for x in host[60:]]))


def test_device_refuses_what_the_host_refuses(tmp_path):
    good = cc.caterpillar(6)
    bad = good.copy()
    bad[[8, 9]] = bad[[9, 8]]
    bad[bad == 8], bad[bad == 9] = -9, 8
    bad[bad == -9] = 9
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    for a, b, which in ((bad, good, "A"), (good, bad, "B")):
        np.savez(src, A=a[None], B=b[None], pairs=np.zeros((1, 2), np.int32))
        p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], 120)
        err = p.stderr.decode()
        assert p.returncode == 1 and "error -1" in err and "of %s" % which in err and "label above" in err, err[-2000:]


def test_end_to_end_exact_and_fast_modes(tmp_path):
    """PaintBuildTopology of synth70 with --sum_mode exact twice and lanes32 once; CompareTopology of the sections'
    .anc files: exact against exact is identical everywhere, exact against lanes32 is whatever the brute-force oracle
    says of the same two files (no magnitude is asserted: the figures go to the report)"""
    runs = {}
    for tag, mode in (("exact1", "exact"), ("exact2", "exact"), ("lanes32", "lanes32")):
        work = tmp_path / tag
        (work / "out").mkdir(parents=True)
        fx = Fixture("synth70", work / "out")
        p = gpu_step([CLI, "--mode", "PaintBuildTopology", "--chunk_index", "0", "-o", "out", "--sum_mode", mode], 600,
                     cwd=str(work))
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        runs[tag] = work / "out" / "chunk_0"
    N, W = fx.N, fx.W
    totals = {"exact2": [0, 0, 0.0, 0], "lanes32": [0, 0, 0.0, 0]}  # SNPs, identical SNPs, sum of len * d / full, max d
    for w in range(W):
        a = str(runs["exact1"] / ("out_%d.anc" % w))
        for tag in ("exact2", "lanes32"):
            b = str(runs[tag] / ("out_%d.anc" % w))
            cmp = tmp_path / ("%s_%d" % (tag, w))
            p = gpu_step([CLI, "--mode", "CompareTopology", "-i", a + "," + b, "-o", cmp.name, "--device", "0"], 120,
                         cwd=str(tmp_path))
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            said = dict(line.split() for line in p.stdout.decode().splitlines())
            cli_rows = np.loadtxt(str(cmp) + ".cmp", dtype=np.int64, ndmin=2).tolist()
            host = api.compare_anc(a, b)  # device=None: the host implementation
            assert cli_rows == host["per_interval"].tolist()
            assert float(said["mean_normalised_distance"]) == host["mean_normalised"]
            assert float(said["share_identical"]) == host["share_identical"]
            assert int(said["max_distance"]) == host["max_distance"]
            na, ta = cc.read_anc(open(a, "rb").read())
            nb, tb = cc.read_anc(open(b, "rb").read())
            rows, want = cc.oracle_compare(N, [t[:2] for t in ta], ta[-1][3], [t[:2] for t in tb], tb[-1][3])
            cc.check_summary(host, rows, want)
            if tag == "exact2":
                assert all(r[4] == 0 for r in cli_rows) and host["share_identical"] == 1.0
                assert host["max_distance"] == 0 and host["mean_normalised"] == 0.0
            t = totals[tag]
            snps = want["snp_end"] - want["snp_begin"]
            t[0] += snps
            t[1] += want["snps_identical"]
            t[2] += want["mean_normalised"] * snps
            t[3] = max(t[3], want["max_distance"])
    for tag, (snps, same, weighted, worst) in totals.items():
        bigtile.record("compare_topology/synth70_exact_vs_%s" % tag,
                       dict(N=N, sections=W, snps=snps, share_identical=same / snps, mean_normalised=weighted / snps,
                            max_distance=worst, full_distance=2 * (N - 2)))
