"""SubTreesForSubpopulation on the device (relate_amd/csrc/subtrees_kernels.hip) against the host twin, the chains
restated in subtrees_cases.py and what the reference held and wrote (tests/golden/subtrees_ref.npz): equal bits of all
five outputs, equal bytes of the three files, no time asserted (the device calls' seconds go to the test report).
Every step that uses the GPU is a child process under a time limit of its own; after one that was killed, aborted or
timed out no further step is started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import subtrees_cases as sc
import test_subtrees_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SMALL_N = 2048  # kSubtreesSmallN: above it a workgroup is 1024 threads, not 256

# the jobs of an .npz (parents<i>, bl<i>, subset<i>) one after another in one process
CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
out = {}
for i in range(int(z["jobs"])):
    t0 = time.perf_counter()
    got = api.subtrees_trees(z["parents%d" % i], z["bl%d" % i], z["subset%d" % i], device=0)
    print("seconds", time.perf_counter() - t0)
    for k, a in got.items():
        out["%s%d" % (k, i)] = a
np.savez(sys.argv[3], **out)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import subtrees_cases as sc
import test_subtrees_cpu as host_tests
fx = sc.fixture()
for key in sys.argv[4:]:
    host_tests.check_trees(fx, key, 0)
    s = host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), key, 0)
    print("equal", key, s["trees_kept"])
"""

CHILD_REFUSED = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
subset = z["subset"]
def refused(*a):
    try:
        api.subtrees_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
refused(z["big"], np.ones(z["big"].shape), [0, 1])  # N = 10,241
refused(z["parents"], z["neg"], subset)              # a negative branch length in tree 2
refused(z["parents"], z["nan"], subset)              # a NaN in tree 0
refused(z["low"], z["bl"], subset)                   # a parent below its child in tree 1
refused(z["parents"], z["bl"], [1, 4, 9])            # a subset label out of range
got = api.subtrees_trees(z["parents"], z["bl"], subset, device=0)  # the process is healthy
np.savez(sys.argv[3], **got)
"""


def on_device(tmp_path, jobs, seconds=120):
    """jobs = [(parents, bl, subset)] -> [dict of the five outputs] of the device, one process"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"jobs": len(jobs)}
    for i, job in enumerate(jobs):
        for name, a in zip(("parents", "bl", "subset"), job):
            arrays["%s%d" % (name, i)] = a
    np.savez(src, **arrays)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    z = np.load(dst)
    return [{k: z["%s%d" % (k, i)] for k in sc.OUTPUTS} for i in range(len(jobs))], secs


def check(tmp_path, key, jobs):
    """device == host twin == the chains on every job: all five outputs, to the bit"""
    got, secs = on_device(tmp_path, jobs)
    for (parents, bl, subset), out in zip(jobs, got):
        parents, bl = np.atleast_2d(parents), np.atleast_2d(bl)
        assert not sc.same(out, api.subtrees_trees(parents, bl, subset)), (key, len(subset))
        assert not sc.same(out, sc.subtrees(parents, bl, subset)), (key, len(subset))
    bigtile.record("subtrees/" + key, dict(N=(np.atleast_2d(jobs[0][0]).shape[1] + 1) // 2, jobs=len(jobs),
                                           trees=sum(len(np.atleast_2d(j[0])) for j in jobs), device_call_seconds=secs))
    return got


def subsets(N, rng):
    """M = 2 with the two lowest leaves (on a caterpillar the chain of N-2 steps) and with the two highest, every
    second leaf, M = N - 1, M = N, a random subset"""
    out = [[0, 1], [N - 2, N - 1], list(range(0, N, 2)), list(range(1, N)), list(range(N)),
           sorted(rng.choice(N, max(2, N // 3), replace=False).tolist())]
    return [np.array(s, np.int32) for s in out if 2 <= len(s) <= N]


def trees_at(N, seed, randoms=2):
    """the shapes at N (a caterpillar, its reverse, a balanced tree, random ones) with lengths of mixed magnitudes"""
    rng = np.random.default_rng(seed)
    parents = np.stack(sc.shapes(N, rng, randoms=randoms))
    return parents, np.stack([sc.mixed_lengths(p, rng) for p in parents]), rng


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 129, SMALL_N, SMALL_N + 1])
def test_device_equals_host_twin(tmp_path, N):
    """one and two internal nodes; 62, 63, 64 and 128 internal nodes, the edges of the 64-wide pull scan; either side
    of the switch of workgroup sizes.  Every shape with every subset; the sums depend on the order of addition"""
    parents, bl, rng = trees_at(N, 11 * N)
    jobs = [(parents, bl, s) for s in subsets(N, rng)]
    if N >= 63:
        assert sc.reversed_chain_differs(parents[0], bl[0], jobs[0][2])  # the caterpillar's long chain
    check(tmp_path, "N%d" % N, jobs)


def test_documented_maximum(tmp_path):
    """N = 10,240, the largest N: 80 KB of LDS in a workgroup of 1024 threads.  A caterpillar with its two lowest leaves
    (one chain of 10,238 steps on one lane), its reverse with the two highest, a balanced and a random tree with every
    second leaf, all but one leaf and all leaves"""
    N = 10240
    parents, bl, rng = trees_at(N, N, randoms=1)
    assert sc.reversed_chain_differs(parents[0], bl[0], [0, 1])
    jobs = [(parents[:2], bl[:2], np.array([0, 1], np.int32)), (parents[:2], bl[:2], np.array([N - 2, N - 1], np.int32)),
            (parents[2:], bl[2:], np.arange(0, N, 2, dtype=np.int32)), (parents[2:], bl[2:], np.arange(1, N, dtype=np.int32)),
            (parents[3:], bl[3:], np.arange(N, dtype=np.int32))]
    check(tmp_path, "N10240", jobs)


def test_more_trees_than_a_batch(tmp_path):
    """more trees than a batch takes at N = 24 (the library's accessor says how many): two launches"""
    N = 24
    batch = api.subtrees_batch_trees(N)
    assert batch == (16 << 20) // ((2 * N - 1) * 36 + 4) == 9892
    rng = np.random.default_rng(N)
    base = np.stack(sc.shapes(N, rng, randoms=5))
    parents = base[np.arange(batch + 300) % len(base)]
    bl = np.exp(rng.uniform(0.0, 14.0, parents.shape))
    got, secs = on_device(tmp_path, [(parents, bl, np.arange(0, N, 3, dtype=np.int32))])
    assert not sc.same(got[0], api.subtrees_trees(parents, bl, np.arange(0, N, 3)))
    bigtile.record("subtrees/N24_batches", dict(N=N, trees=len(parents), device_call_seconds=secs))


def test_fixture_cases_on_the_device(tmp_path):
    """every fixture case: rl_subtrees_trees on the device gives what the reference's harness held, rl_subtrees_files
    the reference's three files"""
    keys = list(sc.CASES)
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path)] + keys, 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = p.stdout.decode().split()
    assert out[0::3] == ["equal"] * len(keys) and out[1::3] == keys and all(int(m) > 0 for m in out[2::3])


@pytest.mark.parametrize("key", list(sc.CASES))
def test_cli_on_the_device(tmp_path, key):
    """`Relate --mode SubTreesForSubpopulation --device 0`: the reference's files and banner"""
    host_tests.run_cli(sc.fixture(), tmp_path, key, 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))


def test_refusals_on_the_device(tmp_path):
    """N = 10,241 is RL_EINVAL with the limit in the message, before any launch; a negative or NaN branch length and a
    parent below its child are named by tree; a subset label out of range by its entry; the process goes on to a
    correct small case"""
    rng = np.random.default_rng(9)
    N = 9
    parents = np.stack(sc.shapes(N, rng))
    bl = np.stack([sc.mixed_lengths(p, rng) for p in parents])
    subset = np.array([1, 4, 5, 8], np.int32)
    neg, nan, low = bl.copy(), bl.copy(), parents.copy()
    neg[2, 4], nan[0, 7], low[1, 12] = -0.5, np.nan, 10
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, big=sc.caterpillar(10241)[None], parents=parents, bl=bl, subset=subset, neg=neg, nan=nan, low=low)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 5 and all(ln.startswith("refused:") for ln in lines), lines
    assert "10240" in lines[0] and "N=10241" in lines[0]
    assert "tree 2" in lines[1] and "node 4" in lines[1] and "negative" in lines[1]
    assert "tree 0" in lines[2] and "node 7" in lines[2]
    assert "tree 1" in lines[3] and "label above" in lines[3]
    assert "entry 2" in lines[4] and "not a leaf" in lines[4]
    z = np.load(dst)
    assert not sc.same({k: z[k] for k in sc.OUTPUTS}, sc.subtrees(parents, bl, subset))
