"""AvgMutationRate on the device (relate_amd/csrc/mutrate_kernels.hip) against the host twin, the closed form restated
in mutrate_cases.py and what the reference held and wrote (tests/golden/mutrate_ref.npz): equal bits and bytes
throughout, no time asserted (the device calls' seconds go to the test report).  Every step that uses the GPU is a
child process under a time limit of its own; after one that was killed, aborted or timed out no further step is
started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import mutrate_cases as mc
import test_mutrate_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SMALL_N = 2048  # kMutrateSmallN: above it a workgroup is 1024 threads, not 256

# the jobs of an .npz (parents<i>, bl<i>, ep<i>) one after another in one process
CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
out = {}
for i in range(int(z["jobs"])):
    t0 = time.perf_counter()
    out["out%d" % i] = api.mutrate_trees(z["parents%d" % i], z["bl%d" % i], z["ep%d" % i], device=0)
    print("seconds", time.perf_counter() - t0)
np.savez(sys.argv[3], **out)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import mutrate_cases as mc
import test_mutrate_cpu as host_tests
fx = mc.fixture()
for key in sys.argv[4:]:
    host_tests.check_trees(fx, key, 0)
    mapped = host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), key, 0)
    print("equal", key, mapped)
"""

CHILD_REFUSED = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
ep = z["epochs"]
def refused(*a):
    try:
        api.mutrate_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
refused(z["big"], np.ones(z["big"].shape), ep)     # N = 10,241
refused(z["parents"], z["bl"], np.arange(65.0))    # E = 65
refused(z["parents"], z["neg"], ep)                # a negative branch length in tree 2
refused(z["parents"], z["nan"], ep)                # a NaN in tree 0
refused(z["low"], z["bl"], ep)                     # a parent below its child in tree 1
np.savez(sys.argv[3], out=api.mutrate_trees(z["parents"], z["bl"], ep, device=0))  # the process is healthy
"""


def on_device(tmp_path, jobs, seconds=120):
    """jobs = [(parents, bl, epochs)] -> [out] of the device, one process"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"jobs": len(jobs)}
    for i, (parents, bl, ep) in enumerate(jobs):
        arrays["parents%d" % i], arrays["bl%d" % i], arrays["ep%d" % i] = parents, bl, ep
    np.savez(src, **arrays)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    z = np.load(dst)
    return [z["out%d" % i] for i in range(len(jobs))], secs


def check(tmp_path, key, jobs, closed_form=True):
    """device == host twin (== the closed form) on every job, to the bit"""
    got, secs = on_device(tmp_path, jobs)
    for (parents, bl, ep), g in zip(jobs, got):
        parents, bl = np.atleast_2d(parents), np.atleast_2d(bl)
        want = api.mutrate_trees(parents, bl, ep)
        assert g.dtype == np.float64 and host_tests.same_bits(g, want), (key, ep)
        assert not g[:, -1].any()
        if closed_form:
            for p, b, row in zip(parents, bl, g):
                assert host_tests.same_bits(row, mc.lengths_in_epochs(p, b, ep))
    bigtile.record("mutrate/" + key, dict(N=(np.atleast_2d(jobs[0][0]).shape[1] + 1) // 2, jobs=len(jobs),
                                          trees=sum(len(np.atleast_2d(j[0])) for j in jobs), device_call_seconds=secs))
    return got


def dated(N, seed):
    """the shapes at N (a caterpillar, its reverse, a balanced tree, random ones), half with lengths whose float sums
    tie at large N, half with times that rise with the label"""
    rng = np.random.default_rng(seed)
    parents = np.stack(mc.shapes(N, rng))
    bl = np.stack([mc.dated_lengths(N, rng) if k % 2 else mc.clock_lengths(p, rng) for k, p in enumerate(parents)])
    return parents, bl


@pytest.mark.parametrize("N", [2, 3, 4, 64, 65, 1025, 1026, SMALL_N, SMALL_N + 1])
def test_device_equals_host_twin(tmp_path, N):
    """one internal node; the 64-lane blocks of the time pass; the sort's padding at a power of two exactly (1024
    internal nodes) and one past it (1025: 1023 slots that do not exist); either side of the switch of workgroup
    sizes.  Default epochs and epochs over the times of clock_lengths"""
    parents, bl = dated(N, 7 * N)
    over_clock = np.concatenate(([0.0], np.exp(np.linspace(2.0, 6.0, 30))))
    check(tmp_path, "N%d" % N, [(parents, bl, mc.default_epochs()), (parents, bl, over_clock)], closed_form=N <= 65)


def test_documented_maximum(tmp_path):
    """N = 10,240, the largest N: 80 KB of LDS in a workgroup of 1024 threads, a sort network of 16,384 slots of which
    6,145 do not exist.  One random tree against the host twin and the closed form."""
    N = 10240
    rng = np.random.default_rng(N)
    parent = mc.random_tree(N, rng)
    bl = mc.dated_lengths(N, rng)
    check(tmp_path, "N10240", [(parent, bl, mc.default_epochs())])


def test_a_second_batch(tmp_path):
    """one tree more than a batch takes at N = 8 (the library's accessor says how many)"""
    N = 8
    batch = api.mutrate_batch_trees(N)
    assert batch == (2 << 20) // ((2 * N - 1) * 12 + 4)
    rng = np.random.default_rng(N)
    base = np.stack(mc.shapes(N, rng, randoms=5))
    parents = base[np.arange(batch + 1) % len(base)]
    bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
    got = check(tmp_path, "N8_batches", [(parents, bl, mc.default_epochs())], closed_form=False)[0]
    assert host_tests.same_bits(got[-1], mc.lengths_in_epochs(parents[-1], bl[-1], mc.default_epochs()))


def test_tie_heavy_trees(tmp_path):
    """N = 300 with lengths from a small set, many of them 0: runs of equal times, internal nodes at time 0; boundaries
    on those times"""
    N = 300
    rng = np.random.default_rng(300)
    parents = np.stack(mc.shapes(N, rng, randoms=3))
    bl = rng.choice(np.array([0.0, 0.0, 0.0, 100.0, 200.0, 400.0]), parents.shape)
    ep = np.array([0, 100, 200, 300, 400, 800, 1000, 1200, 5000, 1e6], np.float64)
    check(tmp_path, "N300_ties", [(parents, bl, mc.default_epochs()), (parents, bl, ep)])


def test_times_on_boundaries_empty_epochs_and_a_root_above_the_last(tmp_path):
    """epochs through the ABI so that float node times fall exactly on boundaries -- neighbouring boundaries that are
    neighbouring node times, boundaries skipped between two node times (the serial walk's cursor stays one epoch
    behind) --, an interval that crosses several empty epochs, a root above the last boundary, E = 2; and float times
    that are no round numbers with boundaries picked from them"""
    parents, bl, eps = host_tests.boundary_cases()
    jobs = [(parents, bl, ep) for ep in eps + [np.array([0, 1, 2, 3, 4, 5, 250, 1e4], np.float64)]]
    rng = np.random.default_rng(77)
    for N in (9, 40):
        p = np.stack(mc.shapes(N, rng))
        b = np.stack([mc.dated_lengths(N, rng, top=6.0) for _ in p])
        t = np.unique(np.concatenate([mc.max_times(x, y)[N:] for x, y in zip(p, b)])).astype(np.float64)
        jobs.append((p, b, np.unique(np.concatenate(([0.0], t[::3], [t[-1] * 2])))[:64]))
        jobs.append((p, b, np.unique(np.concatenate(([0.0], t[1::5], t[2::5], [t[-1] / 2])))[:64]))
    got = check(tmp_path, "boundaries", jobs)
    assert all(len(j[2]) >= 2 and j[2][0] == 0.0 for j in jobs)
    assert got[5].shape[1] == 9 and got[5][:, :-1].all()  # boundaries 0..8 under times in the hundreds: every epoch crossed


@pytest.mark.parametrize("E", [2, 64])
def test_epoch_counts(tmp_path, E):
    """N = 130 with the fewest and the most boundaries"""
    parents, bl = dated(130, E)
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1))))
    check(tmp_path, "N130_E%d" % E, [(parents, bl, ep)])


def test_fixture_cases_on_the_device(tmp_path):
    """every fixture case: rl_mutrate_trees on the device gives the harness's doubles, rl_mutrate_anc the harness's
    sums, rl_mutrate_write the reference's bytes"""
    keys = list(mc.CASES)
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path)] + keys, 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = p.stdout.decode().split()
    assert out[0::3] == ["equal"] * len(keys) and out[1::3] == keys and all(int(m) > 0 for m in out[2::3])


@pytest.mark.parametrize("key", list(mc.CASES))
def test_cli_on_the_device(tmp_path, key):
    """`Relate --mode AvgMutationRate --device 0`: the reference's _avg.rate and banner"""
    host_tests.run_cli(mc.fixture(), tmp_path, key, 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))


def test_refusals_on_the_device(tmp_path):
    """N = 10,241 and E = 65 are RL_EINVAL with the limit in the message, before any launch; a negative or NaN branch
    length and a parent below its child are named by tree; the process goes on to a correct small case"""
    rng = np.random.default_rng(9)
    parents = np.stack(mc.shapes(9, rng))
    bl = np.stack([mc.dated_lengths(9, rng) for _ in parents])
    ep = mc.default_epochs()
    neg, nan, low = bl.copy(), bl.copy(), parents.copy()
    neg[2, 4] = -0.5
    nan[0, 7] = np.nan
    low[1, 12] = 10
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, big=mc.caterpillar(10241)[None], parents=parents, bl=bl, epochs=ep, neg=neg, nan=nan, low=low)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 5 and all(ln.startswith("refused:") for ln in lines), lines
    assert "10240" in lines[0] and "N=10241" in lines[0]
    assert "64" in lines[1] and "65 given" in lines[1]
    assert "tree 2" in lines[2] and "node 4" in lines[2] and "negative" in lines[2]
    assert "tree 0" in lines[3] and "node 7" in lines[3]
    assert "tree 1" in lines[4] and "label above" in lines[4]
    assert host_tests.same_bits(np.load(dst)["out"], api.mutrate_trees(parents, bl, ep))
