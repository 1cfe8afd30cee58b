"""CoalRateForTree on the device (relate_amd/csrc/coaltree_kernels.hip) against the host twin, the closed form restated
in coaltree_cases.py and what the reference held and wrote (tests/golden/coaltree_ref.npz): equal bits of num and denom
in every block, equal bytes, no time asserted (the device calls' seconds go to the test report).  Every step that uses
the GPU is a child process under a time limit of its own; after one that was killed, aborted or timed out no further
step is started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import coaltree_cases as ct
import test_coaltree_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SMALL_N = 2048  # kCoaltreeSmallN: above it a workgroup of the terms kernel is 1024 threads, not 256

# the jobs of an .npz (parents<i>, bl<i>, f<i>, ep<i>, bs<i>) one after another in one process
CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
out = {}
for i in range(int(z["jobs"])):
    t0 = time.perf_counter()
    out["num%d" % i], out["denom%d" % i] = api.coaltree_trees(z["parents%d" % i], z["bl%d" % i], z["f%d" % i], z["ep%d" % i],
                                                              int(z["bs%d" % i]), device=0)
    print("seconds", time.perf_counter() - t0)
np.savez(sys.argv[3], **out)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import coaltree_cases as ct
import test_coaltree_cpu as host_tests
fx = ct.fixture()
for key in sys.argv[4:]:
    host_tests.check_blocks(fx, key, 0)
    trees = host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), key, 0)
    print("equal", key, trees)
"""

CHILD_REFUSED = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
ep, f = z["epochs"], z["f"]
def refused(*a):
    try:
        api.coaltree_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
refused(z["big"], np.ones(z["big"].shape), [1.0], ep)  # N = 10,241
refused([-1], [0.0], [1.0], ep)                       # N = 1
refused(z["parents"], z["bl"], f, np.arange(65.0))    # E = 65
refused(z["parents"], z["bl"], f, np.zeros(1))        # E = 1
refused(z["parents"], z["bl"], z["fneg"], ep)         # a negative factor on tree 3
refused(z["parents"], z["bl"], z["fnan"], ep)         # a NaN factor on tree 1
refused(z["parents"], z["neg"], f, ep)                # a negative branch length in tree 2
refused(z["parents"], z["nan"], f, ep)                # a NaN in tree 0
refused(z["low"], z["bl"], f, ep)                     # a parent below its child in tree 1
num, denom = api.coaltree_trees(z["parents"], z["bl"], f, ep, device=0)  # the process is healthy
np.savez(sys.argv[3], num=num, denom=denom)
"""


def on_device(tmp_path, jobs, seconds=120):
    """jobs = [(parents, bl, factors, epochs, block size)] -> [(num, denom)] of the device, one process"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"jobs": len(jobs)}
    for i, job in enumerate(jobs):
        for name, a in zip(("parents", "bl", "f", "ep", "bs"), job):
            arrays["%s%d" % (name, i)] = a
    np.savez(src, **arrays)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    z = np.load(dst)
    return [(z["num%d" % i], z["denom%d" % i]) for i in range(len(jobs))], secs


def check(tmp_path, key, jobs, closed_form=True):
    """device == host twin (== the closed form) on every job: num and denom of every block, to the bit"""
    got, secs = on_device(tmp_path, jobs)
    for (parents, bl, f, ep, bs), (num, denom) in zip(jobs, got):
        parents, bl = np.atleast_2d(parents), np.atleast_2d(bl)
        want_num, want_denom = api.coaltree_trees(parents, bl, f, ep, bs)
        assert num.dtype == denom.dtype == np.float64 and num.shape == (api.coaltree_num_blocks(len(parents), bs), len(ep))
        assert host_tests.same_bits(num, want_num) and host_tests.same_bits(denom, want_denom), (key, ep, bs)
        assert not num[:, -1].any() and not denom[:, -1].any()
        if closed_form:
            cf_num, cf_denom = ct.block_sums(parents, bl, f, ep, bs)
            assert host_tests.same_bits(num, cf_num) and host_tests.same_bits(denom, cf_denom), (key, ep, bs)
    bigtile.record("coaltree/" + key, dict(N=(np.atleast_2d(jobs[0][0]).shape[1] + 1) // 2, jobs=len(jobs),
                                           trees=sum(len(np.atleast_2d(j[0])) for j in jobs), device_call_seconds=secs))
    return got


def factors_for(n, rng):
    """float32 bases, halves among them, every fifth tree without SNPs"""
    f = rng.integers(1, 20000, n).astype(np.float32) / np.float32(2)
    f[::5] = 0
    return f


def dated(N, seed):
    """the shapes at N (a caterpillar, its reverse, a balanced tree, random ones), half with lengths whose float sums
    tie at large N, half with times that rise with the label"""
    rng = np.random.default_rng(seed)
    parents = np.stack(ct.shapes(N, rng))
    bl = np.stack([ct.dated_lengths(N, rng) if k % 2 else ct.clock_lengths(p, rng) for k, p in enumerate(parents)])
    return parents, bl, factors_for(len(parents), rng)


@pytest.mark.parametrize("N", [2, 3, 64, 65, 66, 100, SMALL_N, SMALL_N + 1])
def test_device_equals_host_twin(tmp_path, N):
    """one and two internal nodes; 63, 64 and 65 internal nodes, around one wavefront of the time pass; 99 internal
    nodes, where 29 slots of the sort network do not exist; either side of the switch of workgroup sizes.  Default
    epochs and epochs over the times of clock_lengths, blocks of two trees"""
    parents, bl, f = dated(N, 7 * N)
    over_clock = np.concatenate(([0.0], np.exp(np.linspace(2.0, 6.0, 30))))
    check(tmp_path, "N%d" % N, [(parents, bl, f, ct.default_epochs(), 2), (parents, bl, f, over_clock, 2)], closed_form=N <= 100)


def test_documented_maximum(tmp_path):
    """N = 10,240, the largest N: 80 KB of LDS in a workgroup of 1024 threads, a sort network of 16,384 slots of which
    6,145 do not exist; three random trees in blocks of two, against the host twin and the closed form"""
    N = 10240
    rng = np.random.default_rng(N)
    parents = np.stack([ct.random_tree(N, rng) for _ in range(3)])
    bl = np.stack([ct.dated_lengths(N, rng) for _ in range(3)])
    check(tmp_path, "N10240", [(parents, bl, np.array([1500.5, 0.0, 320.0], np.float32), ct.default_epochs(), 2)])


@pytest.mark.parametrize("E", [2, 64])
def test_epoch_counts(tmp_path, E):
    """N = 130 with the fewest and the most boundaries"""
    parents, bl, f = dated(130, E)
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1))))
    check(tmp_path, "N130_E%d" % E, [(parents, bl, f, ep, ct.BLOCK_SIZE)])


def test_tie_heavy_trees(tmp_path):
    """N = 300 with lengths from a small set, many of them 0: runs of equal times, internal nodes at time 0; boundaries
    on those times"""
    N = 300
    rng = np.random.default_rng(300)
    parents = np.stack(ct.shapes(N, rng, randoms=3))
    bl = rng.choice(np.array([0.0, 0.0, 0.0, 100.0, 200.0, 400.0]), parents.shape)
    ep = np.array([0, 100, 200, 300, 400, 800, 1000, 1200, 5000, 1e6], np.float64)
    f = factors_for(len(parents), rng)
    check(tmp_path, "N300_ties", [(parents, bl, f, ct.default_epochs(), 4), (parents, bl, f, ep, 4)])


def test_times_on_boundaries_empty_epochs_and_a_root_above_the_last(tmp_path):
    """epochs through the ABI so that float node times fall exactly on boundaries, an interval that crosses several
    empty epochs, a root above the last boundary, all nodes in one epoch (E = 2 and E = 3), every epoch empty but the
    first and the last; and float times that are no round numbers with boundaries picked from them"""
    parents, bl, f, eps = host_tests.boundary_cases()
    jobs = [(parents, bl, f, ep, 4) for ep in eps + [np.array([0, 150, 151, 152, 153, 154, 1e9], np.float64),
                                                     np.array([0, 1e9, 2e9], np.float64)]]
    rng = np.random.default_rng(77)
    for N in (9, 40):
        p = np.stack(ct.shapes(N, rng))
        b = np.stack([ct.dated_lengths(N, rng, top=6.0) for _ in p])
        t = np.unique(np.concatenate([ct.max_times(x, y)[N:] for x, y in zip(p, b)])).astype(np.float64)
        g = factors_for(len(p), rng)
        jobs.append((p, b, g, np.unique(np.concatenate(([0.0], t[::3], [t[-1] * 2])))[:64], 3))
        jobs.append((p, b, g, np.unique(np.concatenate(([0.0], t[1::5], t[2::5], [t[-1] / 2])))[:64], 3))
    got = check(tmp_path, "boundaries", jobs)
    assert all(len(j[3]) >= 2 and j[3][0] == 0.0 for j in jobs)
    num, denom = got[len(eps)]  # [0, 150, 151 .. 154, 1e9]: nothing coalesces in epochs 1 to 4, every tree crosses them
    assert num[:, 0].all() and num[:, 5].all() and not num[:, 1:5].any() and denom[:, 1:5].all()
    assert got[len(eps) + 1][0][:, 0].all() and not got[len(eps) + 1][1][:, 1:].any()  # all nodes in epoch 0, no exit


def test_blocks_of_three(tmp_path):
    """10 trees in blocks of 3, of 1 and of 50: the chains kernel starts and ends inside a batch at every block edge"""
    parents, bl, f, ep = host_tests.random_case(24, 31, 3, trees=10)
    got = check(tmp_path, "N24_blocks", [(parents, bl, f, ep, bs) for bs in (3, 1, 50)])
    assert [len(g[0]) for g in got] == [4, 11, 1]


def test_a_block_across_two_launches(tmp_path):
    """more trees than a batch takes at N = 24 (the library's accessor says how many) in blocks of 350, which divide
    neither the batch nor the tree count: block 26 gets its first trees from one launch of the chains kernel and the
    rest from the next, through the accumulators in device memory"""
    N = 24
    batch = api.coaltree_batch_trees(N)
    assert batch == (16 << 20) // ((2 * N - 1) * 12 + (N - 1) * 8 + 64 * 16 + 8) == 9425
    trees, bs = batch + 300, 350
    assert batch % bs and trees % bs and (batch - 1) // bs == batch // bs == 26
    rng = np.random.default_rng(N)
    base = np.stack(ct.shapes(N, rng, randoms=5))
    parents = base[np.arange(trees) % len(base)]
    bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
    check(tmp_path, "N24_batches", [(parents, bl, factors_for(trees, rng), ct.default_epochs(), bs)])


def test_fixture_cases_on_the_device(tmp_path):
    """every fixture case: rl_coaltree_trees on the device gives the harness's doubles in every block, rl_coaltree_anc
    their sum, rl_coaltree_write the reference's bytes"""
    keys = list(ct.CASES)
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path)] + keys, 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = p.stdout.decode().split()
    assert out[0::3] == ["equal"] * len(keys) and out[1::3] == keys and all(int(m) > 0 for m in out[2::3])


@pytest.mark.parametrize("key", list(ct.CASES))
def test_cli_on_the_device(tmp_path, key):
    """`Relate --mode CoalRateForTree --device 0`: the reference's .coal and banner"""
    host_tests.run_cli(ct.fixture(), tmp_path, key, 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))


def test_refusals_on_the_device(tmp_path):
    """N = 10,241, N = 1, E = 65 and E = 1 are RL_EINVAL with the limit in the message, before any launch; a negative
    or NaN factor, a negative or NaN branch length and a parent below its child are named by tree; the process goes
    on to a correct small case"""
    parents, bl, f, ep = host_tests.random_case(9, 31, 9)
    neg, nan, low, fneg, fnan = bl.copy(), bl.copy(), parents.copy(), f.copy(), f.copy()
    neg[2, 4] = -0.5
    nan[0, 7] = np.nan
    low[1, 12] = 10
    fneg[3] = -1.0
    fnan[1] = np.nan
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, big=ct.caterpillar(10241)[None], parents=parents, bl=bl, f=f, epochs=ep, neg=neg, nan=nan, low=low,
             fneg=fneg, fnan=fnan)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 9 and all(ln.startswith("refused:") for ln in lines), lines
    assert "10240" in lines[0] and "N=10241" in lines[0]
    assert "N=1)" in lines[1]
    assert "64" in lines[2] and "65 given" in lines[2]
    assert "1 given" in lines[3]
    assert "tree 3" in lines[4] and "factor" in lines[4]
    assert "tree 1" in lines[5] and "factor" in lines[5]
    assert "tree 2" in lines[6] and "node 4" in lines[6] and "negative" in lines[6]
    assert "tree 0" in lines[7] and "node 7" in lines[7]
    assert "tree 1" in lines[8] and "label above" in lines[8]
    z = np.load(dst)
    want_num, want_denom = api.coaltree_trees(parents, bl, f, ep)
    assert host_tests.same_bits(z["num"], want_num) and host_tests.same_bits(z["denom"], want_denom)
