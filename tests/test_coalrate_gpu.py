"""CoalescentRateForSection on the device (relate_amd/csrc/coalrate_kernels.hip) against the host implementation, the
numpy restatement of coalrate_cases.py and the reference's files (tests/golden/coalrate_ref.npz): equal bits and
bytes throughout, no time asserted (the device calls' seconds go to the test report).  Every step that uses the GPU
is a child process under a time limit of its own; after one that was killed, aborted or timed out no further step is
started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import coalrate_cases as cc
import test_coalrate_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SMALL_N = 1024  # kCoalrateSmallN: above it the kernels run with larger workgroups (256 / 1024 threads, not 64 / 256)
# dynamic LDS above 48 KB is asked for with hipFuncSetAttribute: the accumulation (11 N bytes, rounded up to 16) from
# N = 4469, the preparation (8 (N-1) bytes) from N = 6146
LDS_ACCUMULATE_N = 4469
LDS_PREPARE_N = 6146

CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
counts = [int(c) for c in z["counts"]]
for k, c in enumerate(counts):
    t0 = time.perf_counter()
    D = api.coalrate_trees(z["parents"][:c], z["bl"][:c], z["factors"][:c], z["epochs"], device=0)
    print("seconds", time.perf_counter() - t0)
    np.save(sys.argv[3] + "_%d.npy" % k, D)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import coalrate_cases as cc
import test_coalrate_cpu as host_tests
fx = cc.fixture()
for tag in "abc":
    host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), tag, 0)
    print("equal", tag)
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
        api.coalrate_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
refused(z["big"], np.ones(z["big"].shape), [1.0], ep)                       # N = 10,241
refused(z["parents"], z["bl"], z["factors"], np.arange(65, dtype=np.float32))   # E = 65
refused(z["parents"], z["neg"], z["factors"], ep)                          # a negative branch length in tree 2
refused(z["ternary"], z["bl"], z["factors"], ep)                           # a node with three children in tree 1
np.save(sys.argv[3], api.coalrate_trees(z["parents"], z["bl"], z["factors"], ep, device=0))  # the process is healthy
"""


def on_device(tmp_path, parents, bl, factors, ep, counts=None, seconds=120):
    """-> ([D per count of leading trees], [seconds per device call])"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out")
    counts = [len(parents)] if counts is None else counts
    np.savez(src, parents=parents, bl=bl, factors=np.asarray(factors, np.float32), epochs=ep, counts=counts)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    return [np.load("%s_%d.npy" % (dst, k), mmap_mode="r") for k in range(len(counts))], secs


def check(tmp_path, key, parents, bl, factors, ep, restatement=True, host=True):
    (D,), (secs,) = on_device(tmp_path, parents, bl, factors, ep)
    N = (parents.shape[1] + 1) // 2
    assert D.dtype == np.float32 and D.shape == (len(ep), N, N)
    if host:
        assert cc.same_bits(D, api.coalrate_trees(parents, bl, factors, ep))
    if restatement:
        assert cc.same_bits(D, cc.reference_bins(parents, bl, factors, ep))
    bigtile.record("coalescent_rate/" + key, dict(N=N, E=len(ep), trees=len(parents), device_call_seconds=secs))


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 257, SMALL_N, SMALL_N + 1])
def test_device_equals_host_and_restatement(tmp_path, N):
    """wave-width and workgroup-width edges of the scans, both sides of the switch of workgroup sizes (1025: three rows
    per workgroup, the last workgroup with two); a caterpillar, its reverse, a balanced tree and random ones; the
    factors 0, -1 and 1e6 among them; the default 31 epochs up to N = 257, six above"""
    parents, bl, factors = host_tests.case(N, N)
    check(tmp_path, "N%d" % N, parents, bl, factors, host_tests.epochs_of(31 if N <= 257 else 6))


@pytest.mark.parametrize("N", [1537, LDS_ACCUMULATE_N - 1, LDS_ACCUMULATE_N, LDS_PREPARE_N - 1, LDS_PREPARE_N])
def test_device_across_the_lds_switches(tmp_path, N):
    """the sizes at which the launchers change route, E = 3 (D is 453 MB at N = 6146): 1537, the smallest N with four
    rows per workgroup and a partial last workgroup; either side of the accumulation's and of the preparation's
    48 KB of dynamic LDS.  A caterpillar and a random tree against the restatement and the host."""
    rows = (N + 511) // 512
    assert (N + rows - 1) // rows * rows != N  # a partial last workgroup
    rng = np.random.default_rng(N)
    parents = np.stack(cc.shapes(N, rng, randoms=1))[[0, 3]]
    bl = np.stack([cc.dated_lengths(N, rng) for _ in parents])
    check(tmp_path, "N%d" % N, parents, bl, [3.5, 1e6], host_tests.epochs_of(3))


def test_boundary_cases_of_fixture_b_on_the_device(tmp_path):
    """a time exactly on a boundary, a zero-length branch, a root past the last boundary and exactly on it, a factor 0
    and the trailing -1, through rl_coalrate_trees: the reference's .bin"""
    fx = cc.fixture()
    N, parents, bl = cc.parse_anc_text(fx["b/anc"].tobytes())
    P, B, F = cc.with_trailing_pass(parents, bl, cc.mut_factors(cc.parse_mut_text(fx["b/mut"].tobytes()), len(parents)))
    ep = api.coalrate_epochs()
    (D,), _ = on_device(tmp_path, P, B, F, ep)
    assert cc.bin_bytes(ep, D) == fx["b/bin"].tobytes()


@pytest.mark.parametrize("E", [2, 31, 64])
def test_epoch_counts(tmp_path, E):
    """N = 130 (129 internal nodes: two full blocks of 64 and one lane) with the fewest, the default and the most
    epochs: 64 epochs are eight rounds of eight planes in flight"""
    parents, bl, factors = host_tests.case(130, E)
    check(tmp_path, "N130_E%d" % E, parents, bl, factors, host_tests.epochs_of(E))


def test_batches(tmp_path):
    """N = 4000: a tree takes 131,996 bytes of the 2 MB a batch may, 15 trees per batch (the library's accessor says
    so); 14, 15 and 16 trees -- a batch not full, full, and one tree in a second batch with D waiting on the device --
    against the host's bits"""
    N = 4000
    batch = api.coalrate_batch_trees(N)
    assert batch == (2 << 20) // ((2 * N - 1) * 12 + N * 9 + 8) == 15
    rng = np.random.default_rng(N)
    parents = np.stack([cc.random_tree(N, rng) for _ in range(batch + 1)])
    bl = np.stack([cc.dated_lengths(N, rng) for _ in parents])
    factors = rng.uniform(0.0, 9000.0, batch + 1).astype(np.float32)
    ep = host_tests.epochs_of(3)
    Ds, secs = on_device(tmp_path, parents, bl, factors, ep, counts=[batch - 1, batch, batch + 1])
    for c, D in zip((batch - 1, batch, batch + 1), Ds):
        assert cc.same_bits(D, api.coalrate_trees(parents[:c], bl[:c], factors[:c], ep)), c
    bigtile.record("coalescent_rate/N4000_batches", dict(N=N, E=3, trees=[batch - 1, batch, batch + 1], device_call_seconds=secs))


def test_fixture_cases_on_the_device(tmp_path):
    """rl_coalrate_anc on the device on the three fixture cases: the reference's .bin bytes (a real dated tree
    sequence; the synthetic case, default epochs and --bins) and the md5 of every plane (N = 300, 40 trees)"""
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path)], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().split() == ["equal", "a", "equal", "b", "equal", "c"]


def test_cli_on_the_device(tmp_path):
    """`Relate --mode CoalescentRateForSection --device 0` and `--mode FinalizePopulationSize` on case (a): out.bin and
    out.coal are the reference's bytes"""
    host_tests.run_cli(cc.fixture(), tmp_path, 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))


def test_documented_maximum(tmp_path):
    """N = 10,240 with E = 3 (D is 1.26 GB), the largest N the device takes: 20 rows per workgroup, 113 KB of LDS in a
    workgroup of 1024 threads, internal labels up to 10,238 in 16 bits.  A caterpillar and a random tree against the
    restatement over all of D, bit for bit (the restatement takes a few seconds per tree on the CPU; the device call
    is recorded)."""
    N = 10240
    rng = np.random.default_rng(N)
    parents = np.stack([cc.caterpillar(N), cc.random_tree(N, rng)])
    bl = np.stack([cc.dated_lengths(N, rng) for _ in parents])
    check(tmp_path, "N10240_E3", parents, bl, [812.5, 3.0], host_tests.epochs_of(3), host=False)


def test_refusals_on_the_device(tmp_path):
    """N = 10,241 and E = 65 are RL_EINVAL with the limit in the message; a negative branch length and a node with three
    children are named by tree and node before anything of their batch is added; the process goes on to a correct
    small case"""
    parents, bl, factors = host_tests.case(9, 2)
    ep = host_tests.epochs_of(4)
    neg = bl.copy()
    neg[2, 4] = -0.5
    ternary = parents.copy()
    ternary[1, 0] = ternary[1, 2]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npy")
    np.savez(src, big=cc.caterpillar(10241)[None], parents=parents, bl=bl, factors=factors, epochs=ep, neg=neg, ternary=ternary)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 4 and all(ln.startswith("refused:") for ln in lines), lines
    assert "10240" in lines[0] and "N=10241" in lines[0]
    assert "64" in lines[1] and "65 given" in lines[1]
    assert "tree 2" in lines[2] and "node 4" in lines[2] and "negative" in lines[2]
    assert "tree 1" in lines[3]
    assert cc.same_bits(np.load(dst), cc.reference_bins(parents, bl, factors, ep))
