"""Frequency on the device (relate_amd/csrc/frequency_kernels.hip) against the host walk, the closed form restated in
frequency_cases.py and the reference's files (tests/golden/selection_ref.npz): equal integers and bytes throughout, no
time asserted (the device calls' seconds go to the test report).  Every step that uses the GPU is a child process
under a time limit of its own; after one that was killed, aborted or timed out no further step is started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import frequency_cases as fc
import test_frequency_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SMALL_N = 2048  # kFrequencySmallN: above it a workgroup is 1024 threads, not 256

CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
t0 = time.perf_counter()
freq, lin, marks, root_time, host_trees = api.frequency_trees(z["parents"], z["bl"], z["st"], z["sb"], z["epochs"], device=0)
print("seconds", time.perf_counter() - t0)
np.savez(sys.argv[3], freq=freq, lin=lin, marks=marks, root_time=root_time, host_trees=host_trees)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import frequency_cases as fc
import test_frequency_cpu as host_tests
fx = fc.fixture()
for key in sys.argv[4:]:
    rows, host_trees = host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), key, 0)
    print("equal", key, host_trees)
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
        api.frequency_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
refused(z["big"], np.ones(z["big"].shape), [0], [0], ep)                      # N = 10,241
refused(z["parents"], z["bl"], z["st"], z["sb"], np.arange(65, dtype=np.float32))  # E = 65
refused(z["parents"], z["neg"], z["st"], z["sb"], ep)                         # a negative branch length in tree 2
refused(z["low"], z["bl"], z["st"], z["sb"], ep)                              # a parent below its child in tree 1
freq, lin, marks, root_time, host_trees = api.frequency_trees(z["parents"], z["bl"], z["st"], z["sb"], ep, device=0)
np.savez(sys.argv[3], freq=freq, lin=lin, marks=marks, root_time=root_time, host_trees=host_trees)  # the process is healthy
"""


def on_device(tmp_path, parents, bl, st, sb, ep, seconds=120):
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, parents=parents, bl=bl, st=st, sb=sb, epochs=ep)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    z = np.load(dst)
    return (z["freq"], z["lin"], z["marks"], z["root_time"], int(z["host_trees"])), secs[0]


def check(tmp_path, key, parents, bl, st, sb, ep, closed_form=True, host_trees=0):
    got, secs = on_device(tmp_path, parents, bl, st, sb, ep)
    want = api.frequency_trees(parents, bl, st, sb, ep)
    for g, w, name in zip(got[:4], want[:4], ("freq", "lin", "marks", "root_time")):
        keep = np.ones(len(g), bool) if name in ("marks", "root_time") else want[2]
        assert g.dtype == w.dtype and np.array_equal(g[keep], w[keep]), name
    assert got[4] == host_trees
    if closed_form:
        host_tests.check_against_closed_form(np.atleast_2d(parents), np.atleast_2d(bl), ep, st, sb, got)
    bigtile.record("frequency/" + key, dict(N=(np.atleast_2d(parents).shape[1] + 1) // 2, E=len(ep), trees=len(np.atleast_2d(parents)),
                                            snps=len(st), device_call_seconds=secs))
    return got


@pytest.mark.parametrize("N", [2, 3, 64, 65, 66, 129, 257])
def test_device_equals_host_and_closed_form(tmp_path, N):
    """the 64-lane blocks of the pull scans (63, 64, 65, 128, 256 internal nodes) and the sort's padding (a power of two
    exactly, one past it); a caterpillar, its reverse, a balanced tree and random ones; every branch of every tree up
    to N = 66 -- a leaf, a child of the root, DAF = 2 and 3 among them --, -1 and the root (no row) and 136 branches
    per tree above; several SNPs on every tree"""
    parents, bl, ep = host_tests.generated(N, 7 * N, 31)
    st, sb = host_tests.all_branches(parents, 140, np.random.default_rng(N))
    check(tmp_path, "N%d" % N, parents, bl, st, sb, ep)


@pytest.mark.parametrize("E", [2, 64])
def test_epoch_counts(tmp_path, E):
    """N = 130 with the fewest and the most boundaries; the trees 1 and 4 without SNPs"""
    parents, bl, ep = host_tests.generated(130, E, E)
    st, sb = host_tests.all_branches(parents, 60, np.random.default_rng(E))
    keep = (st != 1) & (st != 4)
    check(tmp_path, "N130_E%d" % E, parents, bl, st[keep], sb[keep], ep)


def test_boundaries_on_node_times_and_a_young_root(tmp_path):
    """boundaries set exactly to internal times (not above them), to the root's time, and several beyond the root"""
    N = 66
    rng = np.random.default_rng(66)
    parents = np.stack([fc.caterpillar(N), fc.random_tree(N, rng)])
    bl = np.stack([fc.dated_lengths(N, rng, top=8.0) for _ in parents])
    assert all(fc.tie_free(p, b) for p, b in zip(parents, bl))
    t = np.unique(np.concatenate([fc.max_times(p, b)[N:] for p, b in zip(parents, bl)]))
    top = t[-1]
    ep = np.unique(np.concatenate(([0.0], t[::9], [fc.max_times(parents[0], bl[0])[-1], fc.max_times(parents[1], bl[1])[-1]],
                                   [top * 2, top * 4, top * 8]))).astype(np.float32)
    assert len(ep) <= 64 and ep[0] == 0.0
    st, sb = host_tests.all_branches(parents, 140, rng)
    got = check(tmp_path, "boundaries", parents, bl, st, sb, ep)
    assert not got[1][st == 0][1, :3].any()  # no lineage at the three boundaries beyond every root


@pytest.mark.parametrize("N", [SMALL_N, SMALL_N + 1])
def test_both_workgroup_sizes_and_a_second_batch(tmp_path, N):
    """either side of the switch of workgroup sizes, with one tree more than a batch takes (the library's accessor says
    how many): the SNPs of the second batch are numbered from its first tree"""
    batch = api.frequency_batch_trees(N)
    assert batch == (2 << 20) // ((2 * N - 1) * 12 + 12)
    rng = np.random.default_rng(N)
    base = np.stack(fc.shapes(N, rng, randoms=1))
    parents = base[np.arange(batch + 1) % len(base)]
    bl = np.stack([fc.clock_lengths(p, rng) for p in parents])  # (dated_lengths' sums tie in float32 at this N)
    assert all(fc.tie_free(p, b) for p, b in zip(parents[:4], bl[:4]))
    st = np.repeat(np.arange(batch + 1), 2)[1:].astype(np.int32)  # one SNP on tree 0, two on the others
    sb = rng.integers(0, 2 * N - 2, len(st)).astype(np.int32)
    sb[-1], sb[-2] = 2 * N - 3, N - 1
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.0, 5.0, 30)))).astype(np.float32)  # over the times of clock_lengths
    check(tmp_path, "N%d_batches" % N, parents, bl, st, sb, ep, closed_form=False)


def test_fixture_cases_on_the_device(tmp_path):
    """rl_frequency_anc on the device: the reference's .freq and .lin bytes of a (a real dated tree sequence), b, b with
    --bins and s, none of whose trees the host walked"""
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path), "a", "b", "b_bins", "s"], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().split() == ["equal", "a", "0", "equal", "b", "0", "equal", "b_bins", "0", "equal", "s", "0"]


def test_tie_case_goes_to_the_host_walk(tmp_path):
    """trees with equal node times and internal nodes at time 0: the device hands them back, the bytes are the
    reference's"""
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path), "tie"], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = p.stdout.decode().split()
    assert out[:2] == ["equal", "tie"] and int(out[2]) > 0


def test_cli_on_the_device(tmp_path):
    """`Relate --mode Frequency --device 0` on case a: both files and the banner"""
    host_tests.run_cli(fc.fixture(), tmp_path, "a", 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))


def test_documented_maximum(tmp_path):
    """N = 10,240, the largest N the device takes: 124 KB of LDS in a workgroup of 1024 threads, a sort of 16,384 slots,
    ranks up to 10,238 in 16 bits.  A caterpillar and a random tree with a handful of SNPs against the host walk."""
    N = 10240
    rng = np.random.default_rng(N)
    parents = np.stack([fc.caterpillar(N), fc.random_tree(N, rng)])
    bl = np.stack([fc.clock_lengths(p, rng) for p in parents])  # (dated_lengths' sums tie in float32 at this N)
    assert all(fc.tie_free(p, b) for p, b in zip(parents, bl))
    st = np.repeat([0, 1], 6).astype(np.int32)
    sb = np.array([0, N + 1, 2 * N - 3, 2 * N - 4, N + 5000, N - 1, 5, N, 2 * N - 3, 2 * N - 2, N + 7000, N + 9000], np.int32)
    ep = np.concatenate(([0.0], np.exp(np.linspace(2.5, 12.5, 30)))).astype(np.float32)  # over the times of clock_lengths
    check(tmp_path, "N10240", parents, bl, st, sb, ep, closed_form=False)


def test_refusals_on_the_device(tmp_path):
    """N = 10,241 and E = 65 are RL_EINVAL with the limit in the message, before any launch; a negative branch length
    and a parent below its child are named by tree; the process goes on to a correct small case"""
    parents, bl, ep = host_tests.generated(9, 2, 4)
    st, sb = host_tests.all_branches(parents, 100, np.random.default_rng(9))
    neg = bl.copy()
    neg[2, 4] = -0.5
    low = parents.copy()
    low[1, 12] = 10
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, big=fc.caterpillar(10241)[None], parents=parents, bl=bl, st=st, sb=sb, epochs=ep, neg=neg, low=low)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 4 and all(ln.startswith("refused:") for ln in lines), lines
    assert "10240" in lines[0] and "N=10241" in lines[0]
    assert "64" in lines[1] and "65 given" in lines[1]
    assert "tree 2" in lines[2] and "node 4" in lines[2] and "negative" in lines[2]
    assert "tree 1" in lines[3] and "label above" in lines[3]
    z = np.load(dst)
    host_tests.check_against_closed_form(parents, bl, ep, st, sb, (z["freq"], z["lin"], z["marks"], z["root_time"], 0))
    assert int(z["host_trees"]) == 0
