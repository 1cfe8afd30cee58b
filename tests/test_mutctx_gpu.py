"""MutationRateWithContext on the device (relate_amd/csrc/mutctx_kernels.hip and the root times out of
mutrate_kernels.hip) against the host twin and what the reference wrote (tests/golden/mutctx_ref.npz): equal bits and
bytes throughout, no time asserted (the device calls' seconds go to the test report).  Every step that uses the GPU is
a child process under a time limit of its own; after one that was killed, aborted or timed out no further step is
started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import mutctx_cases as xc
import mutrate_cases as mc
import test_mutctx_cpu as host_tests
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
D = api.MUTCTX_DEPTH

# the jobs of an .npz (parents<i>, bl<i>, tree<i>, counts<i>, ep<i>) one after another in one process
CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
out = {}
for i in range(int(z["jobs"])):
    t0 = time.perf_counter()
    out["opp%d" % i], out["roots%d" % i], out["parts%d" % i] = api.mutctx_trees(
        z["parents%d" % i], z["bl%d" % i], z["tree%d" % i], z["counts%d" % i], z["ep%d" % i], device=0, details=True)
    print("seconds", time.perf_counter() - t0)
np.savez(sys.argv[3], **out)
"""

CHILD_FILES = """
import pathlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import mutctx_cases as xc
import test_mutctx_cpu as host_tests
fx = xc.fixture()
for key in sys.argv[4:]:
    snps = host_tests.check_fixture_case(fx, pathlib.Path(sys.argv[3]), key, 0)
    print("equal", key, snps[2])
"""

CHILD_REFUSED = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
def refused(*a):
    try:
        api.mutctx_trees(*a, device=0)
        print("accepted")
    except api.RelateError as e:
        print("refused:", e)
for name in sys.argv[4:]:
    refused(z[name + "_parents"], z[name + "_bl"], z[name + "_tree"], z[name + "_counts"], z[name + "_ep"])
np.savez(sys.argv[3], out=api.mutctx_trees(z["parents"], z["bl"], z["tree"], z["counts"], z["ep"], device=0))  # the process is healthy
"""


def on_device(tmp_path, jobs, seconds=120):
    """jobs = [(parents, bl, snp_tree, counts, epochs)] -> [(opportunity, roots)] of the device, one process"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {"jobs": len(jobs)}
    for i, job in enumerate(jobs):
        for name, a in zip(("parents", "bl", "tree", "counts", "ep"), job):
            arrays["%s%d" % (name, i)] = a
    np.savez(src, **arrays)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    secs = [float(ln.split()[1]) for ln in p.stdout.decode().splitlines() if ln.startswith("seconds")]
    z = np.load(dst)
    return [(z["opp%d" % i], z["roots%d" % i], z["parts%d" % i]) for i in range(len(jobs))], secs


def check(tmp_path, key, jobs):
    """device == host twin on every job: the opportunity to the bit, the root times"""
    got, secs = on_device(tmp_path, jobs)
    for (parents, bl, tree, counts, ep), (opp, roots, parts) in zip(jobs, got):
        want, want_roots, _ = api.mutctx_trees(parents, bl, tree, counts, ep, details=True)
        assert opp.dtype == np.float64 and opp.shape == (len(ep), 96) and host_tests.same_bits(opp, want), (key, len(tree))
        assert roots.dtype == np.float32 and np.array_equal(roots.view(np.uint32), want_roots.view(np.uint32))
        assert not opp[-1].any()
    bigtile.record("mutctx/" + key, dict(N=(np.atleast_2d(jobs[0][0]).shape[1] + 1) // 2, jobs=len(jobs),
                                         snps=[len(j[2]) for j in jobs], device_call_seconds=secs,
                                         trees_copies_chains_seconds=[g[2].tolist() for g in got]))
    return got


def snps_on(ntrees, S, rng, top=50):
    """S SNPs over the trees in order; rows of small counts with an all-zero row and a row with one nonzero count"""
    tree = np.sort(rng.integers(0, ntrees, S)).astype(np.int32)
    counts = rng.integers(0, top, (S, 96)).astype(np.uint32)
    counts[rng.integers(0, 3, (S, 96)) == 0] = 0
    if S > 2:
        counts[1] = 0
        counts[2] = 0
        counts[2, 95] = 7
    return tree, counts


@pytest.mark.parametrize("E", [2, 31, 64])
def test_device_equals_host_twin(tmp_path, E):
    """192 cells (three full wavefronts), 2976 (a partial last one) and 6144; no SNP, one, and every remainder of the
    in-flight depth: depth - 1, depth, depth + 1, two depths + 1"""
    rng = np.random.default_rng(E)
    parents, bl = host_tests.small_trees(12, 5, E)
    ep = mc.default_epochs() if E == 31 else np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1))))
    jobs = [(parents, bl) + snps_on(5, S, rng) + (ep,) for S in (0, 1, D - 1, D, D + 1, 2 * D + 1)]
    got = check(tmp_path, "E%d" % E, jobs)
    assert not got[0][0].any() and got[1][0].any() and (got[5][0][0] > 0.0).sum() > 48
    # and the definition itself, SNP by SNP
    assert host_tests.same_bits(got[4][0], host_tests.opportunity_by_hand(parents, bl, jobs[4][2], jobs[4][3], ep))


def big_trees(N, ntrees, seed):
    rng = np.random.default_rng(seed)
    base = np.stack(mc.shapes(N, rng, randoms=1))
    parents = base[np.arange(ntrees) % len(base)]
    bl = np.stack([mc.dated_lengths(N, rng) for _ in range(ntrees)])
    return parents, bl


def test_a_second_batch_and_a_second_chunk(tmp_path):
    """N = 4000: a batch is 21 trees, so 23 trees are two batches and the accumulators persist from one to the next;
    the SNPs of the first batch all sit on its last tree.  And more SNPs than one launch of the chains kernel takes"""
    N = 4000
    batch = api.mutrate_batch_trees(N)
    assert batch == 21
    parents, bl = big_trees(N, batch + 2, N)
    rng = np.random.default_rng(1)
    _, counts = snps_on(1, 3 * D + 5, rng)
    tree = np.array([batch - 1] * (2 * D + 2) + [batch] * 2 + [batch + 1] * (D + 1), np.int32)
    small_p, small_b = host_tests.small_trees(12, 3, 9)
    many = api.MUTCTX_SNP_CHUNK + D + 3
    jobs = [(parents, bl, tree, counts, mc.default_epochs()), (small_p, small_b) + snps_on(3, many, rng) + (mc.default_epochs(),)]
    got = check(tmp_path, "batches_and_chunks", jobs)
    assert got[0][0][:-1].all()
    only_second = api.mutctx_trees(parents[batch:], bl[batch:], tree[2 * D + 2:] - batch, counts[2 * D + 2:], mc.default_epochs())
    assert not host_tests.same_bits(got[0][0], only_second)  # (the first batch's sums are in it)


def test_counts_near_2_to_31_and_lengths_of_every_magnitude(tmp_path):
    """counts around 2^31 and 2^32 - 1 next to counts of 1, trees whose lengths span twenty binades: a sum that was
    re-associated, or a product contracted into the sum, shows in the last bits"""
    rng = np.random.default_rng(31)
    N, T, S = 20, 6, 4 * D + 3
    parents = np.stack([mc.random_tree(N, rng) for _ in range(T)])
    bl = np.exp(rng.uniform(-6.0, 8.0, (T, 2 * N - 1))) * np.array([1e-3, 1.0, 1e3, 1e-2, 1e2, 1.0])[:, None]
    tree = np.sort(rng.integers(0, T, S)).astype(np.int32)
    pool = np.array([1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 0, 12345], np.uint32)
    counts = pool[rng.integers(0, len(pool), (S, 96))]
    ep = np.concatenate(([0.0], np.exp(np.linspace(-8.0, 12.0, 30))))
    got = check(tmp_path, "magnitudes", [(parents, bl, tree, counts, ep)])
    fused = np.zeros((len(ep), 96), np.longdouble)  # what a sum without the roundings in between would hold
    lengths = api.mutrate_trees(parents, bl, ep)
    for t, row in zip(tree, counts):
        fused = fused + lengths[t][:, None].astype(np.longdouble) * row.astype(np.longdouble)[None, :]
    assert not host_tests.same_bits(got[0][0], fused.astype(np.float64))


@pytest.mark.parametrize("N", [2, 2049])
def test_root_time_out_of_both_instantiations(tmp_path, N):
    """the per-tree kernel with 256 threads (N = 2: one internal node) and with 1024 (N = 2049)"""
    rng = np.random.default_rng(N)
    parents = np.stack(mc.shapes(N, rng, randoms=1))[:3]
    bl = np.stack([mc.dated_lengths(N, rng) for _ in parents])
    got = check(tmp_path, "roots_N%d" % N, [(parents, bl) + snps_on(len(parents), D + 2, rng) + (mc.default_epochs(),)])
    assert np.array_equal(got[0][1], np.array([mc.max_times(p, b)[-1] for p, b in zip(parents, bl)], np.float32))


def test_refusals_on_the_device(tmp_path):
    """N = 10,241 and E = 65 are RL_EINVAL with the limit in the message, before any launch; a tree the device refuses
    in the SECOND batch is named; the process goes on to a correct small case"""
    N = 4000
    batch = api.mutrate_batch_trees(N)
    parents, bl = big_trees(N, batch + 2, 7)
    neg = bl.copy()
    neg[batch + 1, 4] = -0.5
    rng = np.random.default_rng(2)
    tree, counts = snps_on(batch + 2, D + 1, rng)
    sp, sb = host_tests.small_trees(9, 4, 1)
    st, sc = snps_on(4, 2 * D, rng)
    ep = mc.default_epochs()
    arrays = dict(parents=sp, bl=sb, tree=st, counts=sc, ep=ep)
    for name, job in (("second", (parents, neg, tree, counts, ep)),
                      ("big", (mc.caterpillar(10241)[None], np.ones((1, 20481)), st[:1] * 0, sc[:1], ep)),
                      ("wide", (sp, sb, st, sc, np.arange(65.0)))):
        for part, a in zip(("parents", "bl", "tree", "counts", "ep"), job):
            arrays[name + "_" + part] = a
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    p = gpu_step([sys.executable, "-c", CHILD_REFUSED, ROOT, src, dst, "second", "big", "wide"], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 3 and all(ln.startswith("refused:") for ln in lines), lines
    assert "tree %d" % (batch + 1) in lines[0] and "node 4" in lines[0] and "negative" in lines[0]
    assert "10240" in lines[1] and "N=10241" in lines[1]
    assert "64" in lines[2] and "65 given" in lines[2]
    assert host_tests.same_bits(np.load(dst)["out"], api.mutctx_trees(sp, sb, st, sc, ep))


def test_fixture_cases_on_the_device(tmp_path):
    """every fixture case through rl_mutctx_anc on the device: the reference's _mut.bin, _opp.bin and .rate"""
    keys = list(xc.CASES)
    p = gpu_step([sys.executable, "-c", CHILD_FILES, ROOT, TESTS, str(tmp_path)] + keys, 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = p.stdout.decode().split()
    assert out[0::3] == ["equal"] * len(keys) and out[1::3] == keys and all(int(m) > 0 for m in out[2::3])


@pytest.mark.parametrize("key", list(xc.CASES))
def test_cli_on_the_device(tmp_path, key):
    """`Relate --mode MutationRateWithContext --device 0`: the reference's files and banner"""
    host_tests.run_cli(xc.fixture(), tmp_path, key, 0, run=lambda cmd, cwd: gpu_step(cmd, 120, cwd=cwd))
