"""PairwiseCoalescence on the host (rl_pairwise_trees / rl_pairwise_anc with device < 0, `Relate --mode
PairwiseCoalescence --device -1`) against the definition restated in Python (pairwise_cases.py).  Every comparison
is exact: uint64 sums against Python ints, double sums against Python floats added in the same order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pairwise_cases as pc
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
METRICS = ["size", "time"]


def case(N, seed):
    """the shapes with unequal weights, one of them zero -> [(parent, branch_length, weight)]"""
    rng = np.random.default_rng(seed)
    trees = pc.shapes(N, rng)
    weights = [7, 1, 0, 1000003, 12, 5]
    return [(p, pc.branch_lengths(N, rng), w) for p, w in zip(trees, weights)]


def call(trees, metric, device=None):
    return api.pairwise_trees(np.stack([t[0] for t in trees]), [t[2] for t in trees],
                              np.stack([t[1] for t in trees]) if metric == "time" else None, metric, device)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N", [2, 3, 8, 70])
def test_sums_against_the_oracle(N, metric):
    trees = case(N, N)
    want, W = pc.oracle_sum(trees, metric)
    S, gotW = call(trees, metric)
    assert S.dtype == (np.uint64 if metric == "size" else np.float64) and S.shape == (N, N)
    assert gotW == W == sum(t[2] for t in trees)
    assert S.tolist() == want  # equal, not close
    assert np.array_equal(S, S.T) and not S.diagonal().any()
    if metric == "size":
        assert S[np.triu_indices(N, 1)].min() >= 2 * W and S.max() <= N * W
    # one tree alone, and no tree at all
    one, w1 = call(trees[3:4], metric)
    assert one.tolist() == pc.oracle_sum(trees[3:4], metric)[0] and w1 == trees[3][2]
    none, w0 = api.pairwise_trees(np.zeros((0, 2 * N - 1), np.int32), [], np.zeros((0, 2 * N - 1)), metric)
    assert w0 == 0 and not none.any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N", [2, 3, 9, 40])
def test_reference_equals_the_oracle(N, metric):
    """the numpy reference of the large device tests against the Python-set oracle, element by element"""
    trees = case(N, N)
    want, W = pc.oracle_sum(trees, metric)
    S, gotW = pc.reference_sum(trees, metric, N)
    assert S.dtype == (np.uint64 if metric == "size" else np.float64) and S.shape == (N, N)
    assert gotW == W and S.tolist() == want  # equal, not close
    big = [(t[0], t[1], w) for t, w in zip(trees, (2 ** 31, 2 ** 33 + 1, 5))]  # sums beyond 32 bits
    S, gotW = pc.reference_sum(big, metric, N)
    want, W = pc.oracle_sum(big, metric)
    assert gotW == W and S.tolist() == want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N", [1537, 3511])
def test_host_equals_the_reference(N, metric):
    """the host implementation above toy size against something that does not share its design: four and seven rows
    per row block, a caterpillar, its reverse, a balanced tree and a random one, a zero weight and one above 2^32"""
    trees = list(zip(*[pc.large_case(N)[k] for k in (0, 2, 1)]))  # (parent, branch_length, weight)
    want, W = pc.reference_sum(trees, metric, N)
    S, gotW = call(trees, metric)
    assert gotW == W == sum(pc.LARGE_WEIGHTS) > 2 ** 32
    assert S.dtype == want.dtype and np.array_equal(S.view(np.uint64), want.view(np.uint64))  # equal bits
    assert np.array_equal(S, S.T) and not S.diagonal().any()


def test_weights_beyond_32_bits():
    """w * N summed over trees passes 2^32: 32-bit accumulators are wrong"""
    rng = np.random.default_rng(31)
    trees = [(pc.random_tree(8, rng), pc.branch_lengths(8, rng), w) for w in (2 ** 31, 2 ** 31, 5)]
    want, W = pc.oracle_sum(trees, "size")
    assert W == 2 ** 32 + 5 and sum(v > 2 ** 32 for row in want for v in row) > 8
    S, gotW = call(trees, "size")
    assert gotW == W and [[int(v) for v in row] for row in S] == want
    T, _ = call(trees, "time")
    assert T.tolist() == pc.oracle_sum(trees, "time")[0]


def two_files(tmp_path, N=8):
    rng = np.random.default_rng(77)
    a = [(pos, pc.random_tree(N, rng), pc.branch_lengths(N, rng)) for pos in (0, 3, 4, 40)]
    b = [(pos, pc.random_tree(N, rng), pc.branch_lengths(N, rng)) for pos in (55, 56, 90)]
    pc.write_anc(str(tmp_path / "a.anc"), N, a, 54)
    pc.write_anc(str(tmp_path / "b.anc"), N, b, 120)
    seq = lambda trees, end: [(p, bl, w) for (_, p, bl), w in zip(trees, pc.file_weights(trees, end))]  # noqa: E731
    return seq(a, 54), seq(b, 120)


@pytest.mark.parametrize("metric", METRICS)
def test_two_anc_files_in_both_orders(tmp_path, metric):
    a, b = two_files(tmp_path)
    assert [t[2] for t in a] == [3, 1, 36, 15] and [t[2] for t in b] == [1, 34, 31]  # the last SNP included
    fa, fb = str(tmp_path / "a.anc"), str(tmp_path / "b.anc")
    ab, Wab = api.pairwise_anc([fa, fb], metric)
    ba, Wba = api.pairwise_anc([fb, fa], metric)
    assert Wab == Wba == 121
    assert ab.tolist() == pc.oracle_sum(a + b, metric)[0]
    assert ba.tolist() == pc.oracle_sum(b + a, metric)[0]  # time: the oracle evaluated in THAT order
    if metric == "size":
        assert np.array_equal(ab, ba)
    alone, Wa = api.pairwise_anc(fa, metric)
    assert Wa == 55 and alone.tolist() == pc.oracle_sum(a, metric)[0]


@pytest.mark.parametrize("metric", METRICS)
def test_cli_on_the_host(tmp_path, metric):
    a, b = two_files(tmp_path)
    want, W = pc.oracle_sum(a + b, metric)
    p = subprocess.run([CLI, "--mode", "PairwiseCoalescence", "-i", "a.anc,b.anc", "-o", "out", "--metric", metric,
                        "--device", "-1"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == pc.oracle_summary(want, W, metric, 2, 7)
    assert open(str(tmp_path / "out.pwc"), "rb").read() == pc.pwc_bytes(want, W, metric)
    assert sorted(os.listdir(str(tmp_path))) == ["a.anc", "b.anc", "out.pwc"]


def test_cli_defaults_and_refusals(tmp_path):
    a, _ = two_files(tmp_path)
    run = lambda *args: subprocess.run([CLI, "--mode", "PairwiseCoalescence"] + list(args), cwd=str(tmp_path),  # noqa: E731
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    helped = subprocess.run([CLI, "--help"], stderr=subprocess.PIPE).stderr.decode()
    assert "PairwiseCoalescence" in helped and "--metric size|time" in helped
    for args in (["-o", "out", "--device", "-1"], ["-i", "a.anc", "--device", "-1"]):  # no -i, no -o
        p = run(*args)
        assert p.returncode == 1 and b"a.anc[,b.anc,...]" in p.stderr and not p.stdout
    p = run("-i", "a.anc", "-o", "out", "--metric", "depth", "--device", "-1")
    assert p.returncode == 1 and b"--metric must be size or time" in p.stderr and not p.stdout
    p = run("-i", "a.anc,nothing.anc", "-o", "out", "--device", "-1")
    assert p.returncode == 1 and b"cannot open" in p.stderr and not p.stdout
    assert not os.path.exists(str(tmp_path / "out.pwc"))
    # the metric defaults to size
    p = run("-i", "a.anc", "-o", "dflt", "--device", "-1")
    assert p.returncode == 0, p.stderr.decode()
    want, W = pc.oracle_sum(a, "size")
    assert p.stdout.decode().splitlines() == pc.oracle_summary(want, W, "size", 1, 4)
    assert open(str(tmp_path / "dflt.pwc"), "rb").read() == pc.pwc_bytes(want, W, "size")


def test_refusals(tmp_path):
    lib = api.lib()
    rng = np.random.default_rng(5)
    good = pc.caterpillar(6)
    bl = pc.branch_lengths(6, rng)
    # a parent whose label is not above its child's: nodes 8 and 9 trade labels
    bad = good.copy()
    bad[[8, 9]] = bad[[9, 8]]
    bad[bad == 8], bad[bad == 9] = -9, 8
    bad[bad == -9] = 9
    with pytest.raises(api.RelateError) as e:
        api.pairwise_trees(np.stack([good, good, bad]), [1, 1, 1])
    assert "error -1" in str(e.value) and "tree 2" in str(e.value) and "label above" in str(e.value)
    assert bad[9] == 8 and "node 9" in str(e.value)
    # not binary: node 6 gets a third child
    three = good.copy()
    three[0] = 7
    with pytest.raises(api.RelateError) as e:
        api.pairwise_trees(np.stack([good, three]), [1, 1])
    assert "error -1" in str(e.value) and "tree 1" in str(e.value) and "node" in str(e.value)
    for spoil in ({0: 1}, {0: 99}, {0: -1}):  # a leaf as a parent / out of range / two roots
        t = good.copy()
        for v, p in spoil.items():
            t[v] = p
        with pytest.raises(api.RelateError):
            api.pairwise_trees(t, [1])
    with pytest.raises(api.RelateError) as e:  # time without branch lengths
        api.pairwise_trees(good, [1], metric="time")
    assert "branch lengths" in str(e.value)
    with pytest.raises(api.RelateError) as e:
        api.pairwise_trees(good, [-1])
    assert "negative" in str(e.value)
    with pytest.raises(api.RelateError):  # an unknown metric
        api.pairwise_trees(good, [1], metric="depth")
    S, W = np.zeros((6, 6), np.uint64), C.c_longlong(0)
    w1 = np.ones(1, np.int64)
    args = (good.ctypes.data_as(C.c_void_p), None, w1.ctypes.data_as(C.c_void_p), 6, 1)
    assert lib.rl_pairwise_trees(*args, 7, -1, S.ctypes.data_as(C.c_void_p), C.byref(W)) == -1
    assert b"metric 7" in lib.rl_last_error()
    assert lib.rl_pairwise_trees(*args, 0, -1, None, C.byref(W)) == -1
    assert lib.rl_pairwise_trees(*args, 0, -1, S.ctypes.data_as(C.c_void_p), C.byref(W)) == 0 and W.value == 1
    # files: other N, sample ages with time (fine with size), a file that is not there
    t8 = [(0, pc.random_tree(8, rng), pc.branch_lengths(8, rng)), (10, pc.random_tree(8, rng), pc.branch_lengths(8, rng))]
    pc.write_anc(str(tmp_path / "n8.anc"), 8, t8, 19)
    pc.write_anc(str(tmp_path / "n9.anc"), 9, [(20, pc.random_tree(9, rng), None)], 30)
    pc.write_anc(str(tmp_path / "aged.anc"), 8, t8, 19, ages=np.arange(8.0))
    for paths, metric, msg in ((["n8.anc", "n9.anc"], "size", "haplotypes"), (["n8.anc", "aged.anc"], "time", "sample ages"),
                               (["n8.anc", "nothing.anc"], "size", "cannot open")):
        with pytest.raises(api.RelateError) as e:
            api.pairwise_anc([str(tmp_path / f) for f in paths], metric)
        assert msg in str(e.value), str(e.value)
    aged, W = api.pairwise_anc(str(tmp_path / "aged.anc"), "size")
    plain, _ = api.pairwise_anc(str(tmp_path / "n8.anc"), "size")
    assert W == 20 and np.array_equal(aged, plain)
