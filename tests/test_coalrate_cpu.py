"""CoalescentRateForSection and FinalizePopulationSize on the host (rl_coalrate_* with device < 0, `Relate --mode
CoalescentRateForSection --device -1`, `--mode FinalizePopulationSize`) against the definition restated in numpy
(coalrate_cases.py) and against what the reference's RelateCoalescentRate wrote (tests/golden/coalrate_ref.npz).
Every comparison is of bits or bytes."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import coalrate_cases as cc
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


@pytest.fixture(scope="module")
def fx():
    return cc.fixture()


def epochs_of(E):
    """E boundaries: the default ones (31), or 0 and E - 1 boundaries spread over the times of dated_lengths"""
    if E == 31:
        return api.coalrate_epochs()
    return np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1)))).astype(np.float32)


def case(N, seed):
    """the shapes with the factors 0, -1 and 1e6 among ordinary ones"""
    rng = np.random.default_rng(seed)
    parents = np.stack(cc.shapes(N, rng))
    bl = np.stack([cc.dated_lengths(N, rng) for _ in parents])
    return parents, bl, np.array([1234.5, 0.0, -1.0, 1e6, 0.25, 77.0], np.float32)


def write_inputs(tmp_path, fx, tag):
    prefix = str(tmp_path / tag)
    if tag == "c":
        trees = list(zip(fx["c/pos"].tolist(), fx["c/parents"].astype(np.int32), fx["c/bl"].astype(np.float64)))
        anc, mut = cc.anc_text(300, trees), cc.mut_text([tuple(r) for r in fx["c/mut"].tolist()])
        assert hashlib.md5(anc).digest() == fx["c/anc_md5"].tobytes() and hashlib.md5(mut).digest() == fx["c/mut_md5"].tobytes()
    else:
        anc, mut = fx[tag + "/anc"].tobytes(), fx[tag + "/mut"].tobytes()
    open(prefix + ".anc", "wb").write(anc)
    open(prefix + ".mut", "wb").write(mut)
    return prefix


def check_fixture_case(fx, tmp_path, tag, device):
    """rl_coalrate_anc on a fixture case against the reference's .bin bytes (a, b, b with --bins) or md5s (c)"""
    prefix = write_inputs(tmp_path, fx, tag)
    if tag == "c":
        D = api.coalrate_anc(prefix + ".anc", prefix + ".mut", fx["c/epochs"], device)
        assert np.array_equal(cc.plane_md5(D), fx["c/plane_md5"])
        return
    ep = api.coalrate_epochs()
    assert cc.bin_bytes(ep, api.coalrate_anc(prefix + ".anc", prefix + ".mut", ep, device)) == fx[tag + "/bin"].tobytes()
    if tag == "b":
        ep = api.coalrate_epochs(bins=cc.BINS)
        assert cc.bin_bytes(ep, api.coalrate_anc(prefix + ".anc", prefix + ".mut", ep, device)) == fx["b/bin_bins"].tobytes()


def test_epochs_equal_the_references(fx):
    ep = api.coalrate_epochs()
    assert ep.dtype == np.float32 and cc.same_bits(ep, cc.parse_bin(fx["a/bin"].tobytes())[0]) and len(ep) == 31
    assert cc.same_bits(api.coalrate_epochs(28.0, cc.BINS), cc.parse_bin(fx["b/bin_bins"].tobytes())[0])
    assert cc.same_bits(ep, fx["c/epochs"])
    for bins in ("2,6", "2", "a,b,c", "2,6,0", "2,6,-1"):
        with pytest.raises(api.RelateError):
            api.coalrate_epochs(bins=bins)
    with pytest.raises(api.RelateError):
        api.coalrate_epochs(years_per_gen=0.0)


@pytest.mark.parametrize("N,E", [(2, 31), (3, 2), (3, 31), (9, 3), (9, 64), (65, 2), (65, 31), (65, 64), (300, 31)])
def test_host_twin_equals_the_restatement(N, E):
    parents, bl, factors = case(N, 100 * N + E)
    if N == 300:
        parents, bl, factors = parents[[0, 2, 3, 5]], bl[[0, 2, 3, 5]], factors[[0, 2, 3, 5]]
    ep = epochs_of(E)
    D = api.coalrate_trees(parents, bl, factors, ep)
    assert D.dtype == np.float32 and D.shape == (E, N, N)
    assert cc.same_bits(D, cc.reference_bins(parents, bl, factors, ep))
    assert not D[E - 1].any() and not np.einsum("eii->ei", D).any()  # the last plane and the diagonals stay 0
    # one tree alone, and no tree at all
    assert cc.same_bits(api.coalrate_trees(parents[3], bl[3], factors[3:4], ep), cc.reference_bins(parents[3:4], bl[3:4], factors[3:4], ep))
    assert not api.coalrate_trees(np.zeros((0, 2 * N - 1), np.int32), np.zeros((0, 2 * N - 1)), [], ep).any()


def test_restatement_on_a_tree_done_by_hand():
    """((0,1),2) with t(3) = 5 by leaf 0, t(4) = 25 by its first child in node order, leaf 2, and the boundaries 0, 10,
    20: the pair (0,1) coalesces in epoch 0, the pairs with leaf 2 past the last boundary"""
    parent, bl, ep = [3, 3, 4, 4, -1], [5.0, 7.0, 25.0, 1.0, 0.0], np.array([0.0, 10.0, 20.0], np.float32)
    want = np.zeros((3, 3, 3), np.float32)
    want[0, 0, 1], want[0, 1, 0] = 2.0, 2.0 * 5.0
    want[0, 2, 0] = want[0, 2, 1] = want[1, 2, 0] = want[1, 2, 1] = 2.0 * 10.0
    assert np.array_equal(cc.reference_bins([parent], [bl], [2.0], ep), want)
    assert np.array_equal(api.coalrate_trees(parent, bl, [2.0], ep), want)


def test_boundary_cases_of_fixture_b(fx):
    """the restatement on the synthetic case -- a time exactly on a boundary, a zero-length branch, a root past the
    last boundary, a tree without SNPs, the trailing pass -- equals the reference's .bin"""
    N, parents, bl = cc.parse_anc_text(fx["b/anc"].tobytes())
    factors = cc.mut_factors(cc.parse_mut_text(fx["b/mut"].tobytes()), len(parents))
    assert factors[4] == 0.0 and min(factors) >= 0.0
    ep = api.coalrate_epochs()
    t0 = np.float32(bl[0][0])
    assert t0 == ep[1] and (bl[0] == 0.0).sum() >= 2 and bl[2].max() > ep[30]
    P, B, F = cc.with_trailing_pass(parents, bl, factors)
    assert cc.bin_bytes(ep, cc.reference_bins(P, B, F, ep)) == fx["b/bin"].tobytes()
    assert cc.bin_bytes(ep, api.coalrate_trees(P, B, F, ep)) == fx["b/bin"].tobytes()
    # without the trailing pass the bytes differ: the pin decides
    assert cc.bin_bytes(ep, api.coalrate_trees(parents, bl, factors, ep)) != fx["b/bin"].tobytes()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_anc_equals_the_reference(fx, tmp_path, tag):
    check_fixture_case(fx, tmp_path, tag, None)


def test_bin_round_trip(tmp_path):
    parents, bl, factors = case(9, 9)
    ep = epochs_of(5)
    D = api.coalrate_trees(parents, bl, factors, ep)
    path = str(tmp_path / "x.bin")
    api.coalrate_write_bin(path, ep, D)
    assert open(path, "rb").read() == cc.bin_bytes(ep, D)
    ep2, D2 = api.coalrate_read_bin(path)
    assert cc.same_bits(ep, ep2) and cc.same_bits(D, D2)
    open(path, "wb").write(cc.bin_bytes(ep, D)[:-5])
    with pytest.raises(api.RelateError, match="x.bin"):
        api.coalrate_read_bin(path)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_finalize_equals_the_reference(fx, tmp_path, tag):
    bin_path, coal, labels = str(tmp_path / "o.bin"), str(tmp_path / "o.coal"), str(tmp_path / "o.poplabels")
    open(bin_path, "wb").write(fx[tag + "/bin"].tobytes())
    open(labels, "wb").write(fx[tag + "/poplabels"].tobytes())
    api.coalrate_finalize_files(bin_path, coal)
    assert open(coal, "rb").read() == fx[tag + "/coal"].tobytes()
    api.coalrate_finalize_files(bin_path, coal, labels)
    assert open(coal, "rb").read() == fx[tag + "/coal_groups"].tobytes()
    # the rates of the entry point are the file's numbers: one group, float sums over i < j in row order
    ep, D = cc.parse_bin(fx[tag + "/bin"].tobytes())
    rates = api.coalrate_finalize(D)
    num, den = np.zeros(len(ep), np.float32), np.zeros(len(ep), np.float32)
    for i in range(D.shape[1]):
        for j in range(i + 1, D.shape[1]):
            num[:-1] += D[:-1, i, j]
            den[:-1] += D[:-1, j, i]
    with np.errstate(invalid="ignore"):
        want = (num / den).astype(np.float64)
    assert rates.shape == (1, 1, len(ep)) and np.array_equal(rates[0, 0, :-1], want[:-1], equal_nan=True) and np.isnan(rates[0, 0, -1])
    with pytest.raises(api.RelateError, match="hap"):
        api.coalrate_finalize_files(bin_path, coal, "hap")
    with pytest.raises(api.RelateError, match="does not match"):
        open(labels, "wb").write(fx[tag + "/poplabels"].tobytes() + b"extra POPA G NA\n")
        api.coalrate_finalize_files(bin_path, coal, labels)


def test_refusals(tmp_path, fx):
    parents, bl, factors = case(9, 1)
    ep = epochs_of(4)
    for bad_ep, word in ((np.zeros(1, np.float32), "64"), (np.arange(65, dtype=np.float32), "64"),
                         (np.array([0, 5, 5, 9], np.float32), "boundary 2"), (np.array([0, 5, 3], np.float32), "boundary 2"),
                         (np.array([1, 5, 9], np.float32), "not 0"), (np.array([0, 5, np.inf], np.float32), "boundary 2")):
        with pytest.raises(api.RelateError, match=word):
            api.coalrate_trees(parents, bl, factors, bad_ep)
    neg = bl.copy()
    neg[2, 4] = -1e-9
    with pytest.raises(api.RelateError, match="tree 2.*node 4"):
        api.coalrate_trees(parents, neg, factors, ep)
    neg[2, 4] = np.nan
    with pytest.raises(api.RelateError, match="tree 2.*node 4"):
        api.coalrate_trees(parents, neg, factors, ep)
    ternary = parents.copy()
    ternary[1, 0] = ternary[1, 2]  # a node with three children, one with a single child
    with pytest.raises(api.RelateError, match="tree 1"):
        api.coalrate_trees(ternary, bl, factors, ep)
    with pytest.raises(api.RelateError, match="tree 3.*finite"):
        api.coalrate_trees(parents, bl, [1, 1, 1, np.inf, 1, 1], ep)
    # files: sample ages in the header, a .mut whose tree indices fall, a compressed input
    prefix = write_inputs(tmp_path, fx, "b")
    anc = fx["b/anc"].tobytes()
    head, rest = anc.split(b"\n", 1)
    open(prefix + "_ages.anc", "wb").write(head + b" " + b" ".join([b"0"] * 23 + [b"100.5"]) + b"\n" + rest)
    with pytest.raises(api.RelateError, match="sample ages"):
        api.coalrate_anc(prefix + "_ages.anc", prefix + ".mut", api.coalrate_epochs())
    rows = cc.parse_mut_text(fx["b/mut"].tobytes())
    rows[3], rows[4] = rows[4], rows[3]
    assert rows[3][2] > rows[4][2]
    open(prefix + "_falls.mut", "wb").write(cc.mut_text(rows))
    with pytest.raises(api.RelateError, match="must not fall"):
        api.coalrate_anc(prefix + ".anc", prefix + "_falls.mut", api.coalrate_epochs())
    import gzip
    with gzip.open(prefix + "_z.anc.gz", "wb") as f:
        f.write(anc)
    with pytest.raises(api.RelateError, match="compressed"):
        api.coalrate_anc(prefix + "_z.anc", prefix + ".mut", api.coalrate_epochs())
    # and the process goes on to a correct answer
    assert cc.same_bits(api.coalrate_trees(parents, bl, factors, ep), cc.reference_bins(parents, bl, factors, ep))


def run_cli(fx, tmp_path, device, run=None):
    """the two modes on case (a): out.bin and out.coal (without and with --poplabels) are the reference's bytes;
    run(cmd, cwd): how a command is started (the GPU suite starts it under a time limit)"""
    if run is None:
        def run(cmd, cwd):
            return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    write_inputs(tmp_path, fx, "a")
    open(str(tmp_path / "a.poplabels"), "wb").write(fx["a/poplabels"].tobytes())
    p = run([CLI, "--mode", "CoalescentRateForSection", "-i", "a", "-o", "out", "--device", str(device)], str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert b"Calculating coalescence rate for a ..." in p.stderr and b"CPU Time spent" in p.stderr
    assert open(str(tmp_path / "out.bin"), "rb").read() == fx["a/bin"].tobytes()
    for extra, key in (([], "a/coal"), (["--poplabels", "a.poplabels"], "a/coal_groups")):
        p = subprocess.run([CLI, "--mode", "FinalizePopulationSize", "-o", "out"] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)  # (no GPU in this mode)
        assert p.returncode == 0, p.stderr.decode()
        assert b"Finalizing coalescence rate..." in p.stderr
        assert open(str(tmp_path / "out.coal"), "rb").read() == fx[key].tobytes()


def test_cli_on_the_host(fx, tmp_path):
    run_cli(fx, tmp_path, -1)
    for extra, word in ((["--mask", "m.fa"], b"--mask"), (["--dist", "d.dist"], b"--dist")):
        p = subprocess.run([CLI, "--mode", "CoalescentRateForSection", "-i", "a", "-o", "out2", "--device", "-1"] + extra,
                           cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr and not os.path.exists(str(tmp_path / "out2.bin"))
