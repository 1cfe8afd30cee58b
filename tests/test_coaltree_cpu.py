"""CoalRateForTree on the host (rl_coaltree_* with device < 0, `Relate --mode CoalRateForTree --device -1`): the
reference's coal_tree::populate restated in relate_amd/csrc/coaltree.cpp against what the reference's coal_tree held
in every block in full precision and what its RelateCoalescentRate wrote (tests/golden/coaltree_ref.npz), and against
the closed form over the internal times restated in numpy (coaltree_cases.py).  Every comparison is of bits or bytes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import coaltree_cases as ct
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
KEYS = tuple(ct.CASES)


@pytest.fixture(scope="module")
def fx():
    return ct.fixture()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def epochs_of(key):
    bins, ypg = ct.CASES[key]
    return api.mutrate_epochs(float(ypg) if ypg else 28.0, bins)


def write_inputs(tmp_path, fx, key):
    """-> the prefix of key.anc and key.mut"""
    _, _, _, _, anc, mut = ct.case_inputs(fx, key)
    prefix = str(tmp_path / key)
    open(prefix + ".anc", "wb").write(anc)
    open(prefix + ".mut", "wb").write(mut)
    return prefix


def check_blocks(fx, key, device):
    """rl_coaltree_trees with the reference's block size on a fixture case: the harness's doubles in every block"""
    _, parents, bl, factors, _, _ = ct.case_inputs(fx, key)
    num, denom = api.coaltree_trees(parents, bl, factors, fx[key + "/epochs"], device=device)
    assert same_bits(num, fx[key + "/num"]) and same_bits(denom, fx[key + "/denom"])
    assert not num[:, -1].any() and not denom[:, -1].any()
    return num, denom


def check_fixture_case(fx, tmp_path, key, device):
    """rl_coaltree_anc, rl_coaltree_rates and rl_coaltree_write on a fixture case: the harness's blocks added in
    order, to the bit, and the reference's bytes"""
    prefix = write_inputs(tmp_path, fx, key)
    ep = epochs_of(key)
    num, denom, ntrees = api.coaltree_anc(prefix + ".anc", prefix + ".mut", ep, device)
    want_num, want_denom, want_rates = ct.rates(fx[key + "/num"], fx[key + "/denom"])
    assert same_bits(num, want_num) and same_bits(denom, want_denom)
    rates = api.coaltree_rates(num, denom)
    assert same_bits(rates, want_rates)
    out = str(tmp_path / (key + ".coal"))
    api.coaltree_write(out, ep, rates)
    assert open(out, "rb").read() == fx[key + "/coal"].tobytes()
    return ntrees


@pytest.mark.parametrize("key", KEYS)
def test_epochs_equal_the_reference(fx, key):
    """the boundaries of CoalescenceRateForTree are rl_mutrate_epochs': doubles, bit for bit"""
    assert same_bits(epochs_of(key), fx[key + "/epochs"])


@pytest.mark.parametrize("key", KEYS)
def test_host_twin_equals_the_harness(fx, key):
    check_blocks(fx, key, None)


@pytest.mark.parametrize("key", KEYS)
def test_anc_equals_the_reference(fx, tmp_path, key):
    assert check_fixture_case(fx, tmp_path, key, None) == len(ct.case_inputs(fx, key)[1])


def test_the_fixture_cases_are_what_they_claim(fx):
    """tie: equal times and internal nodes at 0; on: node times exactly on the first and the last boundary and a root
    above the last; young: a root inside epoch 0, roots above the last boundary; many: blocks of 1000 crossed, the
    fourth block empty, trees without SNPs; b: a tree without SNPs"""
    _, parents, bl, _, _, _ = ct.case_inputs(fx, "tie")
    times = [ct.max_times(p, b)[16:] for p, b in zip(parents, bl)]
    assert any((t == 0).any() for t in times) and any(len(np.unique(t)) < len(t) for t in times)
    _, parents, bl, _, _, _ = ct.case_inputs(fx, "on")
    ep = fx["on/epochs"]
    times = np.stack([ct.max_times(p, b)[16:] for p, b in zip(parents, bl)]).astype(np.float64)
    assert (times == ep[1]).any() and (times == ep[-1]).any() and (times[:, -1] > ep[-1]).any() and (times == 0).any()
    assert (times[5] == ep[1]).all() and (times[7] == ep[-1]).all()
    _, parents, bl, _, _, _ = ct.case_inputs(fx, "young")
    roots = [ct.max_times(p, b)[-1] for p, b in zip(parents, bl)]
    ep = fx["young/epochs"]
    assert roots[0] < ep[1] and roots[1] > ep[-1] and min(ct.max_times(parents[3], bl[3])[16:]) > ep[-1]
    _, parents, _, factors, _, _ = ct.case_inputs(fx, "many")
    assert len(parents) == 3000 and fx["many/num"].shape == (4, 31) and fx["many/num"][:3].any(1).all()
    assert not fx["many/num"][3].any() and not fx["many/denom"][3].any()
    assert factors[0] == 0 and factors[999] == 0 and factors[1000] == 0 and factors[1] > 0
    assert ct.case_inputs(fx, "b")[3][4] == 0


def random_case(N, E, seed, trees=None):
    rng = np.random.default_rng(seed)
    parents = np.stack(ct.shapes(N, rng))
    if trees:
        parents = parents[np.arange(trees) % len(parents)]
    bl = np.stack([ct.dated_lengths(N, rng) for _ in parents])
    factors = rng.integers(0, 20000, len(parents)).astype(np.float32) / np.float32(2)
    ep = ct.default_epochs() if E == 31 else np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1))))
    return parents, bl, factors, ep


@pytest.mark.parametrize("N,E", [(2, 31), (3, 2), (3, 31), (9, 3), (9, 64), (65, 2), (65, 31), (130, 64), (300, 31)])
def test_host_twin_equals_the_closed_form(N, E):
    parents, bl, factors, ep = random_case(N, E, 100 * N + E)
    num, denom = api.coaltree_trees(parents, bl, factors, ep)
    want_num, want_denom = ct.block_sums(parents, bl, factors, ep)
    assert num.shape == (1, E) and same_bits(num, want_num) and same_bits(denom, want_denom)


@pytest.mark.parametrize("block_size", [1, 3, 50])
def test_block_edges(block_size):
    """10 trees in blocks of 1 (11 blocks, the last empty), of 3 (4 blocks) and of 50 (one block)"""
    parents, bl, factors, ep = random_case(24, 31, block_size, trees=10)
    num, denom = api.coaltree_trees(parents, bl, factors, ep, block_size)
    want_num, want_denom = ct.block_sums(parents, bl, factors, ep, block_size)
    assert len(num) == api.coaltree_num_blocks(10, block_size) == {1: 11, 3: 4, 50: 1}[block_size]
    assert same_bits(num, want_num) and same_bits(denom, want_denom)
    if block_size == 1:
        assert not num[10].any() and not denom[10].any() and denom[:10].any(1).all()


def boundary_cases():
    """the tie trees (times are multiples of 100) under boundaries that node times fall on exactly, in runs of
    neighbouring boundaries and with boundaries skipped, under one that crosses several empty epochs, with the root
    above the last boundary, with every node in one epoch, and with every epoch empty but the first and the last"""
    trees = ct.tie_trees(16, 12, 3) + ct.tie_trees(16, 6, 4)
    parents, bl = np.stack([t[1] for t in trees]), np.stack([t[2] for t in trees])
    factors = np.arange(1, len(parents) + 1).astype(np.float32) * np.float32(1234.5)
    eps = [np.array(e, np.float64) for e in (
        [0, 100, 200, 400, 1e6], [0, 200, 400, 500, 1e6], [0, 50, 100, 150, 200, 250, 300, 350, 1e4],
        [0, 100, 100.5, 101, 101.5, 102, 199, 200, 1e5], [0, 300], [0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1e-3, 1e5, 1e6, 1e7],
        [0, 1e9], [0, 1e-3, 2e-3, 3e-3, 1e9], [0, 50, 1e9, 2e9, 3e9, 4e9])]
    return parents, bl, factors, eps


def test_times_on_boundaries_and_empty_epochs():
    parents, bl, factors, eps = boundary_cases()
    for ep in eps:
        num, denom = api.coaltree_trees(parents, bl, factors, ep, 4)
        want_num, want_denom = ct.block_sums(parents, bl, factors, ep, 4)
        assert same_bits(num, want_num) and same_bits(denom, want_denom), ep


def test_a_node_on_a_boundary_belongs_to_the_epoch_below():
    """((0,1),2) with t(3) = 0.1f and t(4) = 0.3f, bases = 2e9 so that bases / 1e9 = 2: with a boundary exactly on
    t(3) the node is counted in epoch 0 and epoch 0 gets its whole width from it, an exit term of width 0 included;
    one float32 step below t(3) the node is counted in epoch 1"""
    a, b = np.float32(0.1), np.float32(0.3)
    parent, bl = [3, 3, 4, 4, -1], [float(a), float(a), float(b), float(np.float64(b) - np.float64(a)), 0.0]
    assert ct.max_times(parent, bl).tolist() == [0, 0, 0, a, b]
    A, B = float(a), float(b)
    num, denom = api.coaltree_trees(parent, bl, [2e9], [0.0, A, 1.0, 2.0])
    assert num.tolist() == [[2.0, 2.0, 0.0, 0.0]]
    assert denom.tolist() == [[2e9 * 3 * 2 / 2.0 * (A - 0.0) / 1e9, 2e9 * 2 * 1 / 2.0 * (B - A) / 1e9, 0.0, 0.0]]
    below = float(np.nextafter(a, np.float32(0)))
    num, denom = api.coaltree_trees(parent, bl, [2e9], [0.0, below, 1.0, 2.0])
    assert num.tolist() == [[0.0, 4.0, 0.0, 0.0]]
    assert denom.tolist() == [[2e9 * 3 * 2 / 2.0 * (below - 0.0) / 1e9,
                               2e9 * 3 * 2 / 2.0 * (A - below) / 1e9 + 2e9 * 2 * 1 / 2.0 * (B - A) / 1e9, 0.0, 0.0]]


def test_rates_rule():
    """num / denom where denom != 0, otherwise the rate before it, 0 at the start"""
    r = api.coaltree_rates([1.0, 2.0, 3.0, 0.0, 5.0, 0.0], [0.0, 4.0, 0.0, 0.0, 2.0, 0.0])
    assert r.tolist() == [0.0, 0.5, 0.5, 0.5, 2.5, 2.5]


def run_cli(fx, tmp_path, key, device, run=None):
    """`Relate --mode CoalRateForTree` on a fixture case: the reference's file and banner, a summary on stdout"""
    if run is None:
        def run(cmd, cwd):
            return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    bins, ypg = ct.CASES[key]
    write_inputs(tmp_path, fx, key)
    cmd = [CLI, "--mode", "CoalRateForTree", "-i", key, "-o", "out_" + key, "--device", str(device)] \
        + (["--bins", bins] if bins else []) + (["--years_per_gen", ypg] if ypg else [])
    p = run(cmd, str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert ("Calculating coalescence rates for %s...\n" % key).encode() in p.stderr and b"CPU Time spent" in p.stderr
    trees = len(fx[key + "/parents"]) if key + "/parents" in fx.files else {"a": 355, "b": 6, "b_bins": 6}[key]
    assert ("%d trees in %d blocks" % (trees, len(fx[key + "/num"]))).encode() in p.stdout
    assert ("%d of %d epochs" % ((fx[key + "/denom"].sum(0) != 0).sum(), len(fx[key + "/epochs"]))).encode() in p.stdout
    assert open(str(tmp_path / ("out_" + key + ".coal")), "rb").read() == fx[key + "/coal"].tobytes()
    return p


@pytest.mark.parametrize("key", KEYS)
def test_cli_on_the_host(fx, tmp_path, key):
    run_cli(fx, tmp_path, key, -1)


def test_cli_help_and_refusals(fx, tmp_path):
    helped = subprocess.run([CLI, "--help"], stderr=subprocess.PIPE).stderr.decode()
    assert "CoalRateForTree: -i,--input prefix" in helped
    write_inputs(tmp_path, fx, "b")
    for opt, val in (("--dist", "b.dist"), ("--chr", "chr.txt")):
        p = subprocess.run([CLI, "--mode", "CoalRateForTree", "-i", "b", "-o", "o", "--device", "-1", opt, val],
                           cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and opt.encode() in p.stderr and not os.path.exists(str(tmp_path / "o.coal"))


def test_refusals(tmp_path, fx):
    parents, bl, factors, ep = random_case(9, 31, 1)
    for bad_ep, word in ((np.zeros(1), "64"), (np.arange(65.0), "65 given"), (np.array([0, 5, 5, 9.0]), "boundary 2"),
                         (np.array([1, 5, 9.0]), "not 0")):
        with pytest.raises(api.RelateError, match=word):
            api.coaltree_trees(parents, bl, factors, bad_ep)
    with pytest.raises(api.RelateError, match="10240.*N=10241"):
        api.coaltree_trees(ct.caterpillar(10241), np.ones(2 * 10241 - 1), [1.0], ep)
    with pytest.raises(api.RelateError, match="N=1"):
        api.coaltree_trees([-1], [0.0], [1.0], ep)
    for bad in (-1.0, np.nan, np.inf):
        f = factors.copy()
        f[3] = bad
        with pytest.raises(api.RelateError, match="tree 3.*factor"):
            api.coaltree_trees(parents, bl, f, ep)
    neg = bl.copy()
    neg[2, 4] = -1e-9
    with pytest.raises(api.RelateError, match="tree 2.*node 4.*negative"):
        api.coaltree_trees(parents, neg, factors, ep)
    low = parents.copy()
    low[2, 12] = 10  # node 12's parent below it
    with pytest.raises(api.RelateError, match="tree 2.*label above"):
        api.coaltree_trees(low, bl, factors, ep)
    with pytest.raises(api.RelateError, match="block size"):
        api.coaltree_trees(parents, bl, factors, ep, 0)
    # files: sample ages in the header, compressed inputs
    prefix = write_inputs(tmp_path, fx, "tie")
    anc = open(prefix + ".anc", "rb").read()
    head, rest = anc.split(b"\n", 1)
    open(prefix + "_ages.anc", "wb").write(head + b" " + b" ".join([b"0"] * 15 + [b"100.5"]) + b"\n" + rest)
    with pytest.raises(api.RelateError, match="sample ages"):
        api.coaltree_anc(prefix + "_ages.anc", prefix + ".mut", ep)
    for ext in (".anc", ".mut"):
        with gzip.open(prefix + "_z" + ext + ".gz", "wb") as f:
            f.write(open(prefix + ext, "rb").read())
    with pytest.raises(api.RelateError, match="_z.anc.gz: compressed"):
        api.coaltree_anc(prefix + "_z.anc", prefix + ".mut", ep)
    with pytest.raises(api.RelateError, match="_z.mut.gz: compressed"):
        api.coaltree_anc(prefix + ".anc", prefix + "_z.mut", ep)
    with pytest.raises(api.RelateError, match="_z.anc.gz is compressed"):
        api.coaltree_anc(prefix + "_z.anc.gz", prefix + ".mut", ep)
    # and the process goes on to a correct answer
    check_blocks(fx, "tie", None)
