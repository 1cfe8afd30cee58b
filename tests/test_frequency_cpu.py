"""Frequency on the host (rl_frequency_* with device < 0, `Relate --mode Frequency --device -1`): the reference's walk
restated in relate_amd/csrc/frequency.cpp against what the reference's RelateSelection wrote
(tests/golden/selection_ref.npz) and, on tie-free trees, against the closed form restated in numpy
(frequency_cases.py).  Every comparison is of integers or bytes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import coalrate_cases as cc
import frequency_cases as fc
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def epochs_of(E):
    """E boundaries: the default ones (31), or 0 and E - 1 boundaries spread over the times of dated_lengths"""
    if E == 31:
        return api.coalrate_epochs()
    return np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1)))).astype(np.float32)


def case_inputs(fx, key):
    """-> (N, trees [(pos, parent, bl)], .anc bytes, .mut bytes, --bins or None) of a fixture case"""
    co = cc.fixture()
    bins = fc.BINS if key == "b_bins" else None
    if key in ("a", "b", "b_bins"):
        tag = key[0]
        anc = co[tag + "/anc"].tobytes()
        N, parents, bl = cc.parse_anc_text(anc)
        return N, [(0, p, b) for p, b in zip(parents, bl)], anc, co[tag + "/mut"].tobytes(), bins
    if key == "s":
        N, trees = fc.case_s_rows(co)
    else:
        N = 16
        trees = list(zip(fx["tie/pos"].tolist(), fx["tie/parents"].astype(np.int32), fx["tie/bl"].astype(np.float64)))
    rows = fc.mut_rows_from_arrays({"rows": fx[key + "/rows"], "ages": fx[key + "/ages"]})
    return N, trees, cc.anc_text(N, trees), fc.mut_text(rows), bins


def write_inputs(tmp_path, fx, key):
    N, trees, anc, mut, bins = case_inputs(fx, key)
    prefix = str(tmp_path / key)
    open(prefix + ".anc", "wb").write(anc)
    open(prefix + ".mut", "wb").write(mut)
    return prefix, bins


def check_fixture_case(fx, tmp_path, key, device):
    """rl_frequency_anc on a fixture case: the reference's .freq and .lin bytes -> (rows, trees walked on the host)"""
    prefix, bins = write_inputs(tmp_path, fx, key)
    ep = api.coalrate_epochs(bins=bins)
    out = str(tmp_path / (key + "_out"))
    rows, host_trees = api.frequency_anc(prefix + ".anc", prefix + ".mut", ep, out + ".freq", out + ".lin", device)
    assert open(out + ".freq", "rb").read() == fx[key + "/freq"].tobytes()
    assert open(out + ".lin", "rb").read() == fx[key + "/lin"].tobytes()
    assert rows == fx[key + "/freq"].tobytes().count(b"\n") - 1
    return rows, host_trees


def generated(N, seed, E):
    """the shapes at N with dated lengths -> (parents, bl, epochs), every tree tie-free"""
    rng = np.random.default_rng(seed)
    parents = np.stack(fc.shapes(N, rng))
    bl = np.stack([fc.dated_lengths(N, rng) for _ in parents])
    assert all(fc.tie_free(p, b) for p, b in zip(parents, bl))
    return parents, bl, epochs_of(E)


def all_branches(parents, limit, rng):
    """(snp_tree, snp_branch): every branch of every tree up to `limit` per tree, -1 and the root among them"""
    nodes = parents.shape[1]
    st, sb = [], []
    for t in range(len(parents)):
        br = np.arange(-1, nodes) if nodes + 1 <= limit else np.concatenate(([-1, nodes - 1, 0, nodes - 2], rng.integers(0, nodes - 1, limit - 4)))
        st += [t] * len(br)
        sb += br.tolist()
    return np.array(st, np.int32), np.array(sb, np.int32)


def check_against_closed_form(parents, bl, ep, st, sb, got):
    freq, lin, marks, root_time, _ = got
    nodes = parents.shape[1]
    assert np.array_equal(marks, (sb != -1) & (sb != nodes - 1))
    assert np.array_equal(root_time, np.array([fc.max_times(p, b)[-1] for p, b in zip(parents, bl)], np.float32))
    for s in np.flatnonzero(marks):
        f, l, half, freq2 = fc.closed_form(parents[st[s]], bl[st[s]], int(sb[s]), ep)
        assert freq[s].tolist() == f + [0], (s, st[s], sb[s])
        assert lin[s].tolist() == l + [half, freq2], (s, st[s], sb[s])


@pytest.mark.parametrize("key", fc.CASES)
def test_anc_equals_the_reference(fx, tmp_path, key):
    rows, host_trees = check_fixture_case(fx, tmp_path, key, None)
    assert host_trees > 0 and rows > 0


def test_the_fixture_cases_are_what_they_claim(fx):
    """a, b and s are tie-free (the device may answer them alone), the tie case is not; s holds rows the filter drops
    and a tree without SNPs; the closed form writes the reference's bytes of s"""
    for key in ("a", "b", "s", "tie"):
        N, trees, anc, mut, _ = case_inputs(fx, key)
        assert all(fc.tie_free(p, b) for _, p, b in trees) == (key != "tie"), key
    N, trees, _, _, _ = case_inputs(fx, "s")
    rows = fc.mut_rows_from_arrays({"rows": fx["s/rows"], "ages": fx["s/ages"]})
    assert 7 not in {r[2] for r in rows} and any(len(r[3]) == 2 for r in rows) and any(r[4] for r in rows)
    assert any(r[3] == [2 * N - 2] for r in rows) and any(r[3] == [-1] for r in rows)
    freq, lin = fc.files_by_closed_form(N, trees, rows, api.coalrate_epochs())
    assert freq == fx["s/freq"].tobytes() and lin == fx["s/lin"].tobytes()
    assert len(rows) > freq.count(b"\n") - 1  # the filter dropped some


@pytest.mark.parametrize("N,E", [(2, 31), (3, 2), (3, 31), (9, 3), (9, 64), (65, 2), (65, 31), (130, 64), (300, 31)])
def test_host_walk_equals_the_closed_form(N, E):
    parents, bl, ep = generated(N, 100 * N + E, E)
    st, sb = all_branches(parents, 140, np.random.default_rng(N))
    got = api.frequency_trees(parents, bl, st, sb, ep)
    assert got[4] == len(parents)
    check_against_closed_form(parents, bl, ep, st, sb, got)


def test_closed_form_on_a_tree_done_by_hand():
    """((0,1),(2,3)) with t(4) = 5, t(5) = 12 (its longer child decides), t(6) = 30 and the boundaries 0, 10, 20, 40:
    a SNP on node 5 (DAF 2) has one carrier between 30 and 12 and two below"""
    parent, bl = [4, 4, 5, 5, 6, 6, -1], [5.0, 3.0, 7.0, 12.0, 25.0, 10.0, 0.0]
    ep = np.array([0.0, 10.0, 20.0, 40.0], np.float32)
    assert fc.max_times(parent, bl).tolist() == [0, 0, 0, 0, 5, 12, 30]
    want = ([0, 1, 2, 2], [0, 2, 3, 4], -1, 3)
    assert fc.closed_form(parent, bl, 5, ep) == want
    freq, lin, marks, root_time, _ = api.frequency_trees(parent, bl, [0], [5], ep)
    assert freq[0].tolist() == want[0] + [0] and lin[0].tolist() == want[1] + [-1, 3] and marks[0] and root_time[0] == 30.0


def test_a_time_on_a_boundary_and_a_young_root():
    """an internal time set exactly to a boundary is not above it; a root younger than several boundaries writes 0
    lineages there"""
    N = 9
    rng = np.random.default_rng(5)
    parent = fc.caterpillar(N)
    bl = fc.dated_lengths(N, rng, top=8.0)
    t = fc.max_times(parent, bl)  # (a caterpillar: the times rise with the label)
    assert fc.tie_free(parent, bl)
    ep = np.array([0.0, t[N + 2], t[N + 5], t[-1], t[-1] * 2, t[-1] * 4, 1e9], np.float32)
    st, sb = all_branches(parent[None], 100, rng)
    got = api.frequency_trees(parent, bl, st, sb, ep)
    check_against_closed_form(parent[None], bl[None], ep, st, sb, got)
    assert got[1][2].tolist()[:3] == [0, 0, 0] and got[1][2][3] == 1  # t(root) == ep[3]: one lineage, not above


def run_cli(fx, tmp_path, key, device, run=None):
    """`Relate --mode Frequency` on a fixture case: the reference's two files and banner"""
    if run is None:
        def run(cmd, cwd):
            return subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    _, bins = write_inputs(tmp_path, fx, key)
    cmd = [CLI, "--mode", "Frequency", "-i", key, "-o", "out_" + key, "--device", str(device)] + (["--bins", bins] if bins else [])
    p = run(cmd, str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()
    assert ("Calculating frequency through time for %s.\n" % key).encode() in p.stderr and b"CPU Time spent" in p.stderr
    assert open(str(tmp_path / ("out_" + key + ".freq")), "rb").read() == fx[key + "/freq"].tobytes()
    assert open(str(tmp_path / ("out_" + key + ".lin")), "rb").read() == fx[key + "/lin"].tobytes()
    return p


@pytest.mark.parametrize("key", fc.CASES)
def test_cli_on_the_host(fx, tmp_path, key):
    run_cli(fx, tmp_path, key, -1)


def test_cli_help_names_the_modes():
    helped = subprocess.run([CLI, "--help"], stderr=subprocess.PIPE).stderr.decode()
    assert "Frequency: -i,--input prefix" in helped and "Selection: -i,--input prefix" in helped


def test_refusals(tmp_path, fx):
    parents, bl, ep = generated(9, 1, 4)
    st, sb = np.array([0, 2, 2], np.int32), np.array([3, 9, 12], np.int32)
    for bad_ep, word in ((np.zeros(1, np.float32), "64"), (np.arange(65, dtype=np.float32), "64"),
                         (np.array([0, 5, 5, 9], np.float32), "boundary 2"), (np.array([1, 5, 9], np.float32), "not 0")):
        with pytest.raises(api.RelateError, match=word):
            api.frequency_trees(parents, bl, st, sb, bad_ep)
    neg = bl.copy()
    neg[2, 4] = -1e-9
    with pytest.raises(api.RelateError, match="tree 2.*node 4"):
        api.frequency_trees(parents, neg, st, sb, ep)
    neg[2, 4] = np.nan
    with pytest.raises(api.RelateError, match="tree 2.*node 4"):
        api.frequency_trees(parents, neg, st, sb, ep)
    low = parents.copy()
    low[2, 12] = 10  # node 12's parent below it
    with pytest.raises(api.RelateError, match="tree 2.*label above"):
        api.frequency_trees(low, bl, st, sb, ep)
    with pytest.raises(api.RelateError, match="must not fall"):
        api.frequency_trees(parents, bl, [2, 0], [3, 3], ep)
    with pytest.raises(api.RelateError, match="branch 17"):
        api.frequency_trees(parents, bl, [0], [17], ep)
    # files: sample ages in the header, a .mut whose tree indices fall, a compressed input, frequency columns
    prefix, _ = write_inputs(tmp_path, fx, "b")
    out = str(tmp_path / "o")
    eps = api.coalrate_epochs()
    anc = open(prefix + ".anc", "rb").read()
    head, rest = anc.split(b"\n", 1)
    open(prefix + "_ages.anc", "wb").write(head + b" " + b" ".join([b"0"] * 23 + [b"100.5"]) + b"\n" + rest)
    with pytest.raises(api.RelateError, match="sample ages"):
        api.frequency_anc(prefix + "_ages.anc", prefix + ".mut", eps, out + ".freq", out + ".lin")
    lines = open(prefix + ".mut", "rb").read().split(b"\n")
    falls = lines[:]
    falls[4], falls[5] = falls[5], falls[4]
    assert falls[4].split(b";")[4] > falls[5].split(b";")[4]
    open(prefix + "_falls.mut", "wb").write(b"\n".join(falls))
    with pytest.raises(api.RelateError, match="must not fall"):
        api.frequency_anc(prefix + ".anc", prefix + "_falls.mut", eps, out + ".freq", out + ".lin")
    annotated = [lines[0]] + [ln + b"N;N;3;0;12;" if ln else ln for ln in lines[1:]]
    open(prefix + "_annot.mut", "wb").write(b"\n".join(annotated))
    with pytest.raises(api.RelateError, match="population-frequency columns"):
        api.frequency_anc(prefix + ".anc", prefix + "_annot.mut", eps, out + ".freq", out + ".lin")
    with gzip.open(prefix + "_z.anc.gz", "wb") as f:
        f.write(anc)
    with pytest.raises(api.RelateError, match="compressed"):
        api.frequency_anc(prefix + "_z.anc", prefix + ".mut", eps, out + ".freq", out + ".lin")
    # and the process goes on to a correct answer
    st, sb = all_branches(parents, 100, np.random.default_rng(0))
    check_against_closed_form(parents, bl, ep, st, sb, api.frequency_trees(parents, bl, st, sb, ep))
