"""CompareTopology on the host (rl_compare_trees / rl_compare_anc with device < 0, `Relate --mode CompareTopology
--device -1`) against the definition restated by brute force (compare_cases.py: sets of frozensets of leaves, a
per-SNP walk of the two sequences).  Every comparison is exact: the metric is an integer, the mean a double summed
in a stated order."""
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
SIZES = [2, 3, 4, 8, 64, 65, 257, 1000]


@pytest.mark.parametrize("N", SIZES)
def test_random_trees_against_the_oracle(N):
    rng = np.random.default_rng(N)
    reps = 3 if N >= 257 else 12
    A = np.stack([cc.random_tree(N, rng) for _ in range(reps)])
    B = np.stack([cc.random_tree(N, rng) for _ in range(reps)])
    want = [cc.oracle_distance(a, b) for a, b in zip(A, B)]
    got = api.compare_trees(A, B)
    assert got.dtype == np.int32 and got.tolist() == want
    assert all(0 <= d <= 2 * max(N - 2, 0) for d in want)
    # explicit pairs, one tree of A against several of B and the other way round
    pairs = [(0, k) for k in range(reps)] + [(k, 0) for k in range(reps)] + [(reps - 1, reps - 1)]
    assert api.compare_trees(A, B, pairs).tolist() == [cc.oracle_distance(A[i], B[j]) for i, j in pairs]


@pytest.mark.parametrize("N", SIZES)
def test_identity_and_symmetry(N):
    rng = np.random.default_rng(100 + N)
    A = np.stack([cc.random_tree(N, rng) for _ in range(4)])
    B = np.stack([cc.random_tree(N, rng) for _ in range(4)])
    assert not api.compare_trees(A, A).any()
    # the same clades under other labels of the internal nodes
    assert not api.compare_trees(A, np.stack([cc.relabel(a[::1]) for a in A])).any()
    assert api.compare_trees(A, B).tolist() == api.compare_trees(B, A).tolist()


@pytest.mark.parametrize("N", [4, 8, 64, 65, 257, 1000])
def test_caterpillar_against_balanced(N):
    rng = np.random.default_rng(200 + N)
    cat, bal = cc.caterpillar(N), cc.balanced(N)
    shuffled = cc.caterpillar(N, rng.permutation(N))
    A, B = np.stack([cat, bal, cat, shuffled]), np.stack([bal, cat, shuffled, bal])
    want = [cc.oracle_distance(a, b) for a, b in zip(A, B)]
    assert api.compare_trees(A, B).tolist() == want
    assert want[0] == want[1] and want[0] > 0


@pytest.mark.parametrize("N", [3, 4, 8, 64, 65, 257, 1000])
def test_one_interchange_is_a_distance_of_two(N):
    rng = np.random.default_rng(300 + N)
    for _ in range(5):
        a = cc.random_tree(N, rng)
        b = cc.nni(a, rng)
        assert cc.oracle_distance(a, b) == 2
        assert api.compare_trees(a, b).tolist() == [2]


def fixture_sequences(tmp_path):
    """synth24's BuildTopology trees as one sequence, and a copy with other boundaries and a few other trees"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "synth24.npz"))
    W = int(z["meta"][2])
    N, seq_a = None, []
    for w in range(W):
        N, trees = cc.read_anc(z["anc/%d" % w].tobytes())
        seq_a += [(pos, parent) for pos, parent, _, _ in trees]
        end = trees[-1][3]
    assert N == 24 and len(seq_a) > W and all(seq_a[t][0] < seq_a[t + 1][0] for t in range(len(seq_a) - 1))
    rng = np.random.default_rng(24)
    seq_b = []
    for t, (pos, parent) in enumerate(seq_a):
        if t % 3 == 1:
            continue  # this tree's SNPs fall to the tree before it
        if t % 3 == 2:
            pos += 1  # a boundary one SNP later
        if t % 4 == 0:
            parent = cc.nni(parent, rng)
        if t % 10 == 5:
            parent = cc.random_tree(N, rng)
        seq_b.append((pos, parent))
    seq_b.insert(3, ((seq_b[2][0] + seq_b[3][0]) // 2, cc.nni(seq_b[2][1], rng)))  # a boundary A does not have
    assert all(seq_b[t][0] < seq_b[t + 1][0] for t in range(len(seq_b) - 1))
    fa, fb = str(tmp_path / "a.anc"), str(tmp_path / "b.anc")
    cc.write_anc(fa, N, seq_a, end)
    cc.write_anc(fb, N, seq_b, end - 7)  # ... and B stops earlier
    return N, fa, fb, seq_a, end, seq_b, end - 7


def test_two_anc_files_with_other_boundaries(tmp_path):
    N, fa, fb, seq_a, end_a, seq_b, end_b = fixture_sequences(tmp_path)
    rows, want = cc.oracle_compare(N, seq_a, end_a, seq_b, end_b)
    assert len(rows) > max(len(seq_a), len(seq_b)) and 0 < want["share_identical"] < 1
    got = api.compare_anc(fa, fb)
    cc.check_summary(got, rows, want)
    assert sum(r[1] - r[0] for r in rows) == want["snp_end"] - want["snp_begin"]
    # the other way round: the same intervals with the trees swapped
    back = api.compare_anc(fb, fa)
    assert back["per_interval"][:, [0, 1, 3, 2, 4]].tolist() == rows and back["mean_normalised"] == want["mean_normalised"]
    # a file against itself
    same = api.compare_anc(fa, fa)
    assert same["max_distance"] == 0 and same["share_identical"] == 1.0 and same["mean_normalised"] == 0.0
    assert same["intervals"] == len(seq_a)


def test_cli_on_the_host(tmp_path):
    N, fa, fb, seq_a, end_a, seq_b, end_b = fixture_sequences(tmp_path)
    rows, want = cc.oracle_compare(N, seq_a, end_a, seq_b, end_b)
    p = subprocess.run([CLI, "--mode", "CompareTopology", "-i", "a.anc,b.anc", "-o", "out", "--device", "-1"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    said = dict(line.split() for line in p.stdout.decode().splitlines())
    assert int(said["haplotypes"]) == N and int(said["intervals"]) == len(rows)
    assert int(said["max_distance"]) == want["max_distance"] and int(said["snps_identical"]) == want["snps_identical"]
    assert float(said["mean_normalised_distance"]) == want["mean_normalised"]  # (%.17g round-trips a double)
    assert float(said["share_identical"]) == want["share_identical"]
    assert np.loadtxt(str(tmp_path / "out.cmp"), dtype=np.int64, ndmin=2).tolist() == rows
    # without -o: the summary alone
    p = subprocess.run([CLI, "--mode", "CompareTopology", "-i", "a.anc,b.anc", "--device", "-1"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout.decode().splitlines()[0] == "haplotypes 24"
    assert sorted(os.listdir(str(tmp_path))) == ["a.anc", "b.anc", "out.cmp"]
    assert "CompareTopology" in subprocess.run([CLI, "--help"], stderr=subprocess.PIPE).stderr.decode()


def test_refusals(tmp_path):
    lib = api.lib()
    rng = np.random.default_rng(5)
    # a parent whose label is not above its child's: nodes 8 and 9 of a 6-leaf tree trade labels
    good = cc.caterpillar(6)
    bad = good.copy()
    bad[[8, 9]] = bad[[9, 8]]
    bad[bad == 8], bad[bad == 9] = -9, 8
    bad[bad == -9] = 9
    assert cc.oracle_distance(good, bad) == 0 and bad[9] == 8  # the same tree, labelled the other way
    for a, b, which in ((bad, good, "A"), (good, bad, "B")):
        with pytest.raises(api.RelateError) as e:
            api.compare_trees(a, b)
        assert "error -1" in str(e.value) and "of %s" % which in str(e.value) and "label above" in str(e.value)
    # not binary / a leaf as a parent / out of range / two roots
    for spoil in ({6: 8}, {0: 1}, {0: 99}, {0: -1}):
        t = good.copy()
        for v, p in spoil.items():
            t[v] = p
        with pytest.raises(api.RelateError):
            api.compare_trees(good, t)
    with pytest.raises(api.RelateError):
        api.compare_trees(cc.random_tree(8, rng), cc.random_tree(9, rng))
    # .anc files: other N, ranges that do not meet, a file that is not there -- messages, not crashes
    cc.write_anc(str(tmp_path / "n8.anc"), 8, [(0, cc.random_tree(8, rng)), (10, cc.random_tree(8, rng))], 19)
    cc.write_anc(str(tmp_path / "n9.anc"), 9, [(0, cc.random_tree(9, rng))], 19)
    cc.write_anc(str(tmp_path / "late.anc"), 8, [(20, cc.random_tree(8, rng))], 30)
    cc.write_anc(str(tmp_path / "touch.anc"), 8, [(19, cc.random_tree(8, rng))], 30)
    for other, msg in (("n9.anc", "haplotypes"), ("late.anc", "do not overlap"), ("nothing.anc", "cannot open")):
        with pytest.raises(api.RelateError) as e:
            api.compare_anc(str(tmp_path / "n8.anc"), str(tmp_path / other))
        assert msg in str(e.value), str(e.value)
        p = subprocess.run([CLI, "--mode", "CompareTopology", "-i", "n8.anc," + other, "--device", "-1"],
                           cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and msg in p.stderr.decode() and not p.stdout
    one = api.compare_anc(str(tmp_path / "n8.anc"), str(tmp_path / "touch.anc"))  # one SNP in common
    assert (one["snp_begin"], one["snp_end"], one["intervals"]) == (19, 20, 1)
    p = subprocess.run([CLI, "--mode", "CompareTopology", "--device", "-1"], stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"a.anc,b.anc" in p.stderr
    assert lib.rl_compare_trees(None, None, 8, 1, None, -1, None) == -1
