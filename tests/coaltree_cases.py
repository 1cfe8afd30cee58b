"""The oracle of the CoalRateForTree tests (test_coaltree_cpu.py, test_coaltree_gpu.py).  Nothing here calls the
library: the definition of include/relate_amd.h (rl_coaltree_trees) is restated as the closed form over the sorted
times of the INTERNAL nodes alone -- no sort of all 2N-1 nodes, no lineage table, no cursor --, and
tests/golden/coaltree_ref.npz (tools/make_golden_coaltree.py) holds what the reference's RelateCoalescentRate wrote in
--mode CoalRateForTree and what its coal_tree held in every block after the last tree, to the bit."""
import bisect
import os

import numpy as np

import coalrate_cases as cc
from coalrate_cases import balanced, caterpillar, dated_lengths, random_tree, shapes  # noqa: F401  (the tests' trees)
from frequency_cases import clock_lengths, max_times, tie_trees  # noqa: F401
from mutrate_cases import default_epochs, young_trees  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "coaltree_ref.npz")
BLOCK_SIZE = 1000  # the reference's
# the fixture's cases -> (--bins, --years_per_gen)
CASES = {"a": (None, None), "b": (None, None), "b_bins": (cc.BINS, None), "tie": (None, None), "on": (None, "8"),
         "young": ("6.5,7.5,0.5", "1e6"), "many": (None, None)}


def fixture():
    return np.load(FIXTURE)


def num_blocks(ntrees, block_size=BLOCK_SIZE):
    return int(ntrees / float(block_size) + 1)


def tree_terms(parent, bl, factor, epochs):
    """one tree by the closed form -> (q, terms, exits): q = bases / 1e9, what every internal node inside the
    boundaries adds to num of its epoch; terms[j]: what the nodes of epoch j add to denom, in sorted order; exits[j]:
    the exit term of epoch j, +0.0 where the walk does not leave it.  With S the sorted float times of the internal
    nodes and S[-1] = 0: node k lies in epoch j with ep[j] < S[k] <= ep[j+1] (time 0: epoch 0; above ep[E-1]: none)
    and its term is bases * n * (n-1) / 2.0 * (S[k] - max(S[k-1], ep[j])) / 1e9 with n = N - k; epoch j has an exit
    term if a node time exceeds ep[j+1]: with k* the first such node, n = N - k* and the width ep[j+1] - max(S[k*-1],
    ep[j]).  Python floats: every operation is one IEEE double operation, left to right"""
    N = (len(parent) + 1) // 2
    ep = [float(x) for x in epochs]
    E = len(ep)
    S = [float(x) for x in np.sort(max_times(parent, bl)[N:])]  # float32 values, widened exactly
    bases = float(np.float32(factor))
    terms = [[] for _ in range(E)]
    for k, s in enumerate(S):
        i = bisect.bisect_left(ep, s, 1)  # the first boundary from 1 on that is not below s
        if i == E:
            continue
        n, lower = N - k, max(S[k - 1] if k else 0.0, ep[i - 1])
        terms[i - 1].append(bases * n * (n - 1) / 2.0 * (s - lower) / 1e9)
    exits = [0.0] * E
    for j in range(E - 1):
        k = bisect.bisect_right(S, ep[j + 1])  # the first node above ep[j+1]
        if k < len(S):
            n, lower = N - k, max(S[k - 1] if k else 0.0, ep[j])
            exits[j] = bases * n * (n - 1) / 2.0 * (ep[j + 1] - lower) / 1e9
    return bases / 1e9, terms, exits


def block_sums(parents, bl, factors, epochs, block_size=BLOCK_SIZE):
    """the accumulators of every block after the last tree -> (num, denom) [blocks][E] float64: one serial sum per
    block and epoch through the block's trees in order -- per tree the node terms one by one, then the exit term"""
    E = len(epochs)
    blocks = num_blocks(len(parents), block_size)
    num, denom = [[0.0] * E for _ in range(blocks)], [[0.0] * E for _ in range(blocks)]
    for t, (p, b, f) in enumerate(zip(parents, bl, factors)):
        q, terms, exits = tree_terms(p, b, f, epochs)
        nu, de = num[t // block_size], denom[t // block_size]
        for j in range(E):
            for x in terms[j]:
                nu[j] += q
                de[j] += x
            de[j] += exits[j]
    return np.array(num, np.float64).reshape(blocks, E), np.array(denom, np.float64).reshape(blocks, E)


def rates(num, denom):
    """coal_tree::Dump's rule over the blocks added in order -> (num [E], denom [E], rates [E])"""
    n, d = np.zeros(num.shape[1]), np.zeros(num.shape[1])
    for b in range(len(num)):
        n, d = n + num[b], d + denom[b]
    r = np.zeros(len(n))
    for i in range(len(n)):
        if d[i] != 0:
            r[i] = n[i] / d[i]
        elif i > 0:
            r[i] = r[i - 1]
    return n, d, r


def trees_with_times(N, times, rng, pos=0):
    """a random tree whose internal nodes have exactly the float32 times given (sorted here; node N gets the
    smallest): labels rise from child to parent, so every branch length, the difference of two float32 times taken
    in double, is >= 0 -> (pos, parent, bl)"""
    t = np.concatenate((np.zeros(N, np.float32), np.sort(np.asarray(times, np.float32))))
    assert len(t) == 2 * N - 1
    parent = random_tree(N, rng)
    bl = np.zeros(2 * N - 1, np.float64)
    for v in range(2 * N - 2):
        bl[v] = np.float64(t[parent[v]]) - np.float64(t[v])
    assert np.array_equal(max_times(parent, bl), t)
    return pos, parent, bl


def on_boundary_trees():
    """N = 16 under --years_per_gen 8, whose default boundaries 1e3 / 8 = 125 and 1e8 / 8 = 12,500,000 are float32
    values: node times exactly ON the first boundary (alone, tied, after nodes at 0, as the first node of all), on
    the last (the root; the root and the node before it), one float32 step to either side of both, and a root above
    the last"""
    N, rng = 16, np.random.default_rng(125)
    lo, hi = np.float32(125.0), np.float32(12500000.0)
    up, down = (lambda x: np.nextafter(x, np.float32(np.inf))), (lambda x: np.nextafter(x, np.float32(0)))
    mid = np.exp(rng.uniform(np.log(200.0), np.log(1e7), (8, N - 1))).astype(np.float32)
    rows = []
    for k, m in enumerate(mid):
        m = np.sort(m)
        if k == 0:
            m[:3], m[-1] = [0, 0, lo], hi
        elif k == 1:
            m[:4], m[-2:] = [lo, lo, lo, up(lo)], [hi, hi]
        elif k == 2:
            m[:3], m[-1] = [down(lo), lo, up(lo)], up(hi)
        elif k == 3:
            m[0], m[-2:] = lo, [down(hi), hi]
        elif k == 4:
            m[:2], m[-1] = [1.5, lo], 2.0e7
        elif k == 5:
            m[:] = lo
        elif k == 6:
            m[:-1], m[-1] = lo, hi
        else:
            m[:] = hi
        rows.append(trees_with_times(N, m, rng, pos=30 * k))
    return N, rows


def many_trees():
    """N = 5, 3000 random dated trees: the reference's blocks of 1000 are crossed twice and the fourth block, which
    (int)(3000 / 1000.0 + 1) makes room for, stays empty"""
    N, T = 5, 3000
    rng = np.random.default_rng(3000)
    return N, [(10 * k, random_tree(N, rng), dated_lengths(N, rng)) for k in range(T)]


def mut_rows(ntrees, rng, skip=(), first_pos=100):
    """a .mut for cc.mut_text: one to three SNPs per tree, none on the trees of `skip` -> [(pos, dist, tree)]"""
    rows, pos = [], first_pos
    for t in range(ntrees):
        if t in skip:
            continue
        for _ in range(int(rng.integers(1, 4))):
            dist = int(rng.integers(1, 9000))
            rows.append((pos, dist, t))
            pos += dist
    return rows


def case_inputs(fx, key):
    """-> (N, parents [T][2N-1] int32, bl [T][2N-1] float64, factors [T] float32, .anc bytes, .mut bytes) of a case"""
    if key in ("a", "b", "b_bins"):
        co = cc.fixture()
        anc, mut = co[key[0] + "/anc"].tobytes(), co[key[0] + "/mut"].tobytes()
        N, parents, bl = cc.parse_anc_text(anc)
        rows = cc.parse_mut_text(mut)
    else:
        parents, bl = fx[key + "/parents"].astype(np.int32), fx[key + "/bl"].astype(np.float64)
        N = (parents.shape[1] + 1) // 2
        rows = [tuple(r) for r in fx[key + "/mut"].tolist()]
        anc = cc.anc_text(N, list(zip(fx[key + "/pos"].tolist(), parents, bl)))
        mut = cc.mut_text(rows)
    factors = np.array(cc.mut_factors(rows, len(parents)), np.float32)
    return N, parents, bl, factors, anc, mut
