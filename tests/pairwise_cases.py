"""The oracle of the PairwiseCoalescence tests (test_pairwise_cpu.py, test_pairwise_gpu.py).  Nothing here calls the
library: the definition of include/relate_amd.h is restated with Python sets, ints and floats -- the ancestors of
every leaf, the MRCA of two leaves as the smallest label among their common ancestors (labels rise towards the root),
sizes by counting leaves, heights by the first-child recursion, sums in tree order.  That oracle is O(N^3);
reference_sum is the same definition in numpy for the sizes the device promises (N <= 10,240), held to the oracle at
small N in test_pairwise_cpu.py."""
import numpy as np

from tree_cases import balanced, caterpillar, random_tree, read_anc, shapes, write_anc  # noqa: F401  (the tests' trees and files)


def tree_values(parent, branch_length, metric):
    """-> (mrca [N][N] of labels, None on the diagonal; value per node label: leaves below it or its height)"""
    parent = [int(p) for p in parent]
    nodes = len(parent)
    N = (nodes + 1) // 2
    above = []
    for leaf in range(N):
        s, v = set(), parent[leaf]
        while v != -1:
            s.add(v)
            v = parent[v]
        above.append(s)
    mrca = [[None if i == j else min(above[i] & above[j]) for j in range(N)] for i in range(N)]
    if metric == "size":
        value = {m: sum(1 for leaf in range(N) if m in above[leaf]) for m in range(N, nodes)}
    else:
        bl = [float(x) for x in branch_length]
        first = {}
        for v, p in enumerate(parent):  # the first child in node order
            if p != -1 and p not in first:
                first[p] = v
        value = {v: 0.0 for v in range(N)}
        for m in range(N, nodes):  # children have smaller labels
            value[m] = value[first[m]] + bl[first[m]]
    return mrca, value


def oracle_sum(trees, metric):
    """trees: [(parent, branch_length or None, weight)] in order -> (S as a list of lists of Python ints (size) or
    floats (time), W)"""
    N = (len(trees[0][0]) + 1) // 2
    S = [[0 if metric == "size" else 0.0 for _ in range(N)] for _ in range(N)]
    W = 0
    for parent, bl, w in trees:
        mrca, value = tree_values(parent, bl, metric)
        W += int(w)
        for i in range(N):
            for j in range(N):
                if i != j:
                    if metric == "size":
                        S[i][j] += int(w) * value[mrca[i][j]]
                    else:
                        S[i][j] = S[i][j] + float(int(w)) * value[mrca[i][j]]  # product rounded, then the sum
    return S, W


def reference_sum(trees, metric, N):
    """the same sums in numpy, affordable at N = 10,240 (a few seconds per tree), and not by the library's algorithm
    (depth-first ranks and running maxima): the internal nodes in label order, children first; every live node keeps
    the indices of the leaves below it; node m with the children a < b (node order) is the MRCA of exactly the pairs
    A x B, so w * value(m) is added to S[A, B] and S[B, A] -- the product formed first, then one addition per element
    and tree, in tree order: the floats carry the bits of oracle_sum.
    trees: [(parent, branch_length or None, weight)] -> (S [N][N] uint64 (size) or float64 (time), W)"""
    assert metric in ("size", "time")
    S = np.zeros((N, N), np.uint64 if metric == "size" else np.float64)
    W = 0
    for parent, bl, w in trees:
        parent = np.asarray(parent, np.int64)
        assert parent.shape == (2 * N - 1,) and parent[-1] == -1 and (parent[:-1] > np.arange(2 * N - 2)).all()
        # sorted by parent, ties in node order: behind the root, the two children of N, of N + 1, ...
        kids = np.argsort(parent, kind="stable")[1:].reshape(N - 1, 2)
        assert np.array_equal(parent[kids], np.repeat(np.arange(N, 2 * N - 1), 2).reshape(N - 1, 2))
        W += int(w)
        below = {}  # live node -> the leaves below it
        h = [0.0] * (2 * N - 1)
        for m in range(N, 2 * N - 1):
            a, b = int(kids[m - N, 0]), int(kids[m - N, 1])
            A = below.pop(a) if a >= N else np.array([a])
            B = below.pop(b) if b >= N else np.array([b])
            if metric == "size":
                add = np.uint64(int(w) * (len(A) + len(B)))
            else:
                h[m] = h[a] + float(bl[a])  # the first child in node order
                add = np.float64(float(int(w))) * np.float64(h[m])
            S[np.ix_(A, B)] += add
            S[np.ix_(B, A)] += add
            below[m] = np.concatenate((A, B))
        assert list(below) == [2 * N - 2] and len(below[2 * N - 2]) == N
    return S, W


LARGE_WEIGHTS = [3, 2 ** 32 + 7, 0, 11]  # of large_case: one above 2^32, a zero


def large_case(N, balanced_too=True):
    """the input of the tests at the sizes only reference_sum affords: a caterpillar, its reverse, a balanced tree
    (weight 0) and one random tree -> (parents [T][2N-1], weights [T], branch lengths [T][2N-1]); without the
    balanced tree the zero weight goes with it"""
    rng = np.random.default_rng(N)
    keep = [0, 1, 2, 3] if balanced_too else [0, 1, 3]
    parents = np.stack(shapes(N, rng, randoms=1))[keep]
    bl = np.stack([branch_lengths(N, rng) for _ in range(4)])[keep]
    return parents, [LARGE_WEIGHTS[k] for k in keep], bl


def oracle_summary(S, W, metric, files, trees):
    """the stdout of `Relate --mode PairwiseCoalescence`: the off-diagonal mean of S / W summed in row order, the
    extreme pairs i < j (the first in row order)"""
    N = len(S)
    total, lo, hi = 0.0, None, None
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            v = float(S[i][j]) / float(W)
            total += v
            if j > i:
                if lo is None or v < lo[2]:
                    lo = (i, j, v)
                if hi is None or v > hi[2]:
                    hi = (i, j, v)
    return ["haplotypes %d" % N, "files %d" % files, "trees %d" % trees, "snps %d" % W, "metric %s" % metric,
            "mean %.17g" % (total / (float(N) * float(N - 1))), "min_pair %d %d %.17g" % lo, "max_pair %d %d %.17g" % hi]


def pwc_bytes(S, W, metric):
    """out.pwc: int32 N, int32 metric, int64 W, N x N sums row-major, little-endian"""
    a = np.array(S, dtype="<u8" if metric == "size" else "<f8")
    return (np.array([len(S), 0 if metric == "size" else 1], "<i4").tobytes() + np.array([W], "<i8").tobytes() +
            a.tobytes())


def branch_lengths(N, rng):
    """positive, not dyadic: a fused multiply-add in the sum would show"""
    return rng.random(2 * N - 1) * 1000.0 + 0.1


def file_weights(trees, end):
    """SNPs each tree of a file covers: to the next tree's position, the last one up to and including `end`"""
    pos = [t[0] for t in trees]
    return [(pos[t + 1] if t + 1 < len(pos) else end + 1) - pos[t] for t in range(len(pos))]
