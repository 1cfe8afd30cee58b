"""The oracle of the CoalescentRateForSection tests (test_coalrate_cpu.py, test_coalrate_gpu.py).  Nothing here calls
the library: the definition of include/relate_amd.h is restated in numpy float32 without ranks or running maxima, the
text .anc / .mut files are written in Python, and tests/golden/coalrate_ref.npz (tools/make_golden_coalrate.py) holds
what the reference's RelateCoalescentRate wrote for three cases."""
import hashlib
import os

import numpy as np

from pairwise_cases import balanced, caterpillar, random_tree, shapes  # noqa: F401  (the tests' trees)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "coalrate_ref.npz")
BINS = "2,6,0.5"  # the --bins of fixture case (b)'s second run


def fixture():
    return np.load(FIXTURE)


def reference_bins(parents, bl, factors, epochs):
    """D [E][N][N] float32 by the definition: the internal nodes in label order, children first; every live node keeps
    the indices of the leaves below it; node m with the children a < b (node order) is the MRCA of exactly the pairs
    A x B.  Its time is t(m) = float32(float64(t(a)) + bl[a]); with e the first epoch whose upper boundary is above
    t(m) (E-1: none), the element of the pair's smaller row and larger column gets the factor at plane e, the element
    of its larger row and smaller column factor * width at the planes before e and factor * (t - ep[e]) at e: one
    float32 addition per element and tree, the product formed first, trees in order."""
    parents = np.atleast_2d(np.asarray(parents, np.int64))
    bl = np.atleast_2d(np.asarray(bl, np.float64))
    ep = np.asarray(epochs, np.float32)
    E, N = len(ep), (parents.shape[1] + 1) // 2
    D = np.zeros((E, N, N), np.float32)
    for parent, b, factor in zip(parents, bl, factors):
        assert parent.shape == (2 * N - 1,) and parent[-1] == -1 and (parent[:-1] > np.arange(2 * N - 2)).all()
        kids = np.argsort(parent, kind="stable")[1:].reshape(N - 1, 2)
        assert np.array_equal(parent[kids], np.repeat(np.arange(N, 2 * N - 1), 2).reshape(N - 1, 2))
        f = np.float32(factor)
        fw = [f * (ep[e + 1] - ep[e]) for e in range(E - 1)]  # float32 throughout
        t = np.zeros(2 * N - 1, np.float32)
        below = {}
        for m in range(N, 2 * N - 1):
            a, c = int(kids[m - N, 0]), int(kids[m - N, 1])
            A = below.pop(a) if a >= N else np.array([a])
            B = below.pop(c) if c >= N else np.array([c])
            t[m] = np.float32(np.float64(t[a]) + b[a])
            e = int(np.searchsorted(ep[1:], t[m], side="right"))  # boundaries at or below t
            own = f * (t[m] - ep[e]) if e < E - 1 else None
            for q in range(min(e, E - 2) + 1):
                for rows, cols in ((A, B), (B, A)):
                    ix = np.ix_(rows, cols)
                    block = D[q][ix]
                    low = rows[:, None] > cols[None, :]  # the larger row, the smaller column: the opportunity
                    block[low] += own if q == e else fw[q]
                    if q == e:
                        block[~low] += f
                    D[q][ix] = block
            below[m] = np.concatenate((A, B))
        assert list(below) == [2 * N - 2] and len(below[2 * N - 2]) == N
    return D


def default_epochs(years_per_gen=28.0, E=31):
    """the reference's default boundaries restated: doubles rounded to float32 (libm's exp through numpy)"""
    ypg, log10 = np.float64(np.float32(years_per_gen)), np.float64(np.float32(np.log(10.0)))
    ep = np.zeros(E, np.float32)
    ep[1] = np.float32(1e3 / ypg)
    for e in range(2, E - 1):
        ep[e] = np.float32(np.exp(log10 * (3.0 + 4.0 * (e - 1.0) / (E - 3.0))) / ypg)
    ep[E - 1] = np.float32(1e8 / ypg)
    return ep


def dated_lengths(N, rng, top=14.0):
    """branch lengths (float32-exact doubles) whose node times spread over the default epochs: exp of a uniform"""
    return np.exp(rng.uniform(0.0, top, 2 * N - 1)).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------- files
def anc_text(N, trees):
    """the text .anc: trees = [(pos, parent, branch_length)]; lengths by repr (they read back exactly)"""
    lines = ["NUM_HAPLOTYPES %d" % N, "NUM_TREES %d" % len(trees)]
    for pos, parent, bl in trees:
        lines.append("%d: " % pos + " ".join("%d:(%s 0.000 %d %d)" % (int(p), repr(float(x)), pos, pos)
                                              for p, x in zip(parent, bl)) + " ")
    return ("\n".join(lines) + "\n").encode()


def mut_text(rows):
    """the .mut: rows = [(pos, dist, tree)]"""
    head = "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n"
    return (head + "".join("%d;%d;%d;rs%d;%d;0;0;0;0.000000;10.000000;A/C;\n" % (k, pos, dist, k, tree)
                           for k, (pos, dist, tree) in enumerate(rows))).encode()


def mut_factors(rows, ntrees):
    """AncMutIterators::NextTree restated: the bases every tree persists for -- half the dist before its first SNP,
    its SNPs' dists, minus half the last; 0 without SNPs -- as float32"""
    out = []
    k, L = 0, len(rows)
    for t in range(ntrees):
        if k == L or rows[k][2] != t:
            out.append(np.float32(0.0))
            continue
        bases = rows[k - 1][1] / 2.0 if k else 0.0
        while k < L and rows[k][2] == t:
            bases += rows[k][1]
            k += 1
        if k < L:
            bases -= rows[k - 1][1] / 2.0
        out.append(np.float32(bases))
    return out


def with_trailing_pass(parents, bl, factors):
    """the reference's loop runs once more after its last tree: that tree again with the factor -1"""
    return (np.concatenate((parents, parents[-1:])), np.concatenate((bl, bl[-1:])),
            list(factors) + [np.float32(-1.0)])


def parse_anc_text(buf):
    """-> (N, parents [T][2N-1] int32, branch lengths [T][2N-1] float64)"""
    lines = buf.decode().split("\n")
    N, T = int(lines[0].split()[1]), int(lines[1].split()[1])
    parents, bl = np.zeros((T, 2 * N - 1), np.int32), np.zeros((T, 2 * N - 1), np.float64)
    for t in range(T):
        body = lines[2 + t].split(": ", 1)[1]
        for v, rec in enumerate(body.strip().split(") ")):
            p, rest = rec.split(":(")
            parents[t, v], bl[t, v] = int(p), float(rest.split(" ")[0])
    return N, parents, bl


def parse_mut_text(buf):
    return [(int(c[1]), int(c[2]), int(c[4])) for c in (ln.split(";") for ln in buf.decode().split("\n")[1:] if ln)]


def bin_bytes(epochs, D):
    """out.bin: int32 E, E floats, then per plane two 64-bit words N, N and N x N floats"""
    ep, D = np.asarray(epochs, "<f4"), np.asarray(D, "<f4")
    N = D.shape[1]
    return np.int32(len(ep)).tobytes() + ep.tobytes() + b"".join(np.array([N, N], "<u8").tobytes() + d.tobytes() for d in D)


def parse_bin(buf):
    E = int(np.frombuffer(buf, "<i4", 1)[0])
    ep = np.frombuffer(buf, "<f4", E, 4)
    N = int(np.frombuffer(buf, "<u8", 1, 4 + 4 * E)[0])
    at, D = 4 + 4 * E, np.zeros((E, N, N), np.float32)
    for e in range(E):
        assert [int(x) for x in np.frombuffer(buf, "<u8", 2, at)] == [N, N]
        D[e] = np.frombuffer(buf, "<f4", N * N, at + 16).reshape(N, N)
        at += 16 + 4 * N * N
    assert at == len(buf)
    return ep.copy(), D


def plane_md5(D):
    return np.stack([np.frombuffer(hashlib.md5(np.ascontiguousarray(d, "<f4").tobytes()).digest(), np.uint8) for d in D])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# -------------------------------------------------------- the fixture's inputs
def case_b():
    """fixture case (b), N = 24: a caterpillar, its reverse, a balanced tree and three random trees with lengths exact
    in float32 -- a zero-length branch, a node time exactly on the default epochs' first boundary, one past the last
    boundary -- and a .mut that leaves tree 4 without SNPs -> (N, trees [(pos, parent, bl)], mut rows)"""
    N = 24
    rng = np.random.default_rng(24)
    ep = default_epochs()
    trees = []
    for k, parent in enumerate(shapes(N, rng, randoms=3)):
        bl = dated_lengths(N, rng, top=12.0)
        kids = np.argsort(parent, kind="stable")[1:].reshape(N - 1, 2)
        if k == 0:
            bl[int(kids[0, 0])] = float(ep[1])   # node N: its time is exactly the boundary ep[1]
            bl[int(kids[1, 0])] = 0.0            # node N + 1 is dated by its first child, leaf 2: a zero-length branch, time 0
        if k == 2:
            bl[int(kids[N - 2, 0])] = 4.0e6      # the root: past the last boundary, 1e8 / 28
        if k == 3:
            bl[int(kids[N - 2, 0])] = float(ep[30])  # the root exactly on the last boundary
        bl[2 * N - 2] = 0.0
        trees.append((100 * k, parent, bl))
    rows, pos = [], 1000
    for t, nsnp in enumerate([3, 1, 4, 2, 0, 5]):
        for _ in range(nsnp):
            dist = int(rng.integers(1, 4000))
            rows.append((pos, dist, t))
            pos += dist
    return N, trees, rows


def case_c():
    """fixture case (c), N = 300: 40 random dated trees and a .mut with one to three SNPs per tree"""
    N, T = 300, 40
    rng = np.random.default_rng(300)
    trees = [(10 * k, random_tree(N, rng), dated_lengths(N, rng)) for k in range(T)]
    rows, pos = [], 500
    for t in range(T):
        for _ in range(int(rng.integers(1, 4))):
            dist = int(rng.integers(1, 9000))
            rows.append((pos, dist, t))
            pos += dist
    return N, trees, rows
