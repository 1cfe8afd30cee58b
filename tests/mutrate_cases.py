"""The oracle of the AvgMutationRate tests (test_mutrate_cpu.py, test_mutrate_gpu.py).  Nothing here calls the
library: the definition of include/relate_amd.h (rl_mutrate_trees) is restated over the sorted times of the INTERNAL
nodes alone -- no sort of all 2N-1 nodes, no per-node lineage table --, the .mut and --dist files are written in
Python, and tests/golden/mutrate_ref.npz (tools/make_golden_mutrate.py) holds what the reference's RelateMutationRate
wrote and what its two per-tree functions and its two sums hold, to the bit."""
import os

import numpy as np

import coalrate_cases as cc
import frequency_cases as fc
from coalrate_cases import balanced, caterpillar, dated_lengths, random_tree, shapes  # noqa: F401  (the tests' trees)
from frequency_cases import MUT_HEAD, clock_lengths, max_times, tie_trees  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mutrate_ref.npz")
BINS = cc.BINS
# the fixture's cases -> (--bins, --years_per_gen, with a --dist file)
CASES = {"a": (None, None, False), "b": (None, None, False), "b_bins": (BINS, None, False), "s": (None, None, False),
         "s_dist": (None, None, True), "tie": (None, None, False), "young": ("6.5,7.5,0.5", "1e6", False)}


def fixture():
    return np.load(FIXTURE)


def default_epochs(years_per_gen=28.0, E=31):
    """the reference's default boundaries restated in doubles: log(10) and years_per_gen pass through a float"""
    ypg, log10 = np.float64(np.float32(years_per_gen)), np.float64(np.float32(np.log(10.0)))
    ep = np.zeros(E, np.float64)
    ep[1] = 1e3 / ypg
    for e in range(2, E - 1):
        ep[e] = np.exp(log10 * (3.0 + 4.0 * (e - 1.0) / (E - 3.0))) / ypg
    ep[E - 1] = 1e8 / ypg
    return ep


def lengths_in_epochs(parent, bl, epochs):
    """the branch length of one tree in every epoch, by the closed form: with t_1 <= ... <= t_{N-1} the sorted float
    times of the internal nodes and t_0 = 0, the interval (t_{k-1}, t_k] carries N - (k-1) lineages; a cursor walks
    the epochs.  An interval that ends below the cursor's upper boundary adds a float32 product of a float32
    difference; one that reaches it adds a double product up to the boundary, ASSIGNS every whole epoch it crosses
    and the part inside the epoch it ends in; the walk ends for good at the last epoch.  -> [E] float64, [E-1] = 0"""
    N = (len(parent) + 1) // 2
    ep = np.asarray(epochs, np.float64)
    E = len(ep)
    t = np.sort(max_times(parent, bl)[N:])
    out = np.zeros(E, np.float64)
    c, a = 0, np.float32(0.0)
    for k, b in enumerate(t):  # interval k: (a, b], N - k lineages
        if not b > a:
            continue
        n = N - k
        if np.float64(b) < ep[c + 1]:
            out[c] += np.float64(np.float32(n) * np.float32(b - a))
        else:
            out[c] += np.float64(n) * (ep[c + 1] - np.float64(a))
            c += 1
            if c == E - 1:
                break
            while c < E - 1 and ep[c + 1] < np.float64(b):
                out[c] = np.float64(n) * (ep[c + 1] - ep[c])
                c += 1
            if c == E - 1:
                break
            out[c] = np.float64(n) * (np.float64(b) - ep[c])
        a = b
    return out


def mut_text(rows):
    """the .mut: rows = [(pos, dist, tree, branches, flipped, age_begin, age_end)], branches a list of node labels"""
    return (MUT_HEAD + "".join("%d;%d;%d;rs%d;%d;%s;%d;%d;%s;%s;A/C;\n" % (
        k, pos, dist, k, tree, " ".join(str(int(b)) for b in br), len(br) != 1, flipped, repr(float(a0)), repr(float(a1)))
        for k, (pos, dist, tree, br, flipped, a0, a1) in enumerate(rows))).encode()


def dist_text(rows, rng):
    """a --dist file for the rows of a .mut: one header line, `pos dist` per line, with positions the .mut does not
    hold before, between and after its own (each splits the dist of the position before it)"""
    lines = ["#pos dist", "%d %d" % (rows[0][0] - 40, 40)]
    for k, r in enumerate(rows):
        pos, dist = r[0], r[1]
        if dist >= 2 and rng.integers(0, 3) == 0:
            cut = int(rng.integers(1, dist))
            lines += ["%d %d" % (pos, cut), "%d %d" % (pos + cut, dist - cut)]
        else:
            lines.append("%d %d" % (pos, dist))
    lines.append("%d %d" % (rows[-1][0] + rows[-1][1], 1))
    return ("\n".join(lines) + "\n").encode()


def branch_rows(N, trees, rng, per_tree=3, skip=(), big_dist_at=5):
    """SNPs on random branches below the root with the branch's real ages [t(b), t(parent(b))], tree indices rising,
    none on the trees of `skip`; every fourth tree also a flipped row (counted) and a row with two branches (not);
    one dist is large"""
    rows, pos = [], 100
    for t, (_, parent, bl) in enumerate(trees):
        if t in skip:
            continue
        times = max_times(parent, bl)
        extra = [("flipped",), ("two",)] if t % 4 == 0 else []
        for k in range(per_tree + len(extra)):
            dist = 40000000 if len(rows) == big_dist_at else int(rng.integers(1, 5000))
            b = int(rng.integers(0, 2 * N - 2))
            kind = extra[k - per_tree][0] if k >= per_tree else ""
            br = [b, (b + 1) % (2 * N - 2)] if kind == "two" else [b]
            rows.append((pos, dist, t, br, int(kind == "flipped"), float(times[b]), float(times[parent[b]])))
            pos += dist
    return rows


def rows_as_arrays(rows):
    a = np.array([(p, d, t, br[0], br[1] if len(br) > 1 else -2, f) for p, d, t, br, f, _, _ in rows], np.int32)
    return a, np.array([(a0, a1) for *_, a0, a1 in rows], np.float64)


def rows_from_arrays(ints, ages):
    return [(int(p), int(d), int(t), [int(b)] + ([int(b2)] if b2 != -2 else []), int(f), float(a0), float(a1))
            for (p, d, t, b, b2, f), (a0, a1) in zip(ints.tolist(), ages.tolist())]


def young_trees():
    """N = 16 for --years_per_gen 1e6 --bins 6.5,7.5,0.5 (boundaries 0, 3.16, 10, 31.6, 100 generations): a tree whose
    root lies inside epoch 0, one whose root is far above the last boundary, one that spans the epochs, and one whose
    first coalescence is already above the last boundary"""
    N = 16
    rng = np.random.default_rng(16)
    trees = []
    for k, (scale, floor) in enumerate(((0.1, 0.0), (300.0, 0.0), (8.0, 0.0), (1.0, 150.0))):
        parent = random_tree(N, rng)
        bl = rng.uniform(0.1, 1.0, 2 * N - 1) * scale
        bl[:N] += floor
        bl[2 * N - 2] = 0.0
        bl = bl.astype(np.float32).astype(np.float64)
        trees.append((20 * k, parent, bl))
    return N, trees


def case_inputs(fx, key):
    """-> (N, trees [(pos, parent, bl)], .anc bytes, .mut bytes, --dist bytes or None) of a fixture case"""
    co = cc.fixture()
    if key in ("a", "b", "b_bins"):
        tag = key[0]
        anc = co[tag + "/anc"].tobytes()
        N, parents, bl = cc.parse_anc_text(anc)
        mut = co["a/mut"].tobytes() if tag == "a" else mut_text(rows_from_arrays(fx["b/rows"], fx["b/ages"]))
        return N, [(0, p, b) for p, b in zip(parents, bl)], anc, mut, None
    src = "s" if key == "s_dist" else key
    if src == "s":
        N, trees = fc.case_s_rows(co)
    else:
        N = 16
        trees = list(zip(fx[src + "/pos"].tolist(), fx[src + "/parents"].astype(np.int32), fx[src + "/bl"].astype(np.float64)))
    rows = rows_from_arrays(fx[src + "/rows"], fx[src + "/ages"])
    dist = fx["s_dist/dist"].tobytes() if key == "s_dist" else None
    return N, trees, cc.anc_text(N, trees), mut_text(rows), dist
