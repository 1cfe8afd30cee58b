"""The oracle of the Frequency / Selection tests (test_frequency_cpu.py, test_selection_cpu.py, test_frequency_gpu.py).
Nothing here calls the library: the closed form of include/relate_amd.h (rl_frequency_trees) is restated with numpy
masks -- no ranks, no sort, no depth-first intervals --, the .mut files are written in Python, and
tests/golden/selection_ref.npz (tools/make_golden_selection.py) holds what the reference's RelateSelection wrote."""
import os

import numpy as np

import coalrate_cases as cc
from coalrate_cases import balanced, caterpillar, dated_lengths, random_tree, shapes  # noqa: F401  (the tests' trees)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "selection_ref.npz")
BINS = cc.BINS
# the fixture's cases: key -> (where the inputs are, --bins)
CASES = ("a", "b", "b_bins", "s", "tie")

MUT_HEAD = "snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n"


def fixture():
    return np.load(FIXTURE)


def mut_text(rows):
    """the .mut: rows = [(pos, dist, tree, branches, flipped, age_begin)], branches a list of node labels"""
    return (MUT_HEAD + "".join("%d;%d;%d;rs%d;%d;%s;%d;%d;%s;%s;A/C;\n" % (
        k, pos, dist, k, tree, " ".join(str(int(b)) for b in br), len(br) != 1, flipped, repr(float(age)), repr(float(age) + 10.0))
        for k, (pos, dist, tree, br, flipped, age) in enumerate(rows))).encode()


def mut_rows_from_arrays(a):
    """[rows][6] ints (pos, dist, tree, branch, second branch or -2, flipped) + ages -> rows of mut_text"""
    return [(int(p), int(d), int(t), [int(b)] + ([int(b2)] if b2 != -2 else []), int(f), float(age))
            for (p, d, t, b, b2, f), age in zip(a["rows"].tolist(), a["ages"].tolist())]


def max_times(parent, bl):
    """Tree::GetCoordinates: t(leaf) = 0, t(m) = float32(max over the children c of float64(t(c)) + bl[c])"""
    parent = np.asarray(parent, np.int64)
    nodes = len(parent)
    t = np.zeros(nodes, np.float32)
    best = np.full(nodes, -1.0, np.float64)
    for v in range(nodes - 1):  # children have smaller labels: t[v] is final when v is met
        if best[v] >= 0.0:
            t[v] = np.float32(best[v])
        best[parent[v]] = max(best[parent[v]], np.float64(t[v]) + np.float64(bl[v]))
    t[nodes - 1] = np.float32(best[nodes - 1])
    return t


def tie_free(parent, bl):
    """no two internal nodes with equal float times, none at or below 0: the closed form is established"""
    N = (len(parent) + 1) // 2
    t = max_times(parent, bl)[N:]
    return len(np.unique(t)) == len(t) and (t > 0).all()


def below_mask(parent, b):
    """nodes in the subtree of b, b included"""
    parent = np.asarray(parent, np.int64)
    inside = np.zeros(len(parent), bool)
    inside[b] = True
    for v in range(b - 1, -1, -1):  # a node's parent has a larger label
        inside[v] = inside[parent[v]] if parent[v] <= b else False
    return inside


def closed_form(parent, bl, b, epochs):
    """one row by the definition -> (freq [E], lin [E] oldest boundary first, when_DAF_is_half,
    when_mutation_has_freq2); b is neither -1 nor the root"""
    parent = np.asarray(parent, np.int64)
    N = (len(parent) + 1) // 2
    ep = np.asarray(epochs, np.float32)
    t = max_times(parent, bl)
    internal = np.arange(len(parent)) >= N
    S = below_mask(parent, b) & internal
    root = t[-1]
    freq, lin = [], []
    for e in ep[::-1]:
        lin.append(0 if root < e else 1 + int((t[internal] > e).sum()))
        freq.append(0 if root < e or t[parent[b]] <= e else 1 + int((t[S] > e).sum()))
    daf = int((below_mask(parent, b) & ~internal).sum())
    h = (daf + 1) // 2
    half = -1
    if h > 1:
        x = np.sort(t[S])[::-1][h - 2]
        half = 1 + int((t[internal] >= x).sum())
    freq2 = -1 if b < N else 1 + int((t[internal] >= t[b]).sum())
    return freq, lin, half, freq2


def header(epochs, lin):
    """std::to_string of every float boundary, oldest first"""
    cols = "".join("%f " % float(e) for e in np.asarray(epochs, np.float32)[::-1])
    return "pos rs_id " + cols + ("when_DAF_is_half when_mutation_has_freq2\n" if lin else "TreeFreq DataFreq\n")


def files_by_closed_form(N, trees, rows, epochs):
    """(.freq, .lin) bytes of tie-free trees by the definition: the filter, the counts, the layout"""
    freq_out, lin_out = [header(epochs, False)], [header(epochs, True)]
    times = {}
    for k, (pos, dist, tree, br, flipped, age) in enumerate(rows):
        _, parent, bl = trees[tree]
        if tree not in times:
            times[tree] = max_times(parent, bl)
        if len(br) != 1 or flipped or not np.float32(age) <= times[tree][-1] or br[0] == -1 or br[0] == 2 * N - 2:
            continue
        f, l, half, freq2 = closed_form(parent, bl, br[0], epochs)
        freq_out.append("%d rs%d " % (pos, k) + "".join("%d " % x for x in f) + " 0 0\n")
        lin_out.append("%d rs%d " % (pos, k) + "".join("%d " % x for x in l) + "%d %d\n" % (half, freq2))
    return "".join(freq_out).encode(), "".join(lin_out).encode()


def random_rows(N, trees, rng, per_tree=3, skip=(), filtered=True):
    """SNPs on random branches (neither -1 nor the root), tree indices rising, none on the trees of `skip`; with
    `filtered`, rows the filter drops among them: two branches, flipped, the root, -1, an age above the root"""
    rows, pos = [], 100
    for t, (_, parent, bl) in enumerate(trees):
        if t in skip:
            continue
        root_time = float(max_times(parent, bl)[-1])
        for k in range(per_tree):
            dist = int(rng.integers(1, 5000))
            b = int(rng.integers(0, 2 * N - 2))
            rows.append((pos, dist, t, [b], 0, 0.0 if k % 2 else root_time * float(rng.uniform(0.0, 1.0))))
            pos += dist
        if filtered and t % 4 == 0:
            for br, flipped, age in (([0, 1], 0, 0.0), ([N - 1], 1, 0.0), ([2 * N - 2], 0, 0.0), ([-1], 0, 0.0),
                                     ([1], 0, root_time * 1.5 + 1.0)):
                rows.append((pos, 7, t, br, flipped, age))
                pos += 7
    return rows


def clock_lengths(parent, rng, first=10.0):
    """branch lengths that are tie-free by construction at any N: the internal nodes get float32 times that rise
    with the label by a random factor in [1 + 2^-12, 1 + 2^-9] (labels rise from child to parent, so this is a dated
    tree), and a branch is the exact difference of its ends -- dated_lengths' sums collide in float32 once a tree has
    thousands of nodes"""
    parent = np.asarray(parent, np.int64)
    nodes = len(parent)
    N = (nodes + 1) // 2
    t = np.zeros(nodes, np.float32)
    t[N:] = (first * np.cumprod(1.0 + rng.uniform(2.0 ** -12, 2.0 ** -9, N - 1))).astype(np.float32)
    assert (np.diff(t[N:]) > 0).all()
    bl = np.zeros(nodes, np.float64)
    bl[:-1] = t[parent[:-1]].astype(np.float64) - t[:-1].astype(np.float64)
    return bl


def tie_trees(N, T, seed):
    """trees whose branch lengths come from {0, 1, 2, 4} x 100 generations: clades coalesce at equal times, internal
    nodes at time 0 among them"""
    rng = np.random.default_rng(seed)
    trees = []
    for k in range(T):
        parent = random_tree(N, rng) if k % 3 else balanced(N)
        bl = rng.choice(np.array([0.0, 100.0, 100.0, 200.0, 400.0]), 2 * N - 1)
        if k % 2 == 0:  # (the first tree without: its lineages at the boundary 0 are the N of Selection's table)
            bl[bl == 0.0] = 100.0
        bl[2 * N - 2] = 0.0
        trees.append((50 * k, parent, bl))
    return trees


def case_s_rows(fx_coalrate):
    """the synthetic case: the 40 random dated trees of coalrate_ref.npz's case c (N = 300) -> (N, trees)"""
    z = fx_coalrate
    return 300, list(zip(z["c/pos"].tolist(), z["c/parents"].astype(np.int32), z["c/bl"].astype(np.float64)))


def rows_as_arrays(rows):
    a = np.array([(p, d, t, br[0], br[1] if len(br) > 1 else -2, f) for p, d, t, br, f, _ in rows], np.int32)
    return a, np.array([age for *_, age in rows], np.float64)
