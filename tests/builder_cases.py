"""Adversarial tree-builder sequences with the reference's answers on file (tests/golden/builder_adversarial.npz,
made by `python tools/make_golden.py builder` from the unmodified reference's MinMatch through oracle/ref_harness):
exact ties decided by the random draws, priors whose minima rise from tree to tree, the symmetric fallback from the
first merge on, a flat matrix (every pair a candidate; at N = 300 its merges still fit the device kernel's pair list
-- at N = 1300, family P below, the first one does not and that tree is the host's), coalescent-shaped matrices.
A case is a sequence of (distance matrix, prior or None) built by ONE builder, theta = 0.001.

Below them the families that take the device builder to the edges of its kernels and lists (FAMILIES; the golden
ones among them in tests/golden/builder_lists.npz), and the prediction of where a tree is built from the host
builder's census (stays_on_device): tests/test_builder_cases_cpu.py holds the host builder to the figures, tests/
test_builder_lists_gpu.py the device builder to the host's trees and to the prediction (check_family there)."""
import numpy as np


# ---- the matrix generators of the builder tests (test_builder_gpu.py and test_builder_ages_gpu.py use them too)
def tied_matrix(rng, N, ties=0.3):
    d = (rng.rand(N, N) * 4 + rng.rand(N)[:, None]).astype(np.float32)
    d[rng.rand(N, N) < ties] = 1.5  # plenty of exact ties: the random draws decide
    np.fill_diagonal(d, 0)
    return d


def coalescent_matrix(rng, N):
    """distances shaped like the path's: near-ultrametric from a random binary tree plus asymmetric noise"""
    order = rng.permutation(N)
    h = np.zeros((N, N), np.float32)
    groups = [[int(x)] for x in order]
    t = 0.0
    while len(groups) > 1:
        t += rng.exponential(1.0 / (len(groups) * (len(groups) - 1) / 2))
        a, b = sorted(rng.choice(len(groups), 2, replace=False))
        for x in groups[a]:
            for y in groups[b]:
                h[x, y] = h[y, x] = t
        groups[a] = groups[a] + groups[b]
        del groups[b]
    d = (h * 20 + rng.rand(N, N) * 0.05).astype(np.float32)
    d -= d.min(axis=1, keepdims=True)
    np.fill_diagonal(d, 0)
    return d


def split_tree_matrix(rng, N):
    """near-ultrametric distances from random recursive splits of a random leaf order (cheap at N = 5000),
    plus asymmetric noise -- the shape of the path's matrices"""
    order = rng.permutation(N)
    h = np.zeros((N, N), np.float32)
    stack = [(0, N, 1.0)]
    while stack:
        lo, hi, t = stack.pop()
        if hi - lo < 2:
            continue
        mid = lo + 1 + rng.randint(0, hi - lo - 1)
        a, b = order[lo:mid], order[mid:hi]
        h[np.ix_(a, b)] = t
        h[np.ix_(b, a)] = t
        stack.append((lo, mid, t * (0.55 + 0.4 * rng.rand())))
        stack.append((mid, hi, t * (0.55 + 0.4 * rng.rand())))
    d = (h * 20 + rng.rand(N, N) * 0.05).astype(np.float32)
    d -= d.min(axis=1, keepdims=True)
    np.fill_diagonal(d, 0)
    return d


def case_tied(N=64, seed=2):
    rng = np.random.RandomState(seed)
    mats = [(tied_matrix(rng, N), None)]
    for t in range(3):
        mats.append((tied_matrix(rng, N), ((np.floor(rng.rand(N, N) * 4) + t) * 6.9).astype(np.float32)))
    mats.append((tied_matrix(rng, N, 0.0), None))
    return N, mats


def case_symmetric(N=100, seed=2):
    rng = np.random.RandomState(seed)
    idx = np.arange(N)
    circ = (((idx[None, :] - idx[:, None]) % N) * 10.0).astype(np.float32)
    return N, [(circ, None), (circ + rng.rand(N, N).astype(np.float32), None),
               (circ + np.floor(rng.rand(N, N) * 3).astype(np.float32), (np.floor(rng.rand(N, N) * 3) * 6.9).astype(np.float32)),
               (tied_matrix(rng, N), None)]


def case_flat(N=300, seed=3):
    rng = np.random.RandomState(seed)
    flat = np.full((N, N), 2.5, np.float32)
    np.fill_diagonal(flat, 0)
    return N, [(coalescent_matrix(rng, N), None), (flat, None), (coalescent_matrix(rng, N), flat * 2),
               (coalescent_matrix(rng, N), None)]


def case_coalescent(N=400, seed=8):
    rng = np.random.RandomState(seed)
    mats = [(coalescent_matrix(rng, N), None)]
    for _ in range(2):
        mats.append((coalescent_matrix(rng, N), (np.floor(rng.rand(N, N) * 3) * 6.9).astype(np.float32)))
    return N, mats


CASES = {"tied": case_tied, "symmetric": case_symmetric, "flat": case_flat, "coalescent": case_coalescent}

# ---- where the device builder builds a tree, from the host builder's census of it
# (relate_amd/csrc/minmatch_params.h; the pair list of a merge in global memory: BuilderLayout::pair_cap.  Restated
#  by hand.  The census counts its tails in C++ from the header, so a changed MM_UPD_LDS, MM_PAIRS_LDS or MM_BUCKET_MIN
#  shows as a census mismatch on any machine; a changed MM_UPD_MAX or pair cap shows only on the GPU, where the families
#  at 512 / 513 rebuilt clusters and at 737 / 736 leaves are then built on the other side of the prediction.)
MM_BLOCK, MM_HITS, MM_UPD_LDS, MM_UPD_MAX, MM_PAIRS_LDS, MM_BUCKET_MIN = 512, 64, 256, 512, 320, 2048
L_LDS, L_GLOBAL, L_HOT, L_WARM = 0, 1, 2, 3


def pair_cap(N, ages):
    return (32 if ages else 8) * N


def stays_on_device(census, N, ages=False, sym_slots=1):
    """The device builder is the host builder's algorithm with the host builder's draws, so the host's counts are the
    lengths of the device's lists: the tree is the device's when the rebuilt clusters of every merge fit the list (the
    plain build hands over at nupd > MM_UPD_MAX, minmatch_build.h `if (!AGES && nupd > MM_UPD_MAX)`; the AGES list
    holds every cluster), the feasible pairs of every merge fit LDS plus the global pair list (`if (m - MM_PAIRS_LDS >
    p.pair_cap)`), and the tree needs no symmetric matrix or the device's pool has one (`if (slot < 0)`)."""
    if not ages and census["max_rebuilt"] > MM_UPD_MAX:
        return False
    if census["max_draws"] - MM_PAIRS_LDS > pair_cap(N, ages):
        return False
    return census["first_sym_merge"] < 0 or sym_slots > 0


# ---- the families
def rising_prior(rng, N, t=0, levels=3):
    return ((np.floor(rng.rand(N, N) * levels) + t) * 6.9).astype(np.float32)


def star_matrix(rng, N, G, interior, partners=False):
    """A group of G leaves, one of them the hub: hub to member and back 1, member to member `interior`, group to the
    rest 2000, the rest a coalescent matrix.  The group's leaves lie anywhere among the N (every thread and register
    slot of the kernel holds some).  Every merge of the hub's cluster moves the row minimum of every member left: all
    of them rebuild -- G - 2 at the first one.  interior = 1000: the members are candidates of the hub's cluster alone,
    one draw each; interior = 3.0: after the first merge of the hub (its distances become 2) the members are within the
    threshold (1.38 at theta = 0.001) of each other too, C(G - 1, 2) draws in one merge.
    partners: every member has a leaf of its own outside the group, c away and back, c between 2 and 8 and another for
    every member.  The first merge of the hub moves every member's row minimum to its c: a member is a candidate with its
    partner by ITS OWN new minimum, and the minima of two members are further apart than the threshold more often than
    not -- the rebuilt list has to hand every member its own."""
    group = np.sort(rng.choice(N, G, replace=False))
    hub = int(group[rng.randint(G)])
    rest = np.setdiff1d(np.arange(N), group)
    d = np.full((N, N), 2000.0, np.float32)
    if partners:
        own = rng.choice(rest, G, replace=False)
        rest = np.setdiff1d(rest, own)
        c = (2.0 + 6.0 * rng.rand(G)).astype(np.float32)
        d[group, own] = c
        d[own, group] = c
    d[np.ix_(rest, rest)] = coalescent_matrix(rng, len(rest))
    d[np.ix_(group, group)] = interior
    d[hub, group] = 1.0
    d[group, hub] = 1.0
    np.fill_diagonal(d, 0)
    return d


def late_symmetric_matrix(rng, N, H):
    """5000 everywhere; the first H leaves a coalescent matrix, the others a circulant block in which no two clusters
    are each other's closest: the tree's first H - 1 merges erase clusters from the kernel's live list -- it lives in
    registers for L_HOT / L_WARM -- before the symmetric fallback starts and mirrors that list to memory."""
    m = N - H
    d = np.full((N, N), 5000.0, np.float32)
    d[:H, :H] = coalescent_matrix(rng, H)
    idx = np.arange(m)
    d[H:, H:] = ((idx[None, :] - idx[:, None]) % m) * 10.0 + 100.0
    np.fill_diagonal(d, 0)
    return d


def flat_matrix(N):
    flat = np.full((N, N), 2.5, np.float32)
    np.fill_diagonal(flat, 0)
    return flat


def ancient_ages(rng, N, levels=4):
    ages = np.zeros(N)
    for lv in range(1, levels):
        ages[rng.rand(N) < 0.15] = lv * 400.0 * (1 + rng.randint(0, 3))
    return ages


class Family:
    """One sequence of trees of ONE builder.  make() -> [(d, prior or None), ...]; want: per tree the census figures
    the case is there for (None: the tree is there for its size or for the state it leaves) -- the host builder is held
    to them on any machine; ages: seed of the sample ages or None; kind: (layout, register slots, workgroups per CU)
    of the worker kernel the size gets, env: the switches of the process it is built in; golden: the reference's parent
    arrays are on file."""

    def __init__(self, name, N, make, want, kind, ages=None, env=None, golden=False, sym_slots=1):
        self.name, self.N, self.make, self.want, self.kind = name, N, make, want, kind
        self.ages, self.env, self.golden, self.sym_slots = ages, dict(env or {}), golden, sym_slots

    def sample_ages(self):
        return None if self.ages is None else ancient_ages(np.random.RandomState(self.ages), self.N)


def _star(N, G, interior, seed, partners=False):
    def make():
        rng = np.random.RandomState(seed)
        return [(star_matrix(rng, N, G, interior, partners), None),
                (star_matrix(rng, N, G, interior, partners), rising_prior(rng, N)), (coalescent_matrix(rng, N), None)]
    return make


def _late(N, H, seed):
    def make():
        rng = np.random.RandomState(seed)
        after = coalescent_matrix(rng, N) if N <= 1000 else split_tree_matrix(rng, N)
        return [(late_symmetric_matrix(rng, N, H), None), (after, None)]
    return make


def _tiles(N, seed, tied=False):
    def make():
        rng = np.random.RandomState(seed)
        gen = (lambda: tied_matrix(rng, N)) if tied else (lambda: split_tree_matrix(rng, N))
        mats = [(gen(), None), (gen(), rising_prior(rng, N))]
        # (a quarter of all pairs of a tied matrix are candidates: at this N more than the pair list holds, and the
        #  device builder takes the state back from the host for the tree behind them)
        return mats + [(split_tree_matrix(rng, N), None)] if tied else mats
    return make


def _small(N, seed):
    def make():
        rng = np.random.RandomState(seed)
        return [(tied_matrix(rng, N, 0.05), None), (tied_matrix(rng, N, 0.05), rising_prior(rng, N))]
    return make


def _flat(N, seed):
    def make():
        rng = np.random.RandomState(seed)
        return [(coalescent_matrix(rng, N), None), (flat_matrix(N), None), (coalescent_matrix(rng, N), None)]
    return make


def _ages_tiles(N, seed):
    def make():
        rng = np.random.RandomState(seed)
        return [(split_tree_matrix(rng, N), None), (split_tree_matrix(rng, N), rising_prior(rng, N))]
    return make


def _ages_star(N, G, interior, seed):
    def make():
        rng = np.random.RandomState(seed)
        return [(star_matrix(rng, N, G, interior), None), (coalescent_matrix(rng, N), None)]
    return make


HOT4, HOT10_2, WARM10, HOT20 = (L_HOT, 4, 2), (L_HOT, 10, 2), (L_WARM, 10, 1), (L_HOT, 20, 1)
AGES_LDS10, AGES_GLOBAL10, AGES_GLOBAL20 = (L_LDS, 10, 1), (L_GLOBAL, 10, 1), (L_GLOBAL, 20, 1)
OCC1, OCC2 = {"RELATE_AMD_BUILD_OCC": "1"}, {"RELATE_AMD_BUILD_OCC": "2"}
# The last N at which the AGES build keeps its state in LDS (worker_kind, minmatch_worker.hip): 33 bytes per cluster
# rounded up to 256 next to the kernel's 15,040 bytes of static LDS in the 160 KB of a CU -- 33 N <= 148,736.  The GPU
# test asks rl_debug_builder_kind for both sides of it: it fails if the kernel's static LDS moves the edge.
AGES_LDS_LAST_N = 4507


def check_census(census, want):
    """the figures of `want` that `census` misses: exact, or at least the value for a key ending in __min"""
    bad = {}
    for key, v in (want or {}).items():
        name = key[:-5] if key.endswith("__min") else key
        if (census[name] < v) if key.endswith("__min") else (census[name] != v):
            bad[key] = (census[name], v)
    return bad


def _families():
    F = []
    # S: the rebuilt list.  G - 2 rebuilt clusters in the first merge of the hub, one fewer in each one after it: G - 2 -
    # MM_UPD_LDS merges with a tail in global memory.  (The hub's row, or the first member's, has more mutually close
    # partners than the pair scan keeps: the kernel scans such rows itself.)
    for G, seed in ((258, 21), (259, 22), (514, 23), (515, 24)):
        want = dict(max_rebuilt=G - 2, merges_rebuilt_tail=max(0, G - 2 - MM_UPD_LDS), max_partners__min=MM_HITS + 1)
        F.append(Family("S_G%d_N700" % G, 700, _star(700, G, 1000.0, seed), [want, want, None], HOT4, golden=True))
    # (members with a partner each: the members in the tail of the list differ in their row minima)
    want = dict(max_rebuilt=300, merges_rebuilt_tail=44)
    F.append(Family("S_G300_N900_partners", 900, _star(900, 300, 1000.0, 26, partners=True), [want, want, None], HOT4,
                    golden=True))
    want = dict(max_rebuilt=512, merges_rebuilt_tail=256, max_partners__min=MM_HITS + 1)
    F.append(Family("S_G514_N2049", 2049, _star(2049, 514, 1000.0, 25), [want, want, None], WARM10))
    # P: the pair list.  C(G - 1, 2) draws in the first merge of the hub: 325 = MM_PAIRS_LDS + 5, the first pairs in
    # global memory; 6216 - MM_PAIRS_LDS = 8 x 737, the last tree the global pair list holds, and one leaf fewer.
    F.append(Family("P_G27_N600", 600, _star(600, 27, 3.0, 31), [dict(max_draws=325, merges_draws_global=1), None, None],
                    HOT4, golden=True))
    F.append(Family("P_G113_N737", 737, _star(737, 113, 3.0, 32), [dict(max_draws=6216)] * 2 + [None], HOT4, golden=True))
    F.append(Family("P_G113_N736", 736, _star(736, 113, 3.0, 33), [dict(max_draws=6216)] * 2 + [None], HOT4, golden=True))
    F.append(Family("P_flat_N1300", 1300, _flat(1300, 3),
                    [None, dict(max_rebuilt=8, max_draws=11412, max_partners=1299), None], HOT4))
    # L: the symmetric fallback after H - 1 merges
    late700, late2049 = dict(first_sym_merge=349, sym_merges=348), dict(first_sym_merge=1499, sym_merges=547)
    F.append(Family("L_N700_H350", 700, _late(700, 350, 41), [late700, None], HOT4, golden=True))
    F.append(Family("L_N2049_H1500", 2049, _late(2049, 1500, 42), [late2049, None], WARM10))
    F.append(Family("L_N2049_H1500_occ2", 2049, _late(2049, 1500, 42), [late2049, None], HOT10_2, env=OCC2))
    F.append(Family("L_N700_H350_no_pool", 700, _late(700, 350, 41), [late700, None], HOT4,
                    env={"RELATE_AMD_TEST_SYM_SLOTS": "0"}, sym_slots=0))
    # T: every register slot of every thread taken (N = MM_BLOCK x 4 / 10 / 20), and one past it
    for N, kind in ((2048, HOT4), (2049, WARM10), (5120, WARM10)):
        F.append(Family("T_split_N%d" % N, N, _tiles(N, N), [None, None], kind))
    F.append(Family("T_split_N10240", 10240, _tiles(10240, 10240), [None, None], HOT20))
    F.append(Family("T_tied_N2048", 2048, _tiles(2048, 7, tied=True), [None, None, None], HOT4))
    F.append(Family("T_split_N3000_occ2", 3000, _tiles(3000, 3000), [None, None], HOT10_2, env=OCC2))
    F.append(Family("T_split_N5120_occ2", 5120, _tiles(5120, 5120), [None, None], HOT10_2, env=OCC2))
    F.append(Family("T_split_N2048_occ1", 2048, _tiles(2048, 2048), [None, None], WARM10, env=OCC1))
    for N in (2, 3, 63, 64, 65, 511, 512, 513):
        F.append(Family("T_tied_N%d" % N, N, _small(N, 100 + N), [None, None], HOT4))
    # A: the AGES build -- both sides of the edge between its two layouts; a rebuilt list beyond the plain build's 512
    # (its tail is a list of its own, AI_UPD_G, that holds every cluster); merges with more than MM_BUCKET_MIN feasible
    # pairs, put in order bucket by bucket
    E = AGES_LDS_LAST_N
    F.append(Family("A_split_N%d" % E, E, _ages_tiles(E, 56), [dict(merges_draws_bucketed__min=1), None], AGES_LDS10,
                    ages=66))
    F.append(Family("A_split_N%d" % (E + 1), E + 1, _ages_tiles(E + 1, 53), [dict(merges_rebuilt_tail__min=1), None],
                    AGES_GLOBAL10, ages=63))
    F.append(Family("A_split_N5120", 5120, _ages_tiles(5120, 57), [None, None], AGES_GLOBAL10, ages=67))
    F.append(Family("A_S_G600_N1100", 1100, _ages_star(1100, 600, 1000.0, 53),
                    [dict(max_rebuilt=598, merges_rebuilt_tail=342), None], AGES_LDS10, ages=63))
    F.append(Family("A_P_G66_N1100", 1100, _ages_star(1100, 66, 3.0, 54),
                    [dict(max_draws=4335, merges_draws_bucketed=7), None], AGES_LDS10, ages=64))
    return F


FAMILIES = _families()
# (the same matrices as another family, built under another switch: the host builder's figures are that family's)
TWINS = {"L_N2049_H1500_occ2": "L_N2049_H1500", "T_split_N5120_occ2": "T_split_N5120",
         "T_split_N2048_occ1": "T_split_N2048", "L_N700_H350_no_pool": "L_N700_H350"}


def family(name):
    return next(f for f in FAMILIES if f.name == name)
