"""The oracle of the SubTreesForSubpopulation tests (test_subtrees_cpu.py, test_subtrees_gpu.py).  Nothing here calls
the library: the per-tree definition of include/relate_amd.h (rl_subtrees_trees) is restated per CHAIN -- the counts
bottom-up, the new labels a cumulative sum of the keep flags, every subset leaf and kept node adding the branch lengths
of the ancestors it contracts, then the times on the subtree -- where the library's host twin restates the reference's
loop over the internal nodes; and tests/golden/subtrees_ref.npz (tools/make_golden_subtrees.py) holds the inputs of
the file cases, what the reference's RelateExtract wrote for them in --mode SubTreesForSubpopulation and what its
Tree::GetSubTree and Tree::GetCoordinates held for every tree, to the bit."""
import os

import numpy as np

import coalrate_cases as cc
from coalrate_cases import dated_lengths  # noqa: F401  (the tests' branch lengths)
from frequency_cases import max_times
from tree_cases import balanced, caterpillar, nni, random_tree, shapes  # noqa: F401  (the tests' trees)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "subtrees_ref.npz")
OUTPUTS = ("sub_parent", "sub_bl", "sub_time", "convert_index", "number_in_subpop")
MUT_HEADER = ("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
              "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;")


def fixture():
    return np.load(FIXTURE)


# ------------------------------------------------------------------ one tree
def subtree(parent, bl, subset):
    """one tree by its chains -> dict of OUTPUTS.  subset: leaf labels, rising.  Python floats: every addition is one
    IEEE double operation, in the order the chain meets its ancestors (bottom-up)"""
    parent = [int(p) for p in parent]
    nodes = len(parent)
    N, M = (nodes + 1) // 2, len(subset)
    length = [float(x) for x in bl]
    count = [0] * nodes
    for s in subset:
        count[int(s)] = 1
    kids = [[] for _ in range(nodes)]
    for v in range(nodes - 1):
        kids[parent[v]].append(v)
    for v in range(N, nodes):  # labels rise from child to parent
        count[v] = count[kids[v][0]] + count[kids[v][1]]
    kept = [v >= N and count[kids[v][0]] > 0 and count[kids[v][1]] > 0 for v in range(nodes)]
    new = [-1] * nodes
    for k, s in enumerate(subset):
        new[int(s)] = k
    rank = np.cumsum(kept) - np.array(kept)  # exclusive
    for v in range(N, nodes):
        if kept[v]:
            new[v] = M + int(rank[v])
    assert sum(kept) == M - 1
    sub = 2 * M - 1
    conv = [new[v] if (v < N or kept[v]) else -1 for v in range(nodes)]
    sub_parent, sub_bl = [-1] * sub, [0.0] * sub
    for v in range(nodes):
        if new[v] < 0:
            continue
        total, p = length[v], parent[v]
        while p != -1 and not kept[p]:
            total += length[p]
            conv[p] = new[v]
            p = parent[p]
        sub_parent[new[v]], sub_bl[new[v]] = (-1 if p == -1 else new[p]), total
    sub_parent, sub_bl = np.array(sub_parent, np.int32), np.array(sub_bl, np.float64)
    return {"sub_parent": sub_parent, "sub_bl": sub_bl, "sub_time": max_times(sub_parent, sub_bl),
            "convert_index": np.array(conv, np.int32), "number_in_subpop": np.array(count, np.int32)}


def subtrees(parents, bl, subset):
    """[trees] -> dict of OUTPUTS stacked"""
    one = [subtree(p, b, subset) for p, b in zip(parents, bl)]
    return {k: np.stack([o[k] for o in one]) for k in OUTPUTS}


def same(got, want):
    """every output equal to the bit -> the names of those that differ"""
    bad = []
    for k in OUTPUTS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


def mixed_lengths(parent, rng):
    """branch lengths whose double sum along a chain depends on the order: magnitudes from 1e-3 to 1e12 with full
    mantissas, mixed along every path"""
    nodes = len(parent)
    return (rng.uniform(1.0, 2.0, nodes) * 10.0 ** rng.integers(-3, 13, nodes)).astype(np.float64)


def reversed_chain_differs(parent, bl, subset):
    """does adding some chain of the case top-down give other bits than bottom-up"""
    want = subtree(parent, bl, subset)
    conv, N = want["convert_index"], (len(parent) + 1) // 2
    for s in range(2 * len(subset) - 1):
        members = [v for v in range(len(parent)) if conv[v] == s]  # rising labels: the head, then its contracted ancestors
        down = 0.0
        for v in reversed(members):
            down += float(bl[v])
        if np.float64(down).tobytes() != np.float64(want["sub_bl"][s]).tobytes():
            return True
    return False


# ------------------------------------------------------------------ the file cases
def poplabels_text(groups_of_lines, ploidy):
    """groups_of_lines: the group of every line; ploidy: the fourth column ("NA" or "1")"""
    return ("sample population group sex\n" + "".join("id%d %s G %s\n" % (k, g, ploidy) for k, g in enumerate(groups_of_lines))).encode()


def sequence(N, T, rng):
    """T dated trees: neighbours differ by a few nearest-neighbour interchanges or only in their lengths
    -> [(pos placeholder 0, parent, bl)]"""
    parent = random_tree(N, rng)
    out = []
    for t in range(T):
        if t and t % 3:
            for _ in range(int(rng.integers(1, 4))):
                parent = nni(parent, rng)
        out.append((0, parent.copy(), np.round(dated_lengths(N, rng, top=9.0), 5)))
    return out


def leaves_below(parent, N):
    below = [set([v]) if v < N else set() for v in range(len(parent))]
    for v in range(len(parent) - 1):
        below[int(parent[v])] |= below[v]
    return below


def mut_lines(trees, group_of_haplotype, G, rng, with_freq, skip=(), outside=(), subset=()):
    """the lines of a full .mut for the trees: one to four SNPs per tree on a random branch below the root, one in
    seven on two branches (not mapping); the trees of `skip` get none, the SNPs of the trees of `outside` lie on
    branches without a leaf of `subset` below them.  with_freq: the flanking bases and a column per group, the
    carriers of the SNP's first branch in that group"""
    lines, pos, k = [], 100, 0
    for t, (_, parent, bl) in enumerate(trees):
        if t in skip:
            continue
        nodes = len(parent)
        N = (nodes + 1) // 2
        below = leaves_below(parent, N)
        times = max_times(parent, bl)
        for _ in range(int(rng.integers(1, 5))):
            if t in outside:
                free = [v for v in range(nodes - 1) if not (below[v] & set(subset))]
                branches = [int(free[int(rng.integers(len(free)))])]
            elif rng.integers(7) == 0:
                branches = sorted(int(x) for x in rng.choice(nodes - 1, 2, replace=False))
            else:
                branches = [int(rng.integers(nodes - 1))]
            b = branches[0]
            dist = int(rng.integers(1, 9000))
            line = "%d;%d;%d;rs%d;%d;%s;%d;%d;%.6g;%.6g;%s;" % (
                k, pos, dist, k, t, " ".join(str(x) for x in branches), len(branches) > 1, int(rng.integers(2)),
                float(times[b]), float(times[int(parent[b])]), "ACGT"[int(rng.integers(4))] + "/" + "ACGT"[int(rng.integers(4))])
            if with_freq:
                freq = [sum(1 for v in below[b] if group_of_haplotype[v] == g) for g in range(G)]
                line += "%s;%s;" % ("ACGT"[int(rng.integers(4))], "ACGT"[int(rng.integers(4))]) + "".join("%d;" % f for f in freq)
            lines.append(line)
            pos += dist
            k += 1
    return lines


def mut_text(lines, groups=None):
    """the .mut of the lines; groups: the names behind the standard header when the lines carry frequency columns"""
    head = MUT_HEADER + ("".join(g + ";" for g in groups) if groups else "")
    return (head + "\n" + "".join(ln + "\n" for ln in lines)).encode()


def anc_text(N, trees, positions):
    return cc.anc_text(N, [(pos, p, b) for pos, (_, p, b) in zip(positions, trees)])


def tree_positions(lines, T):
    """the index of every tree's first SNP (a tree without SNPs: that of the next SNP)"""
    first, k = [], 0
    tree_of = [int(ln.split(";")[4]) for ln in lines]
    for t in range(T):
        while k < len(tree_of) and tree_of[k] < t:
            k += 1
        first.append(k)
    return first


def group_table(lines_groups, diploid):
    """-> (sorted names, group of every haplotype)"""
    names = sorted(set(lines_groups))
    goh = []
    for g in lines_groups:
        goh += [names.index(g)] * (2 if diploid else 1)
    return names, goh


def synthetic_cases():
    """the written cases of the fixture -> {key: dict(anc, mut, poplabels bytes, pops)}: see tools/make_golden_subtrees.py"""
    cases = {}
    N = 24
    three = ["ZED", "ALPHA", "MID"]
    dip = [three[k % 3] for k in range(N // 2)]
    names, goh = group_table(dip, True)
    rng = np.random.default_rng(24)
    trees = sequence(N, 14, rng)
    lines = mut_lines(trees, goh, 3, rng, False)
    anc = anc_text(N, trees, tree_positions(lines, len(trees)))
    labels = poplabels_text(dip, "NA")
    cases["one"] = dict(anc=anc, mut=mut_text(lines), poplabels=labels, pops="MID")
    cases["dup"] = dict(anc=anc, mut=mut_text(lines), poplabels=labels, pops="ZED,ALPHA,ZED")
    cases["all"] = dict(anc=anc, mut=mut_text(lines), poplabels=labels, pops="MID,ZED,ALPHA")
    cases["All"] = dict(anc=anc, mut=mut_text(lines), poplabels=labels, pops="All")
    flines = mut_lines(trees, goh, 3, np.random.default_rng(25), True)
    cases["freq"] = dict(anc=anc_text(N, trees, tree_positions(flines, len(trees))), mut=mut_text(flines, names), poplabels=labels,
                         pops="MID,ALPHA")
    hap = [three[k % 3] for k in range(N)]
    cases["hap"] = dict(anc=anc, mut=mut_text(lines), poplabels=poplabels_text(hap, "1"), pops="ALPHA")
    lone = ["SOLO" if k == 5 else three[k % 3] for k in range(N // 2)]
    cases["m2"] = dict(anc=anc, mut=mut_text(lines), poplabels=poplabels_text(lone, "NA"), pops="SOLO")
    # trees 2, 3 and 9 lose every SNP: theirs lie on branches without a leaf of the subset below them
    _, goh_d = group_table(dip, True)
    sub = [h for h in range(N) if goh_d[h] == names.index("ZED")]
    dlines = mut_lines(trees, goh, 3, np.random.default_rng(26), False, outside=(2, 3, 9), subset=sub)
    cases["drop"] = dict(anc=anc_text(N, trees, tree_positions(dlines, len(trees))), mut=mut_text(dlines), poplabels=labels, pops="ZED")
    # the last three trees have no SNP
    tlines = mut_lines(trees, goh, 3, np.random.default_rng(27), False, skip=(11, 12, 13))
    cases["tail"] = dict(anc=anc_text(N, trees, tree_positions(tlines, len(trees))), mut=mut_text(tlines), poplabels=labels, pops="ALPHA,MID")
    return cases


A_POPLABELS = poplabels_text(["P2", "P0", "P3", "P1"], "NA")
A_POPS = "P3,P0"
CASES = ("a", "one", "dup", "all", "All", "freq", "hap", "m2", "drop", "tail")


def case_inputs(fx, key):
    """-> dict(anc, mut, poplabels: bytes; pops: str) of a fixture case"""
    if key == "a":
        co = cc.fixture()
        return dict(anc=co["a/anc"].tobytes(), mut=co["a/mut"].tobytes(), poplabels=A_POPLABELS, pops=A_POPS)
    return dict(anc=fx[key + "/anc"].tobytes(), mut=fx[key + "/mut"].tobytes(), poplabels=fx[key + "/poplabels"].tobytes(),
                pops=str(fx[key + "/pops"]))


def subset_of(poplabels, pops):
    """Sample::Read and AssignPopOfInterest restated -> (sorted group names, indices of interest, subset labels)"""
    rows = [ln.split() for ln in poplabels.decode().split("\n")[1:] if ln]
    diploid = not any(len(r) > 3 and r[3] == "1" for r in rows)
    names, goh = group_table([r[1] for r in rows], diploid)
    of_interest = sorted(set(range(len(names)) if pops == "All" else (names.index(p) for p in pops.split(","))))
    return names, of_interest, [h for h, g in enumerate(goh) if g in of_interest]
