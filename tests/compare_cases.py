"""Trees, a brute-force clade distance and a per-SNP comparison of two tree sequences for the CompareTopology tests
(test_compare_cpu.py, test_compare_gpu.py).  Nothing here calls the library: the oracle is the definition in
include/relate_amd.h restated with Python sets."""
from tree_cases import balanced, caterpillar, nni, random_tree, read_anc, relabel, write_anc  # noqa: F401  (the tests' trees and files)


# ---------------------------------------------------------------- the oracle
def clades(parent):
    """the leaf sets (frozensets) of the internal nodes other than the root"""
    parent = [int(p) for p in parent]
    nodes = len(parent)
    N = (nodes + 1) // 2
    below = [frozenset([v]) if v < N else frozenset() for v in range(nodes)]
    kids = [[] for _ in range(nodes)]
    for v, p in enumerate(parent):
        if p >= 0:
            kids[p].append(v)
    order, todo = [], [parent.index(-1)]
    while todo:
        v = todo.pop()
        order.append(v)
        todo += kids[v]
    for v in reversed(order):  # children before parents, whatever the labels
        for c in kids[v]:
            below[v] = below[v] | below[c]
    return set(below[v] for v in range(N, nodes) if parent[v] != -1)


def oracle_distance(pa, pb):
    a, b = clades(pa), clades(pb)
    return len(a - b) + len(b - a)


# ------------------------------------------------------- two tree sequences
def oracle_compare(N, trees_a, end_a, trees_b, end_b):
    """SNP by SNP: which tree of each sequence covers it, runs of the same pair of trees are the intervals.
    -> (rows [(snp_begin, snp_end, tree of A, tree of B, d)], summary dict)"""
    begin, end = max(trees_a[0][0], trees_b[0][0]), min(end_a, end_b) + 1
    assert begin < end

    def covering(trees, s):
        return max(t for t in range(len(trees)) if trees[t][0] <= s)

    rows, memo = [], {}
    for s in range(begin, end):
        ta, tb = covering(trees_a, s), covering(trees_b, s)
        if rows and rows[-1][2:4] == [ta, tb]:
            rows[-1][1] = s + 1
            continue
        if (ta, tb) not in memo:
            memo[(ta, tb)] = oracle_distance(trees_a[ta][1], trees_b[tb][1])
        rows.append([s, s + 1, ta, tb, memo[(ta, tb)]])
    full, snps, weighted, same = 2.0 * (N - 2), float(end - begin), 0.0, 0
    for b, e, _, _, d in rows:  # in interval order, in double, as the header says the host does
        if N > 2:
            weighted += float(e - b) * (float(d) / full)
        same += (e - b) if d == 0 else 0
    return rows, dict(N=N, trees_a=len(trees_a), trees_b=len(trees_b), intervals=len(rows), snp_begin=begin,
                      snp_end=end, max_distance=max(r[4] for r in rows), snps_identical=same,
                      mean_normalised=weighted / snps, share_identical=float(same) / snps)


def check_summary(got, rows, want):
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)  # doubles included: equal, not close
    assert got["per_interval"].tolist() == rows
