"""What the tests of the tree modes share (compare_cases.py: CompareTopology; pairwise_cases.py: PairwiseCoalescence):
the tree shapes and the .anc file in Python.  Nothing here calls the library."""
import numpy as np

ANC_NODE = np.dtype([("parent", "<i4"), ("branch_length", "<f8"), ("num_events", "<f4"), ("snp_begin", "<i4"),
                     ("snp_end", "<i4")])  # 24 bytes, no padding: AncesTree::DumpBin writes field by field
assert ANC_NODE.itemsize == 24


# ------------------------------------------------------------------- trees
def relabel(parent):
    """the same tree with its internal nodes numbered so that every parent's label is above its children's"""
    parent = [int(p) for p in parent]
    nodes = len(parent)
    N = (nodes + 1) // 2
    kids = [[] for _ in range(nodes)]
    for v, p in enumerate(parent):
        if p >= 0:
            kids[p].append(v)
    order, todo = [], [parent.index(-1)]
    while todo:
        v = todo.pop()
        order.append(v)
        todo += kids[v]
    new, nxt = {}, N
    for v in reversed(order):  # a reversed pre-order lists every node after its descendants
        if v < N:
            new[v] = v
        else:
            new[v] = nxt
            nxt += 1
    out = np.full(nodes, -1, np.int32)
    for v, p in enumerate(parent):
        if p >= 0:
            out[new[v]] = new[p]
    return out


def random_tree(N, rng):
    """random joins: the next label goes to the parent of two clusters drawn at random"""
    parent = np.full(2 * N - 1, -1, np.int32)
    live = list(range(N))
    for label in range(N, 2 * N - 1):
        i = int(rng.integers(len(live)))
        a = live.pop(i)
        j = int(rng.integers(len(live)))
        b = live.pop(j)
        parent[a] = parent[b] = label
        live.append(label)
    return parent


def caterpillar(N, order=None):
    """((((l0, l1), l2), l3), ...): every internal node is the parent of the one before it"""
    order = list(range(N)) if order is None else [int(x) for x in order]
    parent = np.full(2 * N - 1, -1, np.int32)
    if N == 1:
        return parent
    parent[order[0]] = parent[order[1]] = N
    for k in range(2, N):
        parent[N + k - 2] = parent[order[k]] = N + k - 1
    return parent


def balanced(N):
    """neighbours joined level by level"""
    parent = np.full(2 * N - 1, -1, np.int32)
    level, label = list(range(N)), N
    while len(level) > 1:
        nxt = []
        for k in range(0, len(level) - 1, 2):
            parent[level[k]] = parent[level[k + 1]] = label
            nxt.append(label)
            label += 1
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return parent


def nni(parent, rng):
    """one nearest-neighbour interchange: an internal node other than the root trades one child for its sibling"""
    parent = np.array(parent, dtype=np.int32)
    nodes = len(parent)
    N = (nodes + 1) // 2
    assert N >= 3
    inner = [v for v in range(N, nodes) if parent[v] != -1]
    v = inner[int(rng.integers(len(inner)))]
    p = int(parent[v])
    sib = [c for c in range(nodes) if parent[c] == p and c != v][0]
    child = [c for c in range(nodes) if parent[c] == v][int(rng.integers(2))]
    parent[sib], parent[child] = v, p
    return relabel(parent)


def shapes(N, rng, randoms=3):
    """a caterpillar, the caterpillar on the leaves in reverse order, a balanced tree, random trees"""
    return [caterpillar(N), caterpillar(N, range(N - 1, -1, -1)), balanced(N)] + [random_tree(N, rng) for _ in range(randoms)]


# ------------------------------------------------------------- .anc files
def write_anc(path, N, trees, end, ages=None):
    """trees: [(pos, parent)] or [(pos, parent, branch_length or None)]; SNP_begin / SNP_end of every branch as
    BuildTopology leaves them (the tree's position, the next tree's; the last tree's SNP_end = end, the sequence's
    last SNP); ages: sample ages, written if given"""
    with open(path, "wb") as f:
        f.write(np.uint8(ages is not None).tobytes() + np.uint32(N).tobytes())
        if ages is not None:
            f.write(np.asarray(ages, "<f8").tobytes())
        f.write(np.uint32(len(trees)).tobytes())
        for t, (pos, parent, *bl) in enumerate(trees):
            rec = np.zeros(2 * N - 1, ANC_NODE)
            rec["parent"] = parent
            if bl and bl[0] is not None:
                rec["branch_length"] = bl[0]
            rec["snp_begin"] = pos
            rec["snp_end"] = trees[t + 1][0] if t + 1 < len(trees) else end
            f.write(np.int32(pos).tobytes() + rec.tobytes())


def read_anc(buf):
    """bytes of a .anc file without sample ages -> (N, [(pos, parent, branch_length, largest SNP_end)])"""
    assert buf[0] == 0
    N, T = [int(x) for x in np.frombuffer(buf, "<u4", 2, 1)]
    at, out = 9, []
    for _ in range(T):
        pos = int(np.frombuffer(buf, "<i4", 1, at)[0])
        rec = np.frombuffer(buf, ANC_NODE, 2 * N - 1, at + 4)
        out.append((pos, rec["parent"].astype(np.int32), rec["branch_length"].astype(np.float64), int(rec["snp_end"].max())))
        at += 4 + 24 * (2 * N - 1)
    assert at == len(buf)
    return N, out
