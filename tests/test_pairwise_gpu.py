"""PairwiseCoalescence on the device (relate_amd/csrc/pairwise_kernels.hip) against the host implementation, bit for
bit, for both metrics, and end to end on the trees of a PaintBuildTopology run against the oracle of
pairwise_cases.py.  Every step that uses the GPU is a child process under a time limit of its own; after one that
was killed, aborted or timed out no further step is started."""
import os
import sys

import numpy as np
import pytest

import bigtile
import pairwise_cases as pc
from golden_util import Fixture
from relate_amd import api
from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
SMALL_N = 1024  # kPairwiseSmallN: above it the kernels run with larger workgroups (256 / 1024 threads, not 64 / 256)

CHILD = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
out = {}
for key, metric in (("size", "size"), ("time", "time"), ("time_again", "time")):
    t0 = time.perf_counter()
    out[key], out["W_" + key] = api.pairwise_trees(z["parents"], z["weights"], z["bl"], metric, device=0)
    out["seconds_" + key] = time.perf_counter() - t0
np.savez(sys.argv[3], **out)
"""

CHILD_BAD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
for metric in ("size", "time"):
    try:
        api.pairwise_trees(z["parents"], z["weights"], z["bl"], metric, device=0)
        print("accepted")
    except api.RelateError as e:
        print(metric, e)
good = np.delete(z["parents"], int(z["bad"]), 0)
S, W = api.pairwise_trees(good, np.delete(z["weights"], int(z["bad"])), None, "size", device=0)  # the process is healthy
np.savez(sys.argv[3], S=S, W=W)
"""


CHILD_ONE = """
import sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
t0 = time.perf_counter()
S, W = api.pairwise_trees(z["parents"], z["weights"], z["bl"], sys.argv[4], device=0)
seconds = time.perf_counter() - t0
np.save(sys.argv[3], S)
print(W, seconds)
"""

CHILD_TOO_LARGE = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from relate_amd import api
z = np.load(sys.argv[2])
for metric in ("size", "time"):
    try:
        api.pairwise_trees(z["parents"], z["weights"], z["bl"], metric, device=0)
        print("accepted")
    except api.RelateError as e:
        print(metric, e)
S, W = api.pairwise_trees(z["small"], z["weights"], z["small_bl"], "time", device=0)  # the process is healthy
np.savez(sys.argv[3], S=S, W=W)
"""


def on_device(tmp_path, parents, weights, bl, seconds=120):
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, parents=parents, weights=np.asarray(weights, np.int64), bl=bl)
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, src, dst], seconds)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    z = np.load(dst)
    return {k: z[k] for k in z.files}  # (read once: a matrix is 300 MB at N = 6146)


def check_against_host(tmp_path, N, parents, weights, bl, key):
    host_size, W = api.pairwise_trees(parents, weights, None, "size")
    host_time, _ = api.pairwise_trees(parents, weights, bl, "time")
    z = on_device(tmp_path, parents, weights, bl)
    assert z["size"].dtype == np.uint64 and z["time"].dtype == np.float64
    assert int(z["W_size"]) == int(z["W_time"]) == W
    assert np.array_equal(z["size"], host_size)
    assert np.array_equal(z["time"].view(np.uint64), host_time.view(np.uint64))  # equal bits
    assert np.array_equal(z["time_again"].view(np.uint64), z["time"].view(np.uint64))
    assert host_time[np.triu_indices(N, 1)].min() > 0
    bigtile.record("pairwise_coalescence/" + key,
                   dict(N=N, trees=len(parents), device_call_seconds_size=float(z["seconds_size"]),
                        device_call_seconds_time=float(z["seconds_time_again"])))
    return z


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 257, SMALL_N, SMALL_N + 1])
def test_device_equals_host(tmp_path, N):
    """wave-width and workgroup-width edges of the scans, both sides of the switch of workgroup sizes; a caterpillar,
    its reverse, a balanced tree and random ones, unequal weights with a zero among them"""
    rng = np.random.default_rng(N)
    parents = np.stack(pc.shapes(N, rng))
    bl = np.stack([pc.branch_lengths(N, rng) for _ in parents])
    check_against_host(tmp_path, N, parents, [7, 1, 0, 1000003, 12, 5], bl, "N%d" % N)


def cherry_comb(N):
    """(((l0, l1), (l2, l3)), (l4, l5)), ...: cherries joined in a chain, each label given as it is needed.  The first
    child (smaller label) of a chain node is the chain node two labels below it: the deepest chain of FIRST children a
    tree with rising labels has (a caterpillar's first child is always the leaf).  An odd N ends with (last leaf, chain)"""
    parent = np.full(2 * N - 1, -1, np.int32)
    parent[0] = parent[1] = chain = N
    label = N + 1
    for leaf in range(2, N - 1, 2):
        parent[leaf] = parent[leaf + 1] = label
        parent[chain] = parent[label] = chain = label + 1
        label += 2
    if N % 2:
        parent[N - 1] = parent[chain] = label
    return parent


def test_two_full_blocks_of_64(tmp_path):
    """N = 129: the 128 internal nodes are exactly two full blocks of 64 of the wave passes, no partial block, every
    lane of both blocks at work.  A caterpillar and its reverse: in the sizes and the left ends every lane waits for
    its neighbour, the first lane of a block for what the block before left in LDS.  Their heights do not chain (the
    first child of every node is a leaf), so a comb of cherries goes with them: there the heights pass, the pull scan
    on a double, has lane k wait for lane k - 2 through both blocks.  Both metrics against the host's bits.  (N = 65
    and 257 of test_device_equals_host end in a partial block.)"""
    N = 129
    rng = np.random.default_rng(N)
    parents = np.stack(pc.shapes(N, rng, randoms=0)[:2] + [cherry_comb(N)])
    assert (parents[:2, N:-1] == np.arange(N + 1, 2 * N - 1)).all()  # caterpillars: a chain of all internal nodes
    first = np.array([np.flatnonzero(parents[2] == m)[0] for m in range(N, 2 * N - 1)])
    assert (first[2:-1:2] == np.arange(N, 2 * N - 4, 2)).all()  # comb: the first child of N + 2k is N + 2k - 2
    bl = np.stack([pc.branch_lengths(N, rng) for _ in parents])
    check_against_host(tmp_path, N, parents, [3, 5, 7], bl, "N129_two_full_blocks")


def test_many_row_blocks_and_batches_and_the_same_bits_twice(tmp_path):
    """N = 1500, 40 trees: 500 workgroups of three rows; for `time` a tree takes 54 KB of the 2 MB a batch may, so the
    trees go up in two batches (38 + 2) and S waits on the device between them; `time` run twice gives the same bits
    (asserted in check_against_host for every shape, here for the one with the most workgroups)"""
    N = 1500
    rng = np.random.default_rng(N)
    parents = np.stack(pc.shapes(N, rng, randoms=37))
    assert len(parents) == 40
    bl = np.stack([pc.branch_lengths(N, rng) for _ in parents])
    z = check_against_host(tmp_path, N, parents, rng.integers(0, 5000, 40), bl, "N1500_40_trees")
    assert np.array_equal(z["time_again"].view(np.uint64), z["time"].view(np.uint64))


@pytest.mark.parametrize("N", [1537, 3510, 3511, 4098, 6146])
def test_device_equals_the_reference_across_the_lds_switches(tmp_path, N):
    """The sizes at which the launchers change route, against pairwise_cases.reference_sum (numpy, no ranks and no
    running maxima) over the whole matrix, bit for bit, and against the host implementation.  Dynamic LDS above 48 KB
    is asked for with hipFuncSetAttribute: `time` accumulate (14 N bytes) from N = 3511, `time` prepare (12 (N-1))
    from 4098, `size` accumulate (8 N) from 6145 and `size` prepare (8 (N-1)) from 6146.  1537: the smallest N with
    four rows per workgroup, the last workgroup a partial one (1 row); 3510 / 3511: either side of the first switch;
    6146: all four kernels above it, 13 rows per workgroup.  Below: test_device_equals_host.  A caterpillar, its
    reverse, a balanced tree with weight 0 and a random tree; one weight above 2^32."""
    parents, weights, bl = pc.large_case(N)
    rows = (N + 511) // 512
    assert (N + rows - 1) // rows * rows != N  # a partial last workgroup
    z = check_against_host(tmp_path, N, parents, weights, bl, "N%d" % N)
    trees = list(zip(parents, bl, weights))
    for metric in ("size", "time"):
        want, W = pc.reference_sum(trees, metric, N)
        assert int(z["W_" + metric]) == W == sum(weights)
        assert z[metric].dtype == want.dtype and np.array_equal(z[metric].view(np.uint64), want.view(np.uint64))
        del want


def test_device_equals_the_reference_at_the_documented_maximum(tmp_path):
    """N = 10,240, the largest the device takes: 20 rows per workgroup, 140 KB of LDS in a workgroup of 1024 threads
    (`time`), the root's size N = 10,240 and internal labels up to 10,238 in 16 bits.  Both caterpillars (the deepest
    trees: every boundary of the rank scans has another owner) and a random tree, one weight above 2^32, against
    reference_sum over the whole matrix, bit for bit.  A matrix is 839 MB: one metric at a time, each in a device
    process of its own, freed before the next; no host-twin comparison and no second `time` run here (the sizes
    below have them, and the zero weight).  The test is dominated by the reference on the CPU, about 3 s per tree
    and metric, 15 to 20 s in all; the device calls are recorded, not asserted on."""
    N = 10240
    parents, weights, bl = pc.large_case(N, balanced_too=False)
    assert len(parents) == 3 and max(weights) > 2 ** 32
    trees = list(zip(parents, bl, weights))
    src = str(tmp_path / "in.npz")
    np.savez(src, parents=parents, weights=np.asarray(weights, np.int64), bl=bl)
    seconds = {}
    for metric in ("size", "time"):
        dst = str(tmp_path / (metric + ".npy"))
        p = gpu_step([sys.executable, "-c", CHILD_ONE, ROOT, src, dst, metric], 180)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        gotW, seconds[metric] = p.stdout.decode().split()
        got = np.load(dst)
        os.remove(dst)
        want, W = pc.reference_sum(trees, metric, N)
        assert int(gotW) == W == sum(weights)
        assert got.dtype == want.dtype and got.shape == (N, N)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        if metric == "size":
            # leaves 0 and N-1 meet at the root of both caterpillars: the size 10,240 is among the values added
            assert N * (weights[0] + weights[1]) + 2 * weights[2] <= int(got[0, N - 1]) <= int(got.max()) <= N * W
        del got, want
    bigtile.record("pairwise_coalescence/N10240", dict(N=N, trees=len(parents), device_call_seconds_size=float(seconds["size"]),
                                                       device_call_seconds_time=float(seconds["time"])))


def test_one_leaf_too_many_is_refused(tmp_path):
    """N = 10,241: the device route returns RL_EINVAL (labels, ranks and sizes are 16-bit and the LDS is full) and
    says what it takes; the process computes a small case correctly afterwards"""
    N, n = 10241, 65
    rng = np.random.default_rng(N)
    small, small_bl = pc.random_tree(n, rng), pc.branch_lengths(n, rng)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, parents=pc.caterpillar(N)[None], weights=np.array([5], np.int64), bl=pc.branch_lengths(N, rng)[None],
             small=small[None], small_bl=small_bl[None])
    p = gpu_step([sys.executable, "-c", CHILD_TOO_LARGE, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 2
    for metric, line in zip(("size", "time"), lines):
        assert line.startswith(metric) and "error -1" in line and "2 <= N <= 10240" in line and "N=10241" in line, line
    z = np.load(dst)
    want, W = pc.reference_sum([(small, small_bl, 5)], "time", n)
    assert int(z["W"]) == W == 5 and np.array_equal(z["S"].view(np.uint64), want.view(np.uint64))


def test_weights_beyond_32_bits(tmp_path):
    rng = np.random.default_rng(31)
    parents = np.stack([pc.random_tree(8, rng) for _ in range(3)])
    bl = np.stack([pc.branch_lengths(8, rng) for _ in range(3)])
    weights = [2 ** 31, 2 ** 31, 5]
    want, W = pc.oracle_sum([(p, None, w) for p, w in zip(parents, weights)], "size")
    assert sum(v > 2 ** 32 for row in want for v in row) > 8
    z = check_against_host(tmp_path, 8, parents, weights, bl, "weights_64_bit")
    assert int(z["W_size"]) == W == 2 ** 32 + 5 and [[int(v) for v in row] for row in z["size"]] == want


def test_one_bad_tree_among_good_ones(tmp_path):
    N = 65
    rng = np.random.default_rng(9)
    parents = np.stack([pc.random_tree(N, rng) for _ in range(12)])
    parents[7] = pc.caterpillar(N)
    bad = parents[7]  # (a view: the batch's tree 7)
    a, b = 2 * N - 4, 2 * N - 3  # the two internal nodes below the root, a the child of b, trade labels
    bad[[a, b]] = bad[[b, a]]
    bad[bad == a], bad[bad == b] = -9, a
    bad[bad == -9] = b
    assert bad[b] == a  # parent a of node b: not above its child
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, parents=parents, weights=np.arange(1, 13), bl=np.stack([pc.branch_lengths(N, rng) for _ in parents]), bad=7)
    p = gpu_step([sys.executable, "-c", CHILD_BAD, ROOT, src, dst], 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 2
    for metric, line in zip(("size", "time"), lines):
        assert line.startswith(metric) and "error -1" in line and "tree 7" in line and "node %d" % b in line and "label above" in line
    z = np.load(dst)
    host, W = api.pairwise_trees(np.delete(parents, 7, 0), np.delete(np.arange(1, 13), 7))
    assert int(z["W"]) == W and np.array_equal(z["S"], host)


def test_end_to_end_on_built_trees(tmp_path):
    """PaintBuildTopology of synth24, then PairwiseCoalescence over all its section files on the device and on the
    host: the same bytes, for `size` the oracle's on the files read back in Python"""
    work = tmp_path / "run"
    (work / "out").mkdir(parents=True)
    fx = Fixture("synth24", work / "out")
    p = gpu_step([CLI, "--mode", "PaintBuildTopology", "--chunk_index", "0", "-o", "out", "--sum_mode", "exact"], 600,
                 cwd=str(work))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    files = [str(work / "out" / "chunk_0" / ("out_%d.anc" % w)) for w in range(fx.W)]
    seq = []
    for f in files:
        N, trees = pc.read_anc(open(f, "rb").read())
        assert N == fx.N
        seq += [(t[1], t[2], w) for t, w in zip(trees, pc.file_weights(trees, trees[-1][3]))]
    for metric in ("size", "time"):
        said = {}
        for tag, device in (("dev", "0"), ("host", "-1")):
            p = gpu_step([CLI, "--mode", "PairwiseCoalescence", "-i", ",".join(files), "-o", "%s_%s" % (metric, tag),
                          "--metric", metric, "--device", device], 120, cwd=str(tmp_path))
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            said[tag] = p.stdout.decode()
        dev = open(str(tmp_path / ("%s_dev.pwc" % metric)), "rb").read()
        assert dev == open(str(tmp_path / ("%s_host.pwc" % metric)), "rb").read()
        assert said["dev"] == said["host"]
        if metric == "size":
            want, W = pc.oracle_sum(seq, "size")
            assert dev == pc.pwc_bytes(want, W, "size")
            assert said["dev"].splitlines() == pc.oracle_summary(want, W, "size", len(files), len(seq))
            bigtile.record("pairwise_coalescence/synth24_size", dict(N=fx.N, files=len(files), trees=len(seq), snps=W,
                                                                     mean=said["dev"].splitlines()[5].split()[1]))
