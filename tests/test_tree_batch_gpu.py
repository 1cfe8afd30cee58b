"""The staging of a batch of trees that the device sides of the tree-sequence modes share (relate_amd/csrc/tree_batch.h),
past the first batch: at N = 9 a call of batch + 2 trees whose tree batch + 1 has a parent below its child is refused
with that tree's number in the message (the index within the second batch, rebased), and the same process then runs
batch + 2 good trees -- the staging arrays reused after the refusal, the second batch clean -- and matches the host
twin bit for bit.  One child process per mode under a time limit of its own; after one that was killed, aborted or
timed out no further step is started."""
import os
import sys

import pytest

from rlutil import gpu_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
MODES = ("coalrate", "pairwise", "coaltree", "mutrate", "mutctx", "frequency", "subtrees")

CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from relate_amd import api
from tree_cases import balanced, caterpillar
mode = sys.argv[3]
N = 9
# pairwise has no entry point for it: kPairwiseBatchBytes over the bytes of a tree with metric size (parents 4 a node,
# weight 8, rank, g and size 2 a leaf each, flag 4)
batch = {"pairwise": (2 << 20) // ((2 * N - 1) * 4 + 8 + N * 6 + 4),
         "mutctx": api.mutrate_batch_trees(N)}.get(mode) or getattr(api, mode + "_batch_trees")(N)
T = batch + 2
shapes = np.array([caterpillar(N), balanced(N), caterpillar(N, range(N - 1, -1, -1))], np.int32)
lengths = np.random.default_rng(9).uniform(0.5, 2.0, shapes.shape)
pick = np.arange(T) % 3
P, BL = shapes[pick], lengths[pick]
low = P.copy()
low[batch + 1] = shapes[0]
low[batch + 1, N] = 3  # the parent of node 9 below it
ep64 = np.array([0.0, 1.0, 2.0, 4.0, 8.0, 1e6])
ep32 = ep64.astype(np.float32)
factors = (1.0 + np.arange(T) % 5).astype(np.float32)
snp_tree = np.arange(0, T, 7, dtype=np.int32)
counts = np.ones((len(snp_tree), api.MUTCTX_CATEGORIES), np.uint32)
snp_branch = (snp_tree % (2 * N - 2)).astype(np.int32)
run = {
    "coalrate": lambda p, d: [api.coalrate_trees(p, BL, factors, ep32, device=d)],
    "pairwise": lambda p, d: list(api.pairwise_trees(p, 1 + np.arange(T) % 3, device=d)),
    "coaltree": lambda p, d: list(api.coaltree_trees(p, BL, factors, ep64, device=d)),
    "mutrate": lambda p, d: [api.mutrate_trees(p, BL, ep64, device=d)],
    "mutctx": lambda p, d: [api.mutctx_trees(p, BL, snp_tree, counts, ep64, device=d)],
    "frequency": lambda p, d: list(api.frequency_trees(p, BL, snp_tree, snp_branch, ep32, device=d)[:4]),
    "subtrees": lambda p, d: [a for _, a in sorted(api.subtrees_trees(p, BL, [0, 2, 3, 7], device=d).items())],
}[mode]
print("batch", batch)
try:
    run(low, 0)
    print("accepted")
except api.RelateError as e:
    print("refused:", e)
got, want = run(P, 0), run(P, None)
assert len(got) == len(want)
for a, b in zip(got, want):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (mode, a.dtype, a.shape)
print("equal", len(got))
"""


@pytest.mark.parametrize("mode", MODES)
def test_refusal_in_the_second_batch_then_a_clean_run(mode):
    p = gpu_step([sys.executable, "-c", CHILD, ROOT, TESTS, mode], 120)
    out = p.stdout.decode().splitlines()
    assert p.returncode == 0, (out, p.stderr.decode()[-3000:])
    batch = int(out[0].split()[1])
    assert out[0].startswith("batch ") and 5000 <= batch <= 40000
    assert out[1] == ("refused: librelate_amd error -1: rl_%s_trees: tree %d: parent 3 of node 9 does not have a label "
                      "above its child's" % (mode, batch + 1))
    assert out[2].startswith("equal ")
