"""What the tree-sequence modes say when they refuse an input, and what the epoch makers return, pinned whole: every
message below is the complete text behind a RelateError on the host path (device=None), every epoch array the exact
bits.  The checks, the epoch makers and the walks over an .anc are shared between the modes; a change to the shared
code that moves one byte of one mode's answer fails here."""

import numpy as np
import pytest

import coalrate_cases as cc
import frequency_cases as fc
import mutctx_cases as xc
import mutrate_cases as mc
from relate_amd import api
from tree_cases import balanced, caterpillar

N, T = 5, 3
PARENTS = np.array([caterpillar(N), balanced(N), caterpillar(N)], np.int32)
BL = np.tile(np.arange(1.0, 2 * N), (T, 1))  # node v: v + 1
EP32 = np.array([0.0, 2.0, 5.0, 1e6], np.float32)
FACTORS = np.ones(T, np.float32)
SNP_TREE = np.arange(T, dtype=np.int32)
COUNTS = np.ones((T, api.MUTCTX_CATEGORIES), np.uint32)

# mode -> (call(parents, bl, epochs), the epochs' type); compare, pairwise and subtrees take no epochs
TREES = {
    "compare": (lambda p, b, e: api.compare_trees(p, PARENTS), None),
    "pairwise": (lambda p, b, e: api.pairwise_trees(p, np.ones(T, np.int64)), None),
    "coalrate": (lambda p, b, e: api.coalrate_trees(p, b, FACTORS, e), np.float32),
    "frequency": (lambda p, b, e: api.frequency_trees(p, b, SNP_TREE, np.zeros(T, np.int32), e), np.float32),
    "mutrate": (lambda p, b, e: api.mutrate_trees(p, b, e), np.float64),
    "coaltree": (lambda p, b, e: api.coaltree_trees(p, b, FACTORS, e), np.float64),
    "subtrees": (lambda p, b, e: api.subtrees_trees(p, b, [0, 2, 3]), None),
    "mutctx": (lambda p, b, e: api.mutctx_trees(p, b, SNP_TREE, COUNTS, e), np.float64),
}
WITH_LENGTHS = ("coalrate", "frequency", "mutrate", "coaltree", "subtrees", "mutctx")
BAD_EPOCHS = {"E=1": [0.0], "E=65": np.arange(65.0), "first": [1.0, 2.0, 3.0], "equal": [0.0, 5.0, 5.0, 9.0],
              "inf": [0.0, 5.0, np.inf]}


PREFIX = "librelate_amd error -1: "  # (RL_EINVAL)


def message(call):
    """the text of rl_last_error behind a refusal, or None"""
    try:
        call()
    except api.RelateError as e:
        assert str(e).startswith(PREFIX)
        return str(e)[len(PREFIX):]
    return None


def tree_cases():
    """(name, call) of every refusal of a *_trees entry point"""
    low = PARENTS.copy()
    low[1, 5] = 3  # tree 1: the parent of node 5 below it
    out = []
    for mode, (call, ep_type) in TREES.items():
        ep = None if ep_type is None else EP32.astype(ep_type)
        out.append((mode + "/parent", lambda call=call, ep=ep: call(low, BL, ep)))
        if mode in WITH_LENGTHS:
            for kind, value in (("negative", -0.5), ("nan", np.nan)):
                bl = BL.copy()
                bl[1, 2] = value
                out.append((mode + "/" + kind, lambda call=call, ep=ep, bl=bl: call(PARENTS, bl, ep)))
        if mode == "subtrees":
            bl = BL.copy()
            bl[2, 2 * N - 2] = -1.0  # the root's: the length only this mode reads
            out.append((mode + "/root", lambda call=call, bl=bl: call(PARENTS, bl, None)))
        if ep_type is not None:
            for kind, bad in BAD_EPOCHS.items():
                bad = np.asarray(bad, ep_type)
                out.append((mode + "/" + kind, lambda call=call, bad=bad: call(PARENTS, BL, bad)))
    return out


TREE_CASES = dict(tree_cases())

TREE_MESSAGES = {
    "compare/parent": "rl_compare_trees: tree 1 of A: parent 3 of node 5 does not have a label above its child's",
    "pairwise/parent": "rl_pairwise_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "coalrate/parent": "rl_coalrate_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "coalrate/negative": "rl_coalrate_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "coalrate/nan": "rl_coalrate_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "coalrate/E=1": "rl_coalrate_trees: 2 <= epochs <= 64 (1 given)",
    "coalrate/E=65": "rl_coalrate_trees: 2 <= epochs <= 64 (65 given)",
    "coalrate/first": "rl_coalrate_trees: the first epoch boundary is 1, not 0",
    "coalrate/equal": "rl_coalrate_trees: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "coalrate/inf": "rl_coalrate_trees: epoch boundary 2 (inf) is not finite and above boundary 1 (5)",
    "frequency/parent": "rl_frequency_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "frequency/negative": "rl_frequency_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "frequency/nan": "rl_frequency_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "frequency/E=1": "rl_frequency_trees: 2 <= epochs <= 64 (1 given)",
    "frequency/E=65": "rl_frequency_trees: 2 <= epochs <= 64 (65 given)",
    "frequency/first": "rl_frequency_trees: the first epoch boundary is 1, not 0",
    "frequency/equal": "rl_frequency_trees: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "frequency/inf": "rl_frequency_trees: epoch boundary 2 (inf) is not finite and above boundary 1 (5)",
    "mutrate/parent": "rl_mutrate_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "mutrate/negative": "rl_mutrate_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "mutrate/nan": "rl_mutrate_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "mutrate/E=1": "rl_mutrate_trees: 2 <= epochs <= 64 (1 given)",
    "mutrate/E=65": "rl_mutrate_trees: 2 <= epochs <= 64 (65 given)",
    "mutrate/first": "rl_mutrate_trees: the first epoch boundary is 1, not 0",
    "mutrate/equal": "rl_mutrate_trees: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "mutrate/inf": "rl_mutrate_trees: epoch boundary 2 (inf) is not finite and above boundary 1 (5)",
    "coaltree/parent": "rl_coaltree_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "coaltree/negative": "rl_coaltree_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "coaltree/nan": "rl_coaltree_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "coaltree/E=1": "rl_coaltree_trees: 2 <= epochs <= 64 (1 given)",
    "coaltree/E=65": "rl_coaltree_trees: 2 <= epochs <= 64 (65 given)",
    "coaltree/first": "rl_coaltree_trees: the first epoch boundary is 1, not 0",
    "coaltree/equal": "rl_coaltree_trees: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "coaltree/inf": "rl_coaltree_trees: epoch boundary 2 (inf) is not finite and above boundary 1 (5)",
    "subtrees/parent": "rl_subtrees_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "subtrees/negative": "rl_subtrees_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "subtrees/nan": "rl_subtrees_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "subtrees/root": "rl_subtrees_trees: tree 2: branch length -1 of node 8 is negative or not finite",
    "mutctx/parent": "rl_mutctx_trees: tree 1: parent 3 of node 5 does not have a label above its child's",
    "mutctx/negative": "rl_mutctx_trees: tree 1: branch length -0.5 of node 2 is negative or not finite",
    "mutctx/nan": "rl_mutctx_trees: tree 1: branch length nan of node 2 is negative or not finite",
    "mutctx/E=1": "rl_mutctx_trees: 2 <= epochs <= 64 (1 given)",
    "mutctx/E=65": "rl_mutctx_trees: 2 <= epochs <= 64 (65 given)",
    "mutctx/first": "rl_mutctx_trees: the first epoch boundary is 1, not 0",
    "mutctx/equal": "rl_mutctx_trees: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "mutctx/inf": "rl_mutctx_trees: epoch boundary 2 (inf) is not finite and above boundary 1 (5)",
}


@pytest.mark.parametrize("name", sorted(TREE_CASES))
def test_trees_refusal(name):
    assert message(TREE_CASES[name]) == TREE_MESSAGES[name]


# ---------------------------------------------------------------------------------------------------- the epoch makers
EPOCHS = {  # float32 words | float.hex()
    "coalrate/default": ["00000000", "420edb6e", "42467fd7", "4289e831", "42bf9f04", "430520dc", "4338fb34", "438083ec",
                         "43b2924b", "43f81fcd", "442c623d", "446f86c5", "44a66914", "44e73a01", "4520a4e7", "455f36de",
                         "459b13e1", "45d77acd", "4615b43b", "46500359", "46908441", "46c8ce21", "470b824b", "4741d8d9",
                         "4786acc1", "47bb214b", "48020218", "4834a552", "487b01aa", "48ae62de", "4a59fb92"],
    "coalrate/bins": ["00000000", "4064924a", "4134b39c", "420edb6f", "42e1e083", "43b2924b", "448d2c52", "455f36de",
                      "46307767", "470b824b", "47dc9541", "4a59fb92"],
    "coalrate/2,6": "rl_coalrate_epochs: bins `2,6`: epochs format is wrong. Specify x,y,stepsize.",
    "mutrate/default": ["0x0.0p+0", "0x1.1db6db6db6db7p+5", "0x1.8cffae3faaa58p+5", "0x1.13d061aa309a1p+6",
                        "0x1.7f3e0745fe1d0p+6", "0x1.0a41b8b5fb85bp+7", "0x1.71f667c72c24ap+7", "0x1.0107d750b8841p+8",
                        "0x1.65249547833bfp+8", "0x1.f03f9ad9ccd20p+8", "0x1.58c47acdb0dd6p+9", "0x1.df0d8a187ba1fp+9",
                        "0x1.4cd2279605d93p+10", "0x1.ce7402b10d781p+10", "0x1.4149cdd14246ap+11",
                        "0x1.be6dbb88e1a12p+11", "0x1.3627c16e82b5ep+12", "0x1.aef59a684e38bp+12",
                        "0x1.2b6876efec038p+13", "0x1.a006b25ab59e9p+13", "0x1.21088249b659dp+14",
                        "0x1.919c421d0562bp+14", "0x1.170495cb3b82fp+15", "0x1.83b1b29a1ec2fp+15",
                        "0x1.0d598111af9a4p+16", "0x1.76429574ad72bp+16", "0x1.040430042e74dp+17",
                        "0x1.694aa39df55b1p+17", "0x1.f60353b195e8fp+17", "0x1.5cc5bbf92481ep+18",
                        "0x1.b3f7249249249p+21"],
    "mutrate/bins": ["0x0.0p+0", "0x1.c92494339e977p+1", "0x1.69673776981b2p+3", "0x1.1db6dd398940bp+5",
                     "0x1.c3c106469711dp+6", "0x1.65249547833bfp+8", "0x1.1a58a48396015p+10", "0x1.be6dbb88e1a12p+11",
                     "0x1.60eece61d0fdep+13", "0x1.170495cb3b82fp+15", "0x1.b92a82e6f0190p+16",
                     "0x1.b3f7249249249p+21"],
    "mutrate/2,6": "rl_mutrate_epochs: bins `2,6`: epochs format is wrong. Specify x,y,stepsize.",
}
BINS = "2,6.5,0.5"


def epochs_hex(ep):
    return [x.hex() for x in ep.tolist()] if ep.dtype == np.float64 else ["%08x" % w for w in ep.view(np.uint32).tolist()]


@pytest.mark.parametrize("maker", ("coalrate", "mutrate"))
def test_epochs(maker):
    make = getattr(api, maker + "_epochs")
    default, binned = make(28.0), make(28.0, BINS)
    assert (len(default), len(binned)) == (31, 12)
    assert default.dtype == binned.dtype == (np.float32 if maker == "coalrate" else np.float64)
    assert epochs_hex(default) == EPOCHS[maker + "/default"]
    assert epochs_hex(binned) == EPOCHS[maker + "/bins"]
    assert message(lambda: make(28.0, "2,6")) == EPOCHS[maker + "/2,6"]


# ------------------------------------------------------------------------------------------------ the *_anc entry points
M = 4  # leaves of the files' three trees
FILE_TREES = [(10 * t, p, np.arange(1.0, 2 * M)) for t, p in enumerate((caterpillar(M), balanced(M), caterpillar(M)))]
# one SNP per tree on branch 0 | the tree indices fall on line 3
TREE_OF_SNP = {"good": (0, 1, 2), "falls": (1, 0, 2)}


def mut_bytes(mode, trees_of_snps):
    pos = [(100 + 10 * k, 10, t) for k, t in enumerate(trees_of_snps)]
    if mode in ("coalrate", "coaltree"):
        return cc.mut_text(pos)
    if mode == "frequency":
        return fc.mut_text([(p, d, t, [0], 0, 0.0) for p, d, t in pos])
    if mode == "mutrate":
        return mc.mut_text([(p, d, t, [0], 0, 0.0, 1.0) for p, d, t in pos])
    return (xc.MUT_HEAD + "".join("%d;%d;%d;rs%d;%d;0;0;0;0.0;1.0;A/C;G;T;\n" % (k, p, d, k, t)
                                  for k, (p, d, t) in enumerate(pos))).encode()


def anc_call(mode, ep32=EP32):
    ep64 = ep32.astype(np.float64)
    return {"coalrate": lambda: api.coalrate_anc("t.anc", "t.mut", ep32),
            "coaltree": lambda: api.coaltree_anc("t.anc", "t.mut", ep64),
            "frequency": lambda: api.frequency_anc("t.anc", "t.mut", ep32, "t.freq", "t.lin"),
            "mutrate": lambda: api.mutrate_anc("t.anc", "t.mut", ep64),
            "mutctx": lambda: api.mutctx_anc("t.anc", "t.mut", "mask.fa", "ancestor.fa", ep64)}[mode]


def write_files(mode, mut_kind, trees):
    files = {"t.anc": cc.anc_text(M, trees), "t.mut": mut_bytes(mode, TREE_OF_SNP[mut_kind]),
             "ancestor.fa": xc.fasta_text("ancestor", "ACGT" * 1000), "mask.fa": xc.fasta_text("mask", "P" * 4000)}
    for name, data in files.items():
        with open(name, "wb") as f:
            f.write(data)


ANC_MESSAGES = {
    "coalrate/falls": "CoalescentRateForSection: t.mut: line 3: tree index 0 after 1: the tree indices must not fall",
    "coaltree/falls": "CoalRateForTree: t.mut: line 3: tree index 0 after 1: the tree indices must not fall",
    "frequency/falls": "Frequency: t.mut: line 3: tree index 0 after 1: the tree indices must not fall",
    "mutrate/falls": "AvgMutationRate: t.mut: line 3: tree index 0 after 1: the tree indices must not fall",
    "mutctx/falls": "MutationRateWithContext: t.mut: line 3: tree index 0 after 1: the tree indices must not fall",
    "coalrate/equal": "rl_coalrate_anc: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "coaltree/equal": "rl_coaltree_anc: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "frequency/equal": "rl_frequency_anc: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "mutrate/equal": "rl_mutrate_anc: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
    "mutctx/equal": "rl_mutctx_anc: epoch boundary 2 (5) is not finite and above boundary 1 (5)",
}
# a tree of the file that fails a mode's checks: every mode names the file and the tree's number in it
ANC_NEGATIVE = "t.anc: tree 1: branch length -0.5 of node 2 is negative or not finite"
ANC_PARENT = "t.anc: tree 2: parent 2 of node 4 does not have a label above its child's"
ANC_MODES = ("coalrate", "coaltree", "frequency", "mutrate", "mutctx")


@pytest.mark.parametrize("mode", ANC_MODES)
def test_anc_refusal(mode, tmp_path, monkeypatch):
    """relative paths, so that the messages name the same files everywhere"""
    monkeypatch.chdir(tmp_path)
    write_files(mode, "falls", FILE_TREES)
    assert message(anc_call(mode)) == ANC_MESSAGES[mode + "/falls"]
    bad = [(pos, p, bl.copy()) for pos, p, bl in FILE_TREES]
    bad[1][2][2] = -0.5
    write_files(mode, "good", bad)
    assert message(anc_call(mode)) == ANC_NEGATIVE
    low = [(pos, p.copy(), bl) for pos, p, bl in FILE_TREES]
    low[2][1][4] = 2
    write_files(mode, "good", low)
    assert message(anc_call(mode)) == ANC_PARENT
    write_files(mode, "good", FILE_TREES)
    assert message(anc_call(mode, np.array([0.0, 5.0, 5.0], np.float32))) == ANC_MESSAGES[mode + "/equal"]
    assert message(anc_call(mode)) is None
