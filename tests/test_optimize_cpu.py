"""`Relate --mode OptimizeParameters` without a GPU: the ABI entries and their Python mirror, the mode's argument
checks and messages (pipeline/OptimizeParameters.cpp:25-34, :81-112 of the reference), and the mapping decision
(AncesTreeBuilder::MapMutation without random flipping, src/anc_builder.cpp:1064-1139) on hand-made trees."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from relate_amd import api
from test_makechunks import write_synth_haps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


def test_abi_entries_and_signatures():
    lib = api.lib()
    want = {"rl_optimize_section": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int)],
            "rl_stage_optimize_parameters": [C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float),
                                             C.c_int, C.c_void_p, C.POINTER(C.c_int)],
            "rl_debug_map_mutation": [C.c_int, C.c_void_p, C.c_void_p],
            "rl_debug_cancel_rowmin": [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p]}
    hdr = open(os.path.join(ROOT, "include", "relate_amd.h")).read()
    for name, argtypes in want.items():
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == argtypes, name
        assert getattr(lib, name).restype is C.c_int
        assert ("int %s(" % name) in hdr
    # bad arguments are refused before any device work
    counts = (C.c_int * 1)()
    th, fa = (C.c_float * 1)(1.0), (C.c_float * 1)(1.0)
    assert lib.rl_stage_optimize_parameters(b"/nonexistent", 0, th, 1, fa, 1, None, counts) == -1
    assert b"theta value has to be in (0,1)" in lib.rl_last_error()
    th[0], fa[0] = 0.5, 0.0
    assert lib.rl_stage_optimize_parameters(b"/nonexistent", 0, th, 1, fa, 1, None, counts) == -1
    assert b"rho value has to be positive" in lib.rl_last_error()
    assert lib.rl_optimize_section(None, 0, 0.001, 1.0, counts) == -1
    assert counts[0] == 0
    assert api.OPTIMIZE_THETAS == (1e-4, 1e-3, 1e-2, 1e-1) and api.OPTIMIZE_FACTORS == (0.001, 0.1, 1, 10, 100)


def test_mode_without_haps_prints_the_two_lines_and_help(tmp_path):
    p = subprocess.run([CLI, "--mode", "OptimizeParameters", "-o", "x"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().splitlines()
    assert out[0] == "Not enough arguments supplied."
    assert out[1] == "Needed: haps, sample, map, output. Optional: dist."
    assert any("OptimizeParameters" in line for line in out[2:]), out
    assert out[-1] == "Use to make smaller chunks from the data."
    assert os.listdir(str(tmp_path)) == []
    # the mode is in the list of modes the CLI names
    p = subprocess.run([CLI, "--help"], stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"OptimizeParameters" in p.stderr


@pytest.mark.parametrize("grid,message", [("0.01 1.0\n1 10\n", "Error: theta value has to be in (0,1)"),
                                          ("0.01 0.1\n1 0\n", "Error: rho value has to be positive")])
def test_bad_input_grid_is_refused_like_the_reference(tmp_path, grid, message):
    """the grid is read after MakeChunks (host code), before anything touches a GPU: message and exit status 1"""
    work = str(tmp_path)
    write_synth_haps(work, 8, 3000, seed=8)
    open(os.path.join(work, "grid.txt"), "w").write(grid)
    p = subprocess.run([CLI, "--mode", "OptimizeParameters", "--haps", "s.haps", "--sample", "s.sample", "--map",
                        "s.map", "--memory", "0.0002", "-i", "grid.txt", "-o", "job"], cwd=work,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1, p.stderr.decode()
    err = p.stderr.decode().splitlines()
    assert err[-1] == message, err[-5:]
    assert "Optimizing Parameters..." in err
    assert not os.path.exists(os.path.join(work, "job.opt"))


def balanced8():
    """leaves 0..7; 8 = (0,1), 9 = (2,3), 10 = (4,5), 11 = (6,7), 12 = (8,9), 13 = (10,11), 14 = root"""
    return np.array([8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, -1], np.int32)


def flags(N, carriers):
    f = np.zeros(N, np.uint8)
    f[list(carriers)] = 1
    return f


@pytest.mark.parametrize("carriers,want,why", [
    (range(8), 1, "all carriers: the root branch"),
    ((), 1, "no carrier: nothing to place"),
    ((0, 1, 2, 3), 1, "a clade (node 12): 0 misplaced leaves as it stands and flipped, the unflipped reading wins"),
    ((2, 3, 4, 5, 6, 7), 2, "the complement of clade 8 = (0,1) and no clade itself: maps with the alleles flipped"),
    ((0, 2), 3, "no clade: every branch fails a ratio test in either reading (thr = int(0.03 * 8) = 0)"),
])
def test_mapping_decision_on_hand_made_trees(carriers, want, why):
    assert api.map_mutation(balanced8(), flags(8, carriers)) == want, why


def test_mapping_decision_tolerates_thr_misplaced_leaves():
    """N = 40: thr = int(0.03 * 40) = 1.  A caterpillar whose clade {0..18} holds 19 of the 20 carriers: one misplaced
    leaf, all four ratio tests pass (1/20 < 0.3, 0/20 < 0.3, 19/19 > 0.7, 20/21 > 0.7) -> maps (1); a clade that IS the
    carrier set -> 1; two carriers at the two ends of the caterpillar -> 3"""
    N = 40
    parent = np.empty(2 * N - 1, np.int32)
    parent[0] = parent[1] = N
    for i in range(2, N):
        parent[i] = N + i - 1
        parent[N + i - 2] = N + i - 1
    parent[2 * N - 2] = -1
    assert api.map_mutation(parent, flags(N, list(range(19)) + [30])) == 1
    assert api.map_mutation(parent, flags(N, list(range(20)))) == 1
    assert api.map_mutation(parent, flags(N, (0, 39))) == 3
    with pytest.raises(api.RelateError):
        api.map_mutation(np.zeros(2 * N - 1, np.int32), flags(N, (0,)))
