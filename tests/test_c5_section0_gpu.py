"""BASELINE.json config #5 (synthetic N = 10,000 x L = 200,000, seed 1, --memory 25: 327 windows), section 0 at FULL
length through the command line, against the unmodified reference (tests/golden/c5_first.npz: `Relate --mode
BuildTopology` of section 0 -- md5 of .anc and .mut, the .mut in full, every tree's position and parent array).

    Relate --mode PaintBuildTopology --chunk_index 0 --first_section 0 --last_section 0

paints window 0 alone (rl_stage_opts.paint_windows: 2 x 0.4 GB of stepping stones in HBM, where a Paint of all 327
windows is 2 x 131 GB in pinned host memory) with all 10,000 targets on the two-wave tile, re-paints the window with
the two-wave RePaint kernels and builds the section's 129 trees with the device's workers (the L_HOT x 20 builder of
N > 5120).  The child's time limit is five times the 58 s it measured on one MI355X (profiles/window_range.json:
2.8 s to the end of Paint, 53 s of tree builds) -- the chunk files are 2 GB, written and read back on the host."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import rlutil
from relate_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
GOLD = os.path.join(ROOT, "tests", "golden", "c5_first.npz")
CHILD_TIMEOUT_S = 300


def md5_file(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return np.frombuffer(h.digest(), dtype=np.uint8)


def md5(b):
    return np.frombuffer(hashlib.md5(b).digest(), dtype=np.uint8)


@pytest.fixture(scope="module")
def chunk_dir(tmp_path_factory):
    """the seed-1 chunk on disc, as tools/c5_job_one_gpu.py (tools/chunk_c3_fused.py) makes it"""
    z = np.load(GOLD)
    N, L, W, seed = [int(x) for x in z["meta"]]
    assert (N, L, W) == (10000, 200000, 327)
    lib = api.lib()
    rw = (N + 31) // 32
    seq = np.zeros((L, N), dtype=np.uint8)
    bits = np.zeros((L, rw), dtype=np.uint32)
    bp = np.zeros(L, dtype=np.int32)
    r = np.zeros(L)
    rpos = np.zeros(L + 1)
    assert lib.rl_synth_panel(N, L, C.c_uint64(seed), 100, 1, seq.ctypes.data_as(C.c_void_p),
                              bits.ctypes.data_as(C.c_void_p), rw, bp.ctypes.data_as(C.c_void_p),
                              r.ctypes.data_as(C.c_void_p), rpos.ctypes.data_as(C.c_void_p)) == 0
    budget = float(z["mem"][0]) * 1e9 / 4.0 - (2.0 * N * N + 3.0 * N)
    wb = np.zeros(L + 2, dtype=np.int32)
    assert lib.rl_synth_windows_bits(N, L, bits.ctypes.data_as(C.c_void_p), rw, C.c_double(budget),
                                     wb.ctypes.data_as(C.c_void_p), 499) == W
    assert np.array_equal(wb[:W + 1], z["wb"])
    del bits
    work = str(tmp_path_factory.mktemp("c5s0"))
    d = os.path.join(work, "out")
    os.makedirs(d)
    lib.rl_write_chunk_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
    assert lib.rl_write_chunk_files(d.encode(), 0, N, L, seq.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p),
                                    r.ctypes.data_as(C.c_void_p), rpos.ctypes.data_as(C.c_void_p),
                                    wb.ctypes.data_as(C.c_void_p), W) == 0
    del seq
    for key in z.files:  # the chunk files the reference was given, where the fixture says
        if key.startswith("in_md5/"):
            assert np.array_equal(md5_file(os.path.join(d, key[7:])), z[key]), key
    return z, work


def test_section_0_of_config_5_is_the_references(chunk_dir):
    z, work = chunk_dir
    # (trees on the device: a call for one section builds on the host unless told, treeseq.cpp; the timing lines say
    #  which builder built them)
    p = subprocess.run([CLI, "--mode", "PaintBuildTopology", "--chunk_index", "0", "--first_section", "0",
                        "--last_section", "0", "-o", "out"], cwd=work, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT_S,
                       env=dict(os.environ, RELATE_AMD_TIMING="1", RELATE_AMD_GPU_BUILD="1"))
    err = p.stderr.decode()
    print("\n".join(l for l in err.replace("\r", "\n").split("\n") if l.startswith("[fused stage]") or l.startswith("[stage]")
                    or l.startswith("[tree sequence]")))
    assert p.returncode == 0, err[-800:]
    m = re.search(r"\[fused stage\] windows 0-0 of 327 painted .* ([\d.]+) GB of stones in (HBM|pinned host memory)", err)
    assert m, "the stage did not say what it painted"
    assert m.group(2) == "HBM" and float(m.group(1)) < 1.0
    anc = os.path.join(work, "out", "chunk_0", "out_0.anc")
    mut = open(os.path.join(work, "out", "chunk_0", "out_0.mut"), "rb").read()
    assert mut == z["s0/mut"].tobytes(), "out_0.mut differs from the reference's"
    assert np.array_equal(md5_file(anc), z["s0/anc_md5"]), "out_0.anc differs from the reference's"
    _, trees = rlutil.parse_anc(anc)
    want = z["s0/tree_parent_md5"]
    assert len(trees) == len(want) == 129
    if "s0/tree_pos" in z.files:
        assert [t[0] for t in trees] == list(z["s0/tree_pos"]), "tree positions"
    for t, (tr, w) in enumerate(zip(trees, want)):
        assert np.array_equal(md5(tr[1].astype("<i4").tobytes()), w), "parent array of tree %d" % t
    m = re.search(r"\[tree sequence\] .*?(\d+) trees kept of (\d+) built.*?\((\d+) trees on the GPU, (\d+) on the host", err)
    assert m, "no [tree sequence] line in the stage's timing output"
    # (a tree that needs MinMatch's symmetric fallback is the host's by design, tree_builder.cpp:255-293: the rest are the device's)
    assert int(m.group(1)) == 129 and int(m.group(3)) > int(m.group(4)) and int(m.group(3)) + int(m.group(4)) >= 129, m.group(0)
