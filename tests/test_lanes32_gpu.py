"""RL_SUM_LANES32 -- the fast mode of K1: packed-FP32 state in the stepping-stone pass (paint32_kernels.hip).  Not
bit-identical to the reference, and held bit for bit to an oracle of its own: RO_SUM_LANES32 (oracle/relate_oracle.c
paint_target_lanes32) restates the kernels' arithmetic step by step in plain C -- the float state, its single float
operations, the float chains of each lane's sum by register pair and half, the float reciprocal of the rescale --, and
tests/test_lanes32_oracle_cpu.py holds that restatement to the FP64 oracle and to a second restatement on the CPU.

compare() paints a chunk in the `lanes` and the `lanes32` order and checks
  * the floor, over every painted target: the stones within a relative 2e-4 of each stone's largest entry of the FP64
    `lanes` kernel's and the log scales within 1e-3 (gross errors; what float arithmetic explains is two orders below,
    see the CPU file);
  * the oracle, at a handful of targets (0, 1, the one whose own slot is the last live register, N/2, N-2, N-1): alpha,
    beta, both log scales and both boundaries of every window equal to RO_SUM_LANES32, to the bit.
Around it: every register tile on both sides of its tail, the switches that must not change a bit (one launch per
direction, the loose tile, the segment setting, a target range), the paint files, K2 on those files, and the CLI.
No tolerance but the floor is left: a disagreement with the oracle is a bug on one of the two sides, and the chunk
with a stone every seven sites (test_a_stone_every_few_sites) says at which step, in which pass, for which donors.

The distances against the REFERENCE are in tests/test_golden_gpu.py (synth70) and tests/test_n5000_gpu.py (the headline
tile), with the tolerance of SURVEY.md 7 H1."""
import ctypes as C
import os

import numpy as np
import pytest

import rlutil
from relate_amd import api
from rlutil import RO_SUM_LANES32, gpu_step
from test_edge_gpu import random_chunk
from test_paint_gpu import bits_equal, oracle_stones
from test_tile_fit_gpu import CASES, STONE_KEYS, last_live_target, target_ranges

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relate_amd", "Relate")
ORACLE_KEYS = ("bsnp_begin", "bsnp_end", "alpha", "beta", "ls_alpha", "ls_beta")  # the order of oracle_stones


def oracle_targets(N, k0, k1):
    return sorted(k for k in set([0, 1, last_live_target(N), N // 2, N - 2, N - 1]) if k0 <= k < k1)


def first_difference(ch, k, w, key, got, want):
    """where a stone leaves the oracle: the donors, and -- the stone belongs to a boundary site -- the step range"""
    bad = np.flatnonzero(np.atleast_1d(got).view(np.uint32) != np.atleast_1d(want).view(np.uint32))
    return dict(N=ch.N, target=k, window=w, key=key, sites=(int(ch.wb[w]), int(ch.wb[w + 1])), differing=len(bad),
                first=bad[:8].tolist(), got=np.atleast_1d(got)[bad[:4]].tolist(), want=np.atleast_1d(want)[bad[:4]].tolist())


def check_oracle(ch, stones, k0, k1, cache):
    """stones[w]: Context.stones(w) of a lanes32 paint of targets k0 .. k1 - 1"""
    for k in oracle_targets(ch.N, k0, k1):
        if k not in cache:
            cache[k] = oracle_stones(ch, k, RO_SUM_LANES32)
        r = k - k0
        for w in range(ch.W):  # (forward stones in the order they are written: the first differing one comes first)
            for key, want in zip(ORACLE_KEYS, cache[k]):
                got = stones[w][key][r]
                if key.startswith("bsnp"):
                    assert got == want[w], (k, w, key, int(got), int(want[w]))
                else:
                    assert bits_equal(got, want[w]), first_difference(ch, k, w, key, got, want[w])


def check_floor(a, b, w):
    """b, the lanes32 stones of window w, against a, the FP64 `lanes` kernel's"""
    assert np.array_equal(a["bsnp_begin"], b["bsnp_begin"]) and np.array_equal(a["bsnp_end"], b["bsnp_end"])
    for key in ("alpha", "beta"):
        scale = np.abs(a[key]).max(axis=1, keepdims=True)
        err = np.abs(a[key].astype(np.float64) - b[key]) / np.maximum(scale, 1e-300)
        assert np.isfinite(b[key]).all()
        assert err.max() <= 2e-4, (w, key, float(err.max()), np.unravel_index(err.argmax(), err.shape))
        assert np.array_equal(a[key] == 0, b[key] == 0) or np.abs(b[key][a[key] == 0]).max() <= 1e-30
    for key in ("ls_alpha", "ls_beta"):
        assert np.abs(a[key].astype(np.float64) - b[key]).max() <= 1e-3 * max(1.0, np.abs(a[key]).max() * 1e-3), (w, key)


def open_ctx(ch, painting=None):
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    if painting:
        ctx.set_painting(*painting)
    return ctx


def compare(ch, ranges=None, painting=None, oracle_chunk=None):
    """ch painted in both orders, all targets or the given ranges of them.  painting = (theta, rho): set_painting on the
    device; the oracle then paints oracle_chunk, which holds them."""
    cache = {}
    for k0, k1 in (ranges or [(0, ch.N)]):
        out = {}
        for name, mode in (("lanes", api.RL_SUM_LANES), ("lanes32", api.RL_SUM_LANES32)):
            ctx = open_ctx(ch, painting)
            if (k0, k1) != (0, ch.N):
                ctx.set_target_range(k0, k1)
            ctx.paint(mode)
            out[name] = [ctx.stones(w) for w in range(ch.W)]
            ctx.close()
        for w in range(ch.W):
            check_floor(out["lanes"][w], out["lanes32"][w], w)
        check_oracle(oracle_chunk or ch, out["lanes32"], k0, k1, cache)
    assert cache


@pytest.mark.parametrize("N,L,budget,seed", [(8, 600, 3000, 3), (64, 1500, 30000, 1), (65, 1200, 30000, 2),
                                             (130, 900, 200000, 4), (300, 2000, 400000, 5)])
def test_small_panels(N, L, budget, seed):
    compare(rlutil.synth_chunk(N, L, seed=seed, budget=budget))


@pytest.mark.parametrize("N", [1000, 2000, 2100, 3500, 5000, 5120])
def test_single_wave_tiles(N):
    compare(random_chunk(N, 420, 0.13, seed=N, wb=[0, 130, 300, 420], special="flat_targets"))


@pytest.mark.parametrize("N", [5121, 7000, 10240])
def test_two_wavefronts_per_target(N):
    compare(random_chunk(N, 90, 0.15, seed=N, wb=[0, 40, 90], special="flat_targets"))


def test_long_run_with_rescales():
    compare(random_chunk(700, 6000, 0.12, seed=77, wb=[0, 1500, 4000, 6000]))


# ---- every register tile, both sides of its tail ---------------------------------------------------------------------
def tile_chunk(N):
    return random_chunk(N, 300, 0.13, seed=N, wb=[0, 90, 210, 300], special="flat_targets")


@pytest.mark.parametrize("N,want", CASES)
def test_every_tile_and_tail(N, want):
    """the shapes of test_tile_fit_gpu.CASES: all six one-wave and all three two-wave tiles, with and without a partial
    last register (this mode has one variant per tile, the list's TAIL; from N = 3008 on ranges of 48 targets)"""
    ch = tile_chunk(N)
    ctx = open_ctx(ch)
    assert (ctx.tile, ctx.waves) == want[:2]
    ctx.close()
    compare(ch, target_ranges(N))


def test_wide_tail():
    compare(tile_chunk(4900), target_ranges(4900))  # q = 76 of S = 80: several tested registers


def test_dense_panel_many_rescales():
    ch = random_chunk(389, 400, 0.5, 5, wb=[0, 100, 250, 400])
    ch.theta = 0.001
    compare(ch)


def test_painting_parameters():
    """set_painting(theta, rho) on the device; the oracle gets theta and the scaled distances (Paint.cpp:57-59)"""
    ch = rlutil.synth_chunk(200, 1500, seed=7, budget=400000)
    theta, rho = 0.025, 3.0
    compare(ch, painting=(theta, rho), oracle_chunk=rlutil.Chunk(ch.seq, ch.r * rho, ch.rpos, ch.wb, ch.bp, theta))


def test_a_stone_every_few_sites():
    """N = 130, a window boundary every 7 SNPs: 58 stones a pass, so that a disagreement names its step range"""
    L = 400
    compare(random_chunk(130, L, 0.15, seed=131, wb=list(range(0, L, 7)) + [L]))


# ---- switches that must not change a bit -----------------------------------------------------------------------------
def painted(ch, k0, k1, setup=None):
    ctx = open_ctx(ch)
    if (k0, k1) != (0, ch.N):
        ctx.set_target_range(k0, k1)
    if setup:
        setup(ctx)
    ctx.paint(api.RL_SUM_LANES32)
    st = [ctx.stones(w) for w in range(ch.W)]
    ctx.close()
    return st


def same_stones(a, b, what, rows=slice(None)):
    for w in range(len(a)):
        for key in STONE_KEYS:
            assert bits_equal(a[w][key][rows].view(np.uint32), b[w][key].view(np.uint32)), (what, w, key)


@pytest.mark.parametrize("N", [453, 2100, 6021])
def test_switches_change_no_bit(N):
    """one launch per direction (the DIR 0 and DIR 1 instantiations against DIR 2), the loose tile and a segment
    setting (this mode has one variant and no segmented twin: both calls must be no-ops), and a target range against
    the same rows of the whole paint"""
    ch = tile_chunk(N)
    cache = {}
    for k0, k1 in target_ranges(N):
        base = painted(ch, k0, k1)
        check_oracle(ch, base, k0, k1, cache)
        same_stones(base, painted(ch, k0, k1, lambda c: c.set_paint_split(True)), "split")
        same_stones(base, painted(ch, k0, k1, lambda c: c.set_paint_fit(0)), "fit 0")
        same_stones(base, painted(ch, k0, k1, lambda c: c.set_paint_segments(2, 4)), "segments")
    k0, k1 = (N // 2 - 24, N // 2 + 24)
    part = painted(ch, k0, k1)
    ctx = open_ctx(ch)
    ctx.paint(api.RL_SUM_LANES32)
    for w in range(ch.W):  # (a window at a time: the whole paint of N = 6021 is 290 MB a window)
        same_stones([ctx.stones(w)], [part[w]], "range, window %d" % w, slice(k0, k1))
    ctx.close()


# ---- paint files, K2 on them, the CLI --------------------------------------------------------------------------------
def oracle_files(ch, folder, threads=4):
    d = ch.ro()
    order = rlutil.RoSumOrder(RO_SUM_LANES32, 0, 0)
    os.makedirs(folder, exist_ok=True)
    assert rlutil.oracle().ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), ch.W, folder.encode(), threads, 0,
                                          C.byref(order), None) == 0
    return [open(os.path.join(folder, "relate_%d.bin" % w), "rb").read() for w in range(ch.W)]


FILE_CHUNKS = {
    96: lambda: rlutil.synth_chunk(96, 1400, seed=9, budget=60000),
    130: lambda: random_chunk(130, 400, 0.15, seed=130, wb=[0, 150, 400]),
    5300: lambda: random_chunk(5300, 70, 0.15, seed=5, wb=[0, 30, 70]),
}


@pytest.mark.parametrize("N", sorted(FILE_CHUNKS))
def test_paint_files_and_repaint(tmp_path, N):
    """write_paint_files after a lanes32 paint: the oracle's files in the same order, byte for byte; a window opened
    from them with RL_SUM_LANES32 runs K2's `lanes` kernels (launch.h kernel_mode): posterior rows and log scales of
    ro_repaint_section, for which RO_SUM_LANES32 means the `lanes` order"""
    o = rlutil.oracle()
    ch = FILE_CHUNKS[N]()
    want = oracle_files(ch, str(tmp_path / "oracle"))
    ctx = open_ctx(ch)
    ctx.paint(api.RL_SUM_LANES32)
    gdir = str(tmp_path / "gpu")
    ctx.write_paint_files(gdir)
    for w in range(ch.W):
        assert open(os.path.join(gdir, "relate_%d.bin" % w), "rb").read() == want[w], w
    if N == 96:
        ctx.close()
        return
    d = ch.ro()
    order = rlutil.RoSumOrder(RO_SUM_LANES32, 0, 0)
    for w in range(ch.W):
        pf = os.path.join(gdir, "relate_%d.bin" % w)
        recs = rlutil.parse_paint_file(pf, N)
        win = ctx.open_window(w, pf, int(ch.wb[w]), api.RL_SUM_LANES32)
        for n in sorted(set([0, 1, N // 2, N - 1])):
            r = recs[n]
            D = win.rows(n)
            top = np.zeros((D + 1, N), np.float32)
            ls = np.zeros(D + 1, np.float32)
            ab, be = np.ascontiguousarray(r["alpha"]), np.ascontiguousarray(r["beta"])
            assert o.ro_repaint_section(C.byref(d), ab.ctypes.data_as(C.c_void_p), be.ctypes.data_as(C.c_void_p),
                                        r["bb"], r["be"], C.c_float(r["la"]), C.c_float(r["lb"]), n, C.byref(order),
                                        top.ctypes.data_as(C.c_void_p), ls.ctypes.data_as(C.c_void_p)) == D
            gtop, gls = win.topology(n)
            assert bits_equal(gls, ls[:D]), (w, n)
            assert bits_equal(gtop, top[:D]), (w, n)
        win.close()
    ctx.close()


def test_paint_through_the_cli(tmp_path):
    """`Relate --mode Paint --sum_mode lanes32` on a written chunk: the oracle's files"""
    ch = rlutil.synth_chunk(70, 1200, seed=12, budget=60000)
    ch.write(str(tmp_path / "out"))
    want = oracle_files(ch, str(tmp_path / "oracle"))
    p = gpu_step([CLI, "--mode", "Paint", "--sum_mode", "lanes32", "--chunk_index", "0", "-o", "out"], 120,
                 cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    pdir = tmp_path / "out" / "chunk_0" / "paint"
    for w in range(ch.W):
        assert open(str(pdir / ("relate_%d.bin" % w)), "rb").read() == want[w], w
