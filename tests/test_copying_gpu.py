"""CopyingMatrix on the GPU: rl_window_copying / rl_copying_matrix / `Relate --mode CopyingMatrix` against the numpy
restatement of the definition on the oracle's posterior rows (copying_cases.py), bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import copying_cases as cc
import rlutil
from relate_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


def oracle_paint(ch, pdir):
    o = rlutil.oracle()
    d = ch.ro()
    assert o.ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), ch.W, pdir.encode(), 4, 0, None, None) == 0


def check_all_windows(ch, pdir, ctx, targets=None):
    """every window of the chunk, one after another into one matrix, device against restatement"""
    want = np.zeros((ch.N if targets is None else len(targets), ch.N), np.float64)
    got = None
    for w in range(ch.W):
        pf = os.path.join(pdir, "relate_%d.bin" % w)
        ow = cc.OracleWindow(ch, pf, w)
        cc.add_window(ow, want, targets)
        ow.close()
        win = ctx.open_window(w, pf, int(ch.wb[w]), api.RL_SUM_EXACT)
        got = win.copying(got)
        win.close()
        assert np.array_equal(cc.bits(got), cc.bits(want)), (w, np.abs(got - want).max())
    return got


@pytest.mark.parametrize("N,L,budget,seed", [
    (8, 600, 3000, 3),          # fewer donors than a wavefront has lanes
    (65, 1200, 30000, 2),       # a row tail
    (130, 1500, 200000, 5),
    (600, 900, 3000000, 11),    # several columns per thread
])
def test_windows_match_the_restatement(tmp_path, N, L, budget, seed):
    ch = rlutil.synth_chunk(N, L, seed=seed, budget=budget)
    oracle_paint(ch, str(tmp_path))
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    got = check_all_windows(ch, str(tmp_path), ctx)
    ctx.close()
    assert not np.diag(got).any()
    rel = np.abs(np.array([sum(float(v) for v in got[n]) for n in range(N)]) / ch.L - 1.0)
    assert rel.max() <= 1e-10, rel.max()


def test_two_wavefronts_per_target(tmp_path):
    """N = 5300: RePaint's 128-lane layout, 21 accumulators per thread"""
    from test_edge_gpu import random_chunk
    N = 5300
    ch = random_chunk(N, 70, 0.15, seed=5, wb=[0, 30, 70])
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    ctx.write_paint_files(str(tmp_path))
    check_all_windows(ch, str(tmp_path), ctx)
    ctx.close()


INSTANTIATIONS = (1, 2, 4, 8, 12, 16, 20, 24, 32, 40)  # launch_copying: copying_reduce_kernel<K> takes N <= 256 K
# the largest N of every instantiation (a full tile: each thread owns a real column in every slot) and the smallest of
# the next; 5120 / 5121 is also the switch from one wavefront per target to two in the painting layout
EDGES = [256 * K + d for K in INSTANTIATIONS for d in (0, 1) if 256 * K + d <= 10240]
# N = 256 K has rem == 0 and 256 K + 1 has rem == 1 in the painting layout (q = N / lanes, rem = N % lanes, 64 or 128
# lanes): the largest remainders, one and two wavefronts, and q + 1 = 80 = the largest register tile
LARGEST_REM = [4095, 8191, 10239]
ENDS = 16  # recipients painted at either end of the panel


def edge_chunk(N):
    from test_edge_gpu import random_chunk
    return random_chunk(N, 70, 0.15, seed=5, wb=[0, 30, 70])


def reduce_of_the_windows_own_rows(ch, k0, k1):
    """The reduce kernel alone: the recipients k0 .. k1-1 painted on the device, and per window the device's
    win.copying() against cc.reduce_rows (numpy) of the posterior rows the SAME window hands out through
    win.topology(n) -- host code that undoes the [wave][register][lane] layout, held to the oracle in
    test_window_gpu.py -- with the weights of cc.row_weights on the oracle's boundary SNPs.  Both windows go into
    one matrix, so the second launch starts from the C the first one left.  Window.topology and Window.rows take
    the GLOBAL index of the recipient under a target range; win.copying() returns the context's rows.
    -> (C [k1-k0][N], layout (tile, waves))"""
    o = rlutil.oracle()
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.set_target_range(k0, k1)
    ctx.paint(api.RL_SUM_EXACT)
    layout = (ctx.tile, ctx.waves)
    want = np.zeros((k1 - k0, ch.N), np.float64)
    got = None
    for w in range(ch.W):
        win = ctx.open_window(w, None, None, api.RL_SUM_EXACT)
        for i, n in enumerate(range(k0, k1)):
            top, _ = win.topology(n)
            bb, be = cc.plan_bounds(o, ch, n)
            site = cc.row_sites(ch, n, bb[w], be[w])
            assert top.shape == (len(site), ch.N) and not top[:, n].any(), (w, n)  # the own-donor slot is pinned to 0
            cc.reduce_rows(top, cc.row_weights(site, ch.rpos, ch.wb[w], ch.wb[w + 1]), want[i])
        got = win.copying(got)
        win.close()
        assert got.shape == want.shape and np.array_equal(cc.bits(got), cc.bits(want)), (w, np.abs(got - want).max())
    ctx.close()
    return got, layout


@pytest.mark.parametrize("N", EDGES + LARGEST_REM)
def test_every_instantiation_at_both_of_its_edges(tmp_path, N):
    """Every K of launch_copying at its largest and its smallest N (N = 256 K: rem == 0 in the layout, every thread
    owns a real column in every slot; 256 K + 1: one column in the last slot, rem == 1), either side of the one-wave /
    two-wave switch of the layout, N = 10,240, and three sizes with the largest remainder.  The first and the last 16
    recipients: the pinned own-donor entry falls in the first lane of the first wavefront and in the last lane of
    the last.  The yardstick is
    reduce_of_the_windows_own_rows; at N = 257, 2049 and 5121 (one wavefront with a short and a long tile, two
    wavefronts) the result is also held to the full oracle route -- the oracle's own painting and RePaint of every
    target -- restricted to these recipients."""
    ch = edge_chunk(N)
    ranges = [(0, ENDS), (N - ENDS, N)]
    rows, layouts = zip(*[reduce_of_the_windows_own_rows(ch, k0, k1) for k0, k1 in ranges])
    assert layouts[0] == layouts[1] and layouts[0][1] == (1 if N <= 5120 else 2), layouts
    got = np.concatenate(rows)
    targets = [n for k0, k1 in ranges for n in range(k0, k1)]
    for i, n in enumerate(targets):
        assert cc.bits(got[i, n:n + 1])[0] == 0, (n, got[i, n])  # +0.0 on the diagonal
    rel = np.abs(np.array([sum(float(v) for v in got[i]) for i in range(len(targets))]) / ch.L - 1.0)
    assert rel.max() <= 1e-10, rel.max()
    assert got.min() >= 0.0 and (got > 0.0).sum(axis=1).min() >= 1
    if N in (257, 2049, 5121):
        oracle_paint(ch, str(tmp_path))
        want = np.zeros((len(targets), N), np.float64)
        for w in range(ch.W):
            ow = cc.OracleWindow(ch, os.path.join(str(tmp_path), "relate_%d.bin" % w), w)
            cc.add_window(ow, want, targets)
            ow.close()
        assert np.array_equal(cc.bits(got), cc.bits(want)), np.abs(got - want).max()


def test_one_haplotype_too_many_has_no_layout():
    """N = 10,241: refused when the chunk is set, before any CopyingMatrix kernel could be asked for it"""
    ch = edge_chunk(10241)
    ctx = api.Context()
    with pytest.raises(api.RelateError, match="exceeds the largest"):
        ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.close()


def test_bounded_window_has_the_bits_of_the_whole_one(tmp_path):
    ch = rlutil.synth_chunk(96, 1400, seed=9, budget=60000)
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    for w in sorted(set([0, ch.W - 1])):
        s0 = int(ch.wb[w])
        full = ctx.open_window(w, None, s0, api.RL_SUM_EXACT)
        rows = sum(full.rows(n) for n in range(ch.N))
        part = ctx.open_window(w, None, s0, api.RL_SUM_EXACT, max_rows=max(1, int(0.08 * rows)))
        A, B = full.copying(), part.copying()
        assert full.repaints == 1 and part.repaints > 2, part.repaints
        assert A.any() and np.array_equal(cc.bits(A), cc.bits(B)), (w, np.abs(A - B).max())
        # the bounded window still serves matrices afterwards, from its own cursors
        assert np.array_equal(full.matrix(s0).view(np.uint32), part.matrix(s0).view(np.uint32))
        part.close()
        full.close()
    ctx.close()


def test_target_range_gives_those_rows(tmp_path):
    ch = rlutil.synth_chunk(130, 1500, seed=5, budget=200000)
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    full, W = ctx.copying_matrix()
    assert W == ch.L
    ctx.close()
    k0, k1 = 37, 101
    sub = api.Context()
    sub.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    sub.set_target_range(k0, k1)
    sub.paint(api.RL_SUM_EXACT)
    rows, W2 = sub.copying_matrix()
    sub.close()
    assert W2 == W and rows.shape == (k1 - k0, ch.N)
    assert np.array_equal(cc.bits(rows), cc.bits(full[k0:k1]))


def test_copying_matrix_over_gpu_paint_equals_the_window_sum(tmp_path):
    ch = rlutil.synth_chunk(96, 1400, seed=9, budget=60000)
    assert ch.W >= 3
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    Cm, W = ctx.copying_matrix(1, ch.W - 1)
    assert W == ch.L - ch.wb[1]
    acc = None
    for w in range(1, ch.W):
        win = ctx.open_window(w, None, None, api.RL_SUM_EXACT)
        acc = win.copying(acc)
        win.close()
    assert np.array_equal(cc.bits(Cm), cc.bits(acc))
    with pytest.raises(api.RelateError):
        ctx.copying_matrix(1, ch.W)
    ctx.close()


def test_lanes_mode_equals_the_host_twin_on_the_windows_rows(tmp_path):
    ch = rlutil.synth_chunk(130, 1500, seed=5, budget=200000)
    o = rlutil.oracle()
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_LANES)
    w = ch.W // 2
    win = ctx.open_window(w, None, None, api.RL_SUM_LANES)
    got = win.copying()
    for n in range(ch.N):
        top, _ = win.topology(n)
        bb, be = cc.plan_bounds(o, ch, n)
        site = cc.row_sites(ch, n, bb[w], be[w])
        wt = api.copying_weights_host(site, ch.rpos, ch.wb[w], ch.wb[w + 1])
        want = api.copying_rows_host(top, wt)
        assert np.array_equal(cc.bits(got[n]), cc.bits(want)), n
    win.close()
    ctx.close()


def test_cli_writes_the_matrix_of_the_api(tmp_path):
    ch = rlutil.synth_chunk(70, 1300, seed=8, budget=40000)
    assert ch.W >= 3
    work = tmp_path / "work"
    ch.write(str(work / "out"))
    a, b = 1, ch.W - 1
    p = subprocess.run([CLI, "--mode", "CopyingMatrix", "--chunk_index", "0", "--first_section", str(a),
                        "--last_section", str(b), "-o", "out"], cwd=str(work), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    f = api.read_cpy(str(work / "out.cpy"))
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.set_window_range(a, b)
    ctx.paint(api.RL_SUM_EXACT)
    Cm, W = ctx.copying_matrix(a, b)
    ctx.close()
    assert (f["N"], f["chunk"], f["first_snp"], f["end_snp"], f["W"]) == (ch.N, 0, int(ch.wb[a]), ch.L, W)
    assert np.array_equal(cc.bits(f["C"]), cc.bits(Cm))
    lines = dict(l.split(" ", 1) for l in p.stdout.decode().strip().split("\n"))
    assert lines["haplotypes"] == str(ch.N) and lines["windows"] == str(b - a + 1) and lines["snps"] == str(W)
    share = Cm / W
    i, j, v = lines["max_share"].split()
    assert float(v) == share.max() and share[int(i), int(j)] == share.max()
    assert float(lines["max_rowsum_error"]) <= 1e-10
    eff = float(lines["mean_effective_donors"])
    assert 1.0 <= eff <= ch.N - 1 and abs(eff - np.mean(1.0 / (share ** 2).sum(axis=1))) <= 1e-9 * eff
    p = subprocess.run([CLI, "--help"], cwd=str(work), stderr=subprocess.PIPE)
    assert b"CopyingMatrix" in p.stderr
