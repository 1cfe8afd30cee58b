"""Segmented passes of K1's merged launch (rl_set_paint_segments; paint_pass.h, DESIGN.md "Segmented passes"): a pass
cut into segments that hand their state over through HBM paints what the whole pass paints.  Every stone key of every
window is compared bit for bit two ways: segments (s_b, s_f) against set_paint_segments(1, 1) of the same library, and
the segmented run against the oracle at a handful of targets; in the `exact` and `lanes` orders.

The shapes are small on purpose: with a few hundred workgroups everything is resident at once, later segments really
do wait for earlier ones, and a CU reads state lines again that another CU has rewritten -- where a wrong hand-off
shows.  Every context paints twice per setting and the two runs are compared as well."""
import numpy as np
import pytest

import rlutil
from relate_amd import api
from test_edge_gpu import random_chunk
from test_paint_gpu import bits_equal, oracle_stones
from test_tile_fit_gpu import last_live_target, target_ranges

pytestmark = pytest.mark.gpu

MODES = {"exact": api.RL_SUM_EXACT, "lanes": api.RL_SUM_LANES}
STONE_KEYS = ("alpha", "beta", "ls_alpha", "ls_beta", "bsnp_begin", "bsnp_end")
AUTO_DEFAULT = (1, 8)  # launch.h PAINT_SEGMENTS_AUTO_*


def painted(ctx, mode, windows, launched=None):
    """paint and fetch; launched: the segments the launch must have had (what rl_paint launched, not the setting)"""
    ctx.paint(MODES[mode])
    if launched is not None:
        assert ctx.paint_launched_segments() == launched, (mode, launched, ctx.paint_launched_segments())
    return [ctx.stones(w) for w in windows]


def launch_of(N, mode, setting):
    """what a paint() of N haplotypes under `setting` must launch: the setting -- but the loose variant of the S = 8
    tile (q = N // 64 < 4) has no segmented kernel in the `lanes` order and runs unsegmented"""
    S, waves, tail, live = api.tile_fit(N)
    return (1, 1) if mode == "lanes" and S == 8 and tail == 8 else setting


def assert_same(a, b, what):
    for w, (x, y) in enumerate(zip(a, b)):
        for key in STONE_KEYS:
            assert bits_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (what, w, key)


def assert_oracle(ch, run, windows, k0, targets, mode, cache):
    for k in targets:
        key = (k, mode == "lanes")
        if key not in cache:
            cache[key] = oracle_stones(ch, k, mode == "lanes")
        bb, be, al, bt, la, lb = cache[key]
        r = k - k0
        for st, w in zip(run, windows):
            assert st["bsnp_begin"][r] == bb[w] and st["bsnp_end"][r] == be[w], (mode, k, w)
            assert bits_equal(st["ls_alpha"][r], la[w]) and bits_equal(st["ls_beta"][r], lb[w]), (mode, k, w)
            assert bits_equal(st["alpha"][r], al[w]) and bits_equal(st["beta"][r], bt[w]), (mode, k, w)


def check_segments(ch, settings, ranges=None, window_range=None, modes=("exact", "lanes"), extra_targets=()):
    """Per target range and order: the unsegmented paint, then every setting twice -- each against the unsegmented
    stones, the second run against the first, the first setting's against the oracle."""
    N = ch.N
    kl = last_live_target(N)
    cache = {}
    windows = list(range(ch.W)) if window_range is None else list(range(window_range[0], window_range[1] + 1))
    for k0, k1 in ranges or [(0, N)]:
        ctx = api.Context()
        ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
        if (k0, k1) != (0, N):
            ctx.set_target_range(k0, k1)
        if window_range is not None:
            ctx.set_window_range(*window_range)
        targets = sorted(k for k in set([0, 1, kl, N // 2, N - 2, N - 1]) | set(extra_targets) if k0 <= k < k1)
        for mode in modes:
            ctx.set_paint_segments(1, 1)
            assert ctx.paint_segments() == (1, 1)
            whole = painted(ctx, mode, windows, (1, 1))
            for n, (sb, sf) in enumerate(settings):
                ctx.set_paint_segments(sb, sf)
                assert ctx.paint_segments() == (sb, sf)
                first = painted(ctx, mode, windows, launch_of(N, mode, (sb, sf)))
                assert_same(first, whole, (mode, sb, sf, "against the whole passes"))
                again = painted(ctx, mode, windows, launch_of(N, mode, (sb, sf)))
                assert_same(again, first, (mode, sb, sf, "second run"))
                if n == 0:
                    assert_oracle(ch, first, windows, k0, targets, mode, cache)
        ctx.close()


@pytest.mark.parametrize("N", [389, 965, 1925, 3008, 5000, 5120])
def test_every_tile_and_fit_variant(N):
    ch = random_chunk(N, 300, 0.13, seed=N, wb=[0, 90, 210, 300], special="flat_targets")
    check_segments(ch, [(2, 3), (8, 8), (1, 5)], ranges=target_ranges(N))


@pytest.mark.parametrize("N", [5893, 10000])
def test_two_waves_per_target(N):
    """the WaveLink restarts in both waves of a segment together, and the barrier stands before the flag"""
    ch = random_chunk(N, 300, 0.13, seed=N, wb=[0, 90, 210, 300], special="flat_targets")
    check_segments(ch, [(3, 2)], ranges=target_ranges(N))


def test_more_segments_than_steps():
    """N = 64, L = 40: some targets walk fewer steps than there are segments (target 0 two sites in all), so empty
    segments must still take the state over and publish it"""
    ch = random_chunk(64, 40, 0.13, seed=64, wb=[0, 15, 40], special="flat_targets")
    check_segments(ch, [(17, 17)])
    # (N = 64 runs the loose S = 8 variant, segmented in the `exact` order only; N = 300 has the `lanes` twin too)
    ch = random_chunk(300, 40, 0.13, seed=300, wb=[0, 15, 40], special="flat_targets")
    assert launch_of(300, "lanes", (17, 17)) == (17, 17)
    check_segments(ch, [(17, 17)])


def test_stones_at_the_seams():
    """Target N - 1 is derived everywhere: it visits every SNP, so its visited index is the SNP.  With 121 SNPs and 4
    segments the forward pass's segment 0 walks steps 1 .. 30, the backward pass's steps 119 .. 90; the window
    boundaries put a forward stone at step 30 and one at 31, a backward stone at 90 and one at 89 -- the last step of
    a segment and the first of the next.  The same target has stones at the first and at the last site."""
    N, L = 300, 121  # (q = 4: the fitted S = 8 variant, which both orders have a twin of)
    assert api.paint_segment_range(1, L, 4, 0) == (1, 31) and api.paint_segment_range(0, L - 1, 4, 0) == (0, 30)
    ch = random_chunk(N, L, 0.13, seed=7, wb=[0, 31, 32, 89, 90, L], special="flat_targets")
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.set_paint_segments(1, 1)
    ctx.paint(api.RL_SUM_EXACT)
    st = [ctx.stones(w) for w in range(ch.W)]
    ctx.close()
    assert {30, 31} <= set(int(s["bsnp_begin"][N - 1]) for s in st)
    assert {89, 90} <= set(int(s["bsnp_end"][N - 1]) for s in st)
    assert st[0]["bsnp_begin"][N - 1] == 0 and st[-1]["bsnp_end"][N - 1] == L - 1
    check_segments(ch, [(4, 4), (3, 7)])


def test_window_range_and_target_range():
    """a window range that cuts both passes short (the segments divide the shortened walk) on a context that holds a
    part of the targets (nloc != N: chains and stone rows are relative to the range)"""
    ch = random_chunk(700, 300, 0.13, seed=11, wb=[0, 60, 130, 200, 260, 300], special="flat_targets")
    check_segments(ch, [(3, 4)], ranges=[(100, 333)], window_range=(1, 3), extra_targets=(100, 200, 332))


def test_dense_panel_rescales_next_to_seams():
    ch = random_chunk(389, 400, 0.5, 5, wb=[0, 100, 250, 400])
    ch.theta = 0.001
    check_segments(ch, [(4, 4)])


def test_uneven_load():
    """dense and sparse targets mixed (no flat targets): the chains are of very different lengths, so the segments of
    one round end at very different times"""
    N, L = 700, 200
    rng = np.random.RandomState(3)
    dens = np.where(rng.rand(N) < 0.5, 0.02, 0.6)
    seq = (rng.rand(L, N) < dens[None, :]).astype(np.uint8) + ord("0")
    bp = 1000 + np.cumsum(rng.randint(1, 200, L)).astype(np.int32)
    rpos = np.concatenate([bp, [bp[-1] + 100]]).astype(np.float64) * 1e-8
    r = np.maximum(np.diff(rpos), 1e-10) * 2500
    ch = rlutil.Chunk(seq, r, rpos, np.array([0, 70, 140, L], np.int32), bp)
    check_segments(ch, [(5, 3)])


def test_switch_and_rule():
    """set_paint_segments(1, 1) and set_paint_split(True) launch the unsegmented kernels and give the same bytes; the
    automatic rule is off for a launch that fits the chip at once and the default for N = 5000"""
    ch = random_chunk(389, 200, 0.13, seed=2, wb=[0, 80, 200], special="flat_targets")
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    assert ctx.paint_segments() == (1, 1)  # automatic: 778 workgroups, thousands of slots
    windows = list(range(ch.W))
    for mode in MODES:
        ctx.set_paint_segments(0, 0)
        auto = painted(ctx, mode, windows, (1, 1))
        ctx.set_paint_segments(4, 4)
        seg = painted(ctx, mode, windows, (4, 4))
        ctx.set_paint_segments(1, 1)
        off = painted(ctx, mode, windows, (1, 1))
        ctx.set_paint_split(True)
        ctx.set_paint_segments(4, 4)
        assert ctx.paint_segments() == (1, 1)  # one launch per direction: never segmented
        split = painted(ctx, mode, windows, (1, 1))
        ctx.set_paint_split(False)
        assert_same(seg, off, (mode, "segments against off"))
        assert_same(auto, off, (mode, "automatic against off"))
        assert_same(split, off, (mode, "split against off"))
    ctx.set_paint_segments(3, 3)  # the serial order has no twin: unsegmented, same bytes as ever
    a = painted(ctx, "exact", windows, (3, 3))
    ctx.paint(api.RL_SUM_EXACT_SERIAL)
    assert ctx.paint_launched_segments() == (1, 1)
    ctx.set_paint_fit(0)  # the loose S = 8 variant has no `lanes` twin: unsegmented there, segmented in `exact`
    c = painted(ctx, "lanes", windows, (1, 1))
    ctx.set_paint_fit(1)
    assert_same(c, painted(ctx, "lanes", windows, (3, 3)), "lanes, loose S = 8 unsegmented against fitted in segments")
    painted(ctx, "exact", windows, (3, 3))
    b = [ctx.stones(w) for w in windows]
    assert_same(a, b, "serial order under a segment setting")
    ctx.close()
    big = random_chunk(5000, 30, 0.13, seed=1, wb=[0, 30])
    ctx = api.Context()
    ctx.set_chunk(big.seq, big.r, big.rpos, big.wb)
    assert ctx.paint_segments() == AUTO_DEFAULT  # 10,000 workgroups on 2048 slots
    ctx.set_target_range(0, 900)
    assert ctx.paint_segments() == (1, 1)  # 1800 workgroups fit
    with pytest.raises(api.RelateError):
        ctx.set_paint_segments(-1, 2)
    ctx.close()
