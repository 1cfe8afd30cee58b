"""K1's register tile fitted to N (rl_set_paint_fit, relate_amd/csrc/launch.h tile_fit): every variant of every tile
paints what the oracle paints, bit for bit, in all three FP64 sum orders, and what the loose variant of the same
library paints (set_paint_fit(0)), stone for stone and log scale for log scale.

The shapes are the smallest that reach each variant at each chunk width (forward chunks of 8 at S = 8, of 16 from
S = 16 on; backward chunks of 4), with and without a partial last register, and the two-wave kernels.  Each case
checks, among others, the target whose own slot -- pinned to +0.0 in every step -- sits in the last live register.
From N = 3008 on the targets are painted as ranges of 48 (rl_set_target_range: the first, the one that begins at
that target, the middle, the last), which keeps the stones of a case to megabytes; the kernels paint each target on
its own.  (In the `lanes` order two tiles have the loose variant alone -- S = 32 with one wave, N = 1925 here, and
S = 64 with two: there the two runs launch the same kernel and only the oracle comparison says anything.)"""
import numpy as np
import pytest

from relate_amd import api
from test_edge_gpu import random_chunk
from test_paint_gpu import bits_equal, oracle_stones

pytestmark = pytest.mark.gpu

MODES = {"exact": api.RL_SUM_EXACT, "lanes": api.RL_SUM_LANES, "serial": api.RL_SUM_EXACT_SERIAL}
STONE_KEYS = ("alpha", "beta", "ls_alpha", "ls_beta", "bsnp_begin", "bsnp_end")


def last_live_target(N):
    """(PaintLane::init) virtual lane 0 holds donors 0 .. len - 1 in registers 0 .. len - 1, and no lane is longer: the
    target k = len_0 - 1 has its own slot in the last register that any lane uses"""
    waves = 2 if N > 5120 else 1
    q, rem = divmod(N, 64 * waves)
    return q + (1 if rem else 0) - 1


def target_ranges(N):
    if N < 3000:
        return [(0, N)]
    kl = last_live_target(N)  # (39 .. 79: its range may overlap the first)
    return [(0, 48), (kl, kl + 48), (N // 2 - 24, N // 2 + 24), (N - 48, N)]


def check_fit(ch, want, modes=("exact", "lanes", "serial")):
    """want = (S, waves, tail, live).  Paint with the fitted variant and with the loose one; the first against the
    oracle at a handful of targets, the second against the first at every painted target."""
    N = ch.N
    assert api.tile_fit(N) == want
    kl = last_live_target(N)
    oracle = {}
    for k0, k1 in target_ranges(N):
        ctx = api.Context()
        ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
        assert (ctx.tile, ctx.waves) == want[:2]
        if (k0, k1) != (0, N):
            ctx.set_target_range(k0, k1)
        targets = sorted(k for k in set([0, 1, kl, N // 2, N - 2, N - 1]) if k0 <= k < k1)
        for mode in modes:
            ctx.set_paint_fit(1)
            ctx.paint(MODES[mode])
            fitted = [ctx.stones(w) for w in range(ch.W)]
            for k in targets:
                key = (k, mode == "lanes")
                if key not in oracle:
                    oracle[key] = oracle_stones(ch, k, mode == "lanes")
                bb, be, al, bt, la, lb = oracle[key]
                r = k - k0
                for w in range(ch.W):
                    st = fitted[w]
                    assert st["bsnp_begin"][r] == bb[w] and st["bsnp_end"][r] == be[w], (mode, k, w)
                    assert bits_equal(st["ls_alpha"][r], la[w]) and bits_equal(st["ls_beta"][r], lb[w]), (mode, k, w)
                    assert bits_equal(st["alpha"][r], al[w]) and bits_equal(st["beta"][r], bt[w]), (mode, k, w)
            ctx.set_paint_fit(0)
            ctx.paint(MODES[mode])
            for w in range(ch.W):
                loose = ctx.stones(w)
                for key in STONE_KEYS:
                    assert bits_equal(fitted[w][key].view(np.uint32), loose[key].view(np.uint32)), (mode, w, key)
        ctx.close()


# N, (S, waves, tail, live)
CASES = [
    (389, (8, 1, 4, 7)),      # q = 6, rem = 5, need 7: tight minus one
    (453, (8, 1, 4, 8)),      # q = 7, rem = 5, need 8: tight, partial last register
    (512, (8, 1, 4, 8)),      # q = 8, rem = 0: tight, no partial register
    (200, (8, 1, 8, 8)),      # q = 3: loose
    (901, (16, 1, 4, 15)),    # q = 14, need 15
    (965, (16, 1, 4, 16)),    # q = 15, need 16
    (1925, (32, 1, 4, 31)),   # need 31
    (3008, (48, 1, 4, 47)),   # q = 47, rem = 0: tight minus one with no partial register at all
    (5000, (80, 1, 4, 79)),   # the headline variant
    (5120, (80, 1, 4, 80)),   # q = 80, rem = 0
    (5893, (48, 2, 4, 47)),   # two waves, q = 46, rem = 5: the longer lanes lie in wave 0 only
    (6021, (48, 2, 4, 48)),   # two waves, need 48
    (10000, (80, 2, 4, 79)),  # two waves, need 79
]


@pytest.mark.parametrize("N,want", CASES)
def test_fitted_tile_matches_oracle_and_loose_variant(N, want):
    ch = random_chunk(N, 300, 0.13, seed=N, wb=[0, 90, 210, 300], special="flat_targets")
    check_fit(ch, want)


def test_wide_tail_inside_the_last_chunk():
    """q >= S - 4 with need <= S - 2 (N = 4900: q = 76, need 77): the tight tail with several tested registers"""
    ch = random_chunk(4900, 300, 0.13, seed=4900, wb=[0, 90, 210, 300], special="flat_targets")
    check_fit(ch, (80, 1, 4, 80))


def test_dense_panel_many_rescales_live_registers():
    """dense derived alleles: frequent rescaling (1e-10 / 1e10), the division loop over the LIVE registers (N = 389:
    7 of 8)"""
    ch = random_chunk(389, 400, 0.5, 5, wb=[0, 100, 250, 400])
    ch.theta = 0.001
    check_fit(ch, (8, 1, 4, 7))
