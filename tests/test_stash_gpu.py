"""K1's exact backward pass keeps the first KS weighted terms of a step in LDS (StashTerm,
relate_amd/csrc/exact_sum.h: KS = 8, 12, 16, 24, 36, 36 of S = 8, 16, 32, 48, 64, 80, what the tile's share of the
CU's LDS holds, 36 at the most) instead of recomputing them in every pass of the sum.  A lane reads back what it wrote,
so nothing may change: stones and logscales bit for bit against the oracle (exact order), the sum bit for bit
against the sequential sum.  Each test names a way the stash can go wrong:

  * the boundary KS inside, at the end of and beyond a lane's S registers, TAIL chunks inside the stash (small S)
    and recomputed (S = 80), in the merged launch and in the backward-only one;
  * two waves per target, one stash region per wave;
  * the stash shares LDS with the staging strip of the stones: stones written between two consecutive sums;
  * the sum itself on adversarial terms through the debug hook's stashing term kind: the chains, the rerun of a
    multi-binade lane and the literal fallback all read the stash -- same paths as the lane-mask kind takes."""
import numpy as np
import pytest

from relate_amd import api
from test_edge_gpu import random_chunk
from test_exact_sum_gpu import NTH, TH, assert_bits, cases, check_terms, seam_cases, serial_sums
from test_paint_gpu import bits_equal, oracle_stones

pytestmark = pytest.mark.gpu


def check_exact(ch, tile, ranges, picks):
    """RL_SUM_EXACT stones of the targets `picks` of every range (the context paints one range of targets at a time),
    once as the merged launch and once with one launch per direction, against the oracle"""
    ref = {}
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    assert (ctx.tile, ctx.waves) == tile
    for split in (False, True):
        ctx.set_paint_split(split)
        for k0, k1 in ranges:
            ctx.set_target_range(k0, k1)
            ctx.paint(api.RL_SUM_EXACT)
            st = [ctx.stones(w) for w in range(ch.W)]
            for k in (k for k in picks if k0 <= k < k1):
                if k not in ref:
                    ref[k] = oracle_stones(ch, k, False)
                bb, be, al, bt, la, lb = ref[k]
                for w in range(ch.W):
                    what = (split, k, w)
                    assert st[w]["bsnp_begin"][k - k0] == bb[w] and st[w]["bsnp_end"][k - k0] == be[w], what
                    assert bits_equal(st[w]["ls_beta"][k - k0], lb[w]), what + ("ls_beta",)
                    assert bits_equal(st[w]["beta"][k - k0], bt[w]), what + ("beta",)
                    assert bits_equal(st[w]["ls_alpha"][k - k0], la[w]), what + ("ls_alpha",)
                    assert bits_equal(st[w]["alpha"][k - k0], al[w]), what + ("alpha",)
    ctx.close()
    assert sorted(ref) == sorted(picks)


def ends_and_middle(N, width=48):
    """three ranges of targets and the targets compared in them: the flat target 0, the saturated target N - 1 (donor
    k in the first / last lane), and the middle of the layout"""
    m = N // 2
    return ([(0, width), (m - width // 2, m + width // 2), (N - width, N)],
            [0, 1, width - 1, m - 1, m, N - 2, N - 1])


@pytest.mark.parametrize("N,S", [(500, 8), (600, 16), (2000, 32), (2100, 48), (3500, 64), (5000, 80)])
def test_backward_stones_on_both_sides_of_the_stash_boundary(N, S):
    """S = 8: every term stashed, the TAIL chunks inside the stash and the last chunk stored behind the loop;
    S = 16, 32, 48: the boundary (12, 16, 24) falls inside the row, a TAIL chunk below it at S = 16; S = 64: the
    boundary at 36; S = 80: the headline tile, TAIL registers recomputed.  A few hundred sites, four windows"""
    ch = random_chunk(N, 330, 0.13, seed=N + 3, wb=[0, 90, 170, 260, 330], special="flat_targets")
    ranges, picks = ends_and_middle(N)
    check_exact(ch, (S, 1), ranges, picks)


@pytest.mark.parametrize("N,S", [(5121, 48), (10240, 80)])
def test_two_waves_per_target_each_with_its_stash(N, S):
    ch = random_chunk(N, 240, 0.14, seed=N + 5, wb=[0, 100, 240], special="flat_targets")
    ranges, picks = ends_and_middle(N, 32)
    check_exact(ch, (S, 2), ranges, picks)


@pytest.mark.parametrize("N,S", [(600, 16), (5000, 80), (5200, 48)])
def test_stones_written_between_consecutive_sums(N, S):
    """windows of one and two SNPs on a dense panel: a target visits most sites, so a backward stone -- staged through
    the strip that the stash overlays -- is written after almost every sum and overwritten by the next step's terms"""
    L = 72
    wb = list(range(0, 24)) + list(range(24, L, 2)) + [L]
    ch = random_chunk(N, L, 0.45, seed=N + 7, wb=wb, special="flat_targets")
    m = N // 2
    check_exact(ch, (S, 2 if N > 5120 else 1), [(0, 24), (m, m + 24), (N - 24, N)], [0, 1, m, m + 5, N - 2, N - 1])


@pytest.mark.parametrize("n", [999, 2000, 2100, 3500, 5000, 5120, 5121, 8193, 10240])
def test_exact_sum_through_the_stash(n):
    """the adversarial families of test_exact_sum_gpu.py with the stashing term kind, 16 sums back to back on one
    WaveLink (the stash is rewritten before every sum): the sequential sum bit for bit, and the path counters of the
    lane-mask kind on the same input -- so the reruns and the fallbacks counted here read the stash"""
    rng = np.random.RandomState(4000 + n)
    families = [(name, x) for name, x, _ in seam_cases(n, 16, rng)] + list(cases(n, 16, rng))
    total = dict(sums=0, fallbacks=0, walked=0, reruns=0)
    for density in (0.0, 0.3):
        for name, x in families:
            assert x.shape == (16, n)
            mis = rng.rand(*x.shape) < density
            t = np.where(mis, TH, NTH) * x
            check_terms(t)
            got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, 16, mis, TH, NTH, stash=True)
            assert_bits(got, serial_sums(t), n, name, density, "stash")
            _, st_mask = api.debug_wave_sum(x, api.RL_SUM_EXACT, 16, mis, TH, NTH)
            assert st == st_mask, (n, name, density, st, st_mask)
            assert st["sums"] == 16 * (2 if n > 5120 else 1), (n, name, st)
            if name == "tiny and subnormal":
                assert st["fallbacks"] > 0, (n, name, density, st)
            for key in total:
                total[key] += st[key]
    assert total["fallbacks"] > 0 and total["walked"] > 0 and total["reruns"] > 0, total


def test_the_stashing_kind_is_exact_and_masked_only():
    lib = api.lib()
    x = np.ones((1, 8))
    with pytest.raises(api.RelateError, match="RL_DEBUG_SUM_STASH"):
        api.debug_wave_sum(x, api.RL_SUM_EXACT, stash=True)  # no mismatch array
    with pytest.raises(api.RelateError, match="RL_DEBUG_SUM_STASH"):
        api.debug_wave_sum(x, api.RL_SUM_LANES, mismatch=np.zeros((1, 8), np.uint8), stash=True)
    assert lib.rl_last_error()
