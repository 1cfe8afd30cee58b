"""K1's exact backward pass holds the LAST R weighted terms of a step in registers from the update loop to the end of
the exact sum (StashTerm::xr, relate_amd/csrc/exact_sum.h reg_stash_terms: R = 28 at S = 64, 12 at S = 80, 0 at the
smaller tiles), next to the first KS in LDS; only terms KS .. S-R-1 are still recomputed by each pass of the sum.  A
register holds what the update loop put there, so nothing may change: stones and logscales bit for bit against the
oracle (exact order), the sum bit for bit against the sequential sum.  Each test names a way registers can go wrong:

  * the held chunks are the TAIL chunks of every fit variant (launch.h tile_fit: loose, tight, tight with a wide tail,
    tight minus one, where the last held chunk has three terms), in the merged launch and in one launch per direction,
    the target's own slot in the first lane, the last lane and the middle;
  * two waves per target, each wave with registers of its own;
  * stones written between two consecutive sums (the staging code runs while nothing is held, and must leave the next
    step's held terms alone);
  * the sum itself on adversarial terms through the debug hook's three-way term kind: the chains, the rerun of a
    multi-binade lane and the literal fallback all read the held terms -- same paths as the lane-mask kind takes."""
import numpy as np
import pytest

from relate_amd import api
from test_edge_gpu import random_chunk
from test_exact_sum_gpu import NTH, TH, assert_bits, cases, check_terms, seam_cases, serial_sums
from test_stash_gpu import check_exact, ends_and_middle

gpu = pytest.mark.gpu

TILES = (8, 16, 32, 48, 64, 80)
HELD = (64, 80)  # the tiles with R > 0 (test_term_split_of_every_tile keeps this list honest)

# N, (S, waves, tail, live): every fit variant of the tiles that hold terms in registers.  S = 80 as
# tests/test_tile_fit_gpu.py has them; S = 64, which that file reaches with two waves only, by the same rule
# (q = N // 64, need = q + (rem > 0)).
VARIANTS = [
    (3500, (64, 1, 16, 64)),  # q = 54 < 60: loose
    (3845, (64, 1, 4, 64)),   # q = 60, need 61: tight, wide tail
    (3973, (64, 1, 4, 63)),   # q = 62, need 63: tight minus one, the held tail chunk has three terms
    (4037, (64, 1, 4, 64)),   # q = 63, need 64: tight, partial last register
    (4200, (80, 1, 16, 80)),  # q = 65 < 76: loose
    (4900, (80, 1, 4, 80)),   # q = 76, need 77: tight, wide tail
    (5000, (80, 1, 4, 79)),   # the headline variant: tight minus one
    (5120, (80, 1, 4, 80)),   # q = 80, rem = 0: tight
]


def test_term_split_of_every_tile():
    """host only: R is a whole number of chunks and the held chunks lie behind the stashed ones"""
    for S in TILES:
        ks, r = api.term_split(S)
        assert ks % 4 == 0 and r % 4 == 0 and 0 <= r and 0 < ks and ks + r <= S, (S, ks, r)
        assert (r > 0) == (S in HELD), (S, r)
    with pytest.raises(api.RelateError, match="rl_debug_term_split"):
        api.term_split(24)


@gpu
@pytest.mark.parametrize("N,want", VARIANTS)
def test_backward_stones_with_held_tail_chunks(N, want):
    assert api.tile_fit(N) == want
    ch = random_chunk(N, 300, 0.13, seed=N + 11, wb=[0, 80, 160, 240, 300], special="flat_targets")
    ranges, picks = ends_and_middle(N)
    check_exact(ch, want[:2], ranges, picks)


@gpu
@pytest.mark.parametrize("N,S", [(8192, 64), (8193, 80), (10240, 80)])
def test_two_waves_per_target_each_with_its_registers(N, S):
    """both sides of the switch between the two tiles that hold terms (N = 8192: q = 64 of 128 lanes, the last shape
    of S = 64; one donor more needs 65 registers in virtual lane 0 and runs S = 80), and the largest N"""
    ch = random_chunk(N, 240, 0.14, seed=N + 13, wb=[0, 100, 240], special="flat_targets")
    ranges, picks = ends_and_middle(N, 32)
    check_exact(ch, (S, 2), ranges, picks)


@gpu
@pytest.mark.parametrize("N,S", [(5000, 80), (8000, 64)])
def test_stones_written_between_consecutive_sums(N, S):
    """windows of one and two SNPs on a dense panel: a backward stone is written after almost every sum"""
    L = 72
    wb = list(range(0, 24)) + list(range(24, L, 2)) + [L]
    ch = random_chunk(N, L, 0.45, seed=N + 17, wb=wb, special="flat_targets")
    m = N // 2
    check_exact(ch, (S, 2 if N > 5120 else 1), [(0, 24), (m, m + 24), (N - 24, N)], [0, 1, m, m + 5, N - 2, N - 1])


@gpu
@pytest.mark.parametrize("n", [3500, 5000, 5120, 5121, 10240])
def test_exact_sum_through_the_held_terms(n):
    """the adversarial families of test_exact_sum_gpu.py with the three-way term kind, 16 sums back to back on one
    WaveLink: the sequential sum bit for bit, and the path counters of the lane-mask kind on the same input -- so the
    reruns and the fallbacks counted here read the held terms.  (n = 5121: S = 48, R = 0, the kind is the stashing
    one there)"""
    rng = np.random.RandomState(5000 + n)
    families = [(name, x) for name, x, _ in seam_cases(n, 16, rng)] + list(cases(n, 16, rng))
    total = dict(sums=0, fallbacks=0, walked=0, reruns=0)
    for density in (0.0, 0.3):
        for name, x in families:
            assert x.shape == (16, n)
            mis = rng.rand(*x.shape) < density
            t = np.where(mis, TH, NTH) * x
            check_terms(t)
            got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, 16, mis, TH, NTH, regstash=True)
            assert_bits(got, serial_sums(t), n, name, density, "regstash")
            _, st_mask = api.debug_wave_sum(x, api.RL_SUM_EXACT, 16, mis, TH, NTH)
            assert st == st_mask, (n, name, density, st, st_mask)
            assert st["sums"] == 16 * (2 if n > 5120 else 1), (n, name, st)
            if name == "tiny and subnormal":
                assert st["fallbacks"] > 0, (n, name, density, st)
            for key in total:
                total[key] += st[key]
    assert total["fallbacks"] > 0 and total["walked"] > 0 and total["reruns"] > 0, total


def test_the_three_way_kind_is_exact_and_masked_only():
    x = np.ones((1, 8))
    with pytest.raises(api.RelateError, match="RL_DEBUG_SUM_REGSTASH"):
        api.debug_wave_sum(x, api.RL_SUM_EXACT, regstash=True)  # no mismatch array
    with pytest.raises(api.RelateError, match="RL_DEBUG_SUM_REGSTASH"):
        api.debug_wave_sum(x, api.RL_SUM_LANES, mismatch=np.zeros((1, 8), np.uint8), regstash=True)
    with pytest.raises(api.RelateError, match="exclude each other"):
        api.debug_wave_sum(x, api.RL_SUM_EXACT, mismatch=np.zeros((1, 8), np.uint8), stash=True, regstash=True)
