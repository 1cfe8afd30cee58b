"""The rule that fits K1's register tile to N (rl_tile_fit, relate_amd/csrc/launch.h tile_fit), on the host: for every
N the tile and waves are choose_S / target_waves', `live` leaves out exactly the register no lane reaches, and the
tight tail is chosen exactly where the validity masks fit into the last backward chunk."""
import pytest

from relate_amd import api

TILES = (8, 16, 32, 48, 64, 80)


def layout(N):
    """launch.h: target_waves, make_layout, choose_S -> (waves, q, rem, need, S)"""
    waves = 2 if N > 80 * 64 else 1
    q, rem = divmod(N, 64 * waves)
    need = q + (1 if rem else 0)
    return waves, q, rem, need, min(s for s in TILES if s >= need)


def test_rule_over_every_N():
    for N in range(2, 10241):
        waves, q, rem, need, S = layout(N)
        s, w, tail, live = api.tile_fit(N)
        assert (s, w) == (S, waves), N
        assert live == need or live == S, N
        assert (live == S - 1) == (need == S - 1), N
        assert (tail == 4) == (q >= S - 4), N
        if tail != 4:  # the loose variant: the tile list's tail, every register kept
            assert (tail, live) == (8 if S <= 16 else 16, S), N


@pytest.mark.parametrize("N,want", [(1000, (16, 4, 16)), (2000, (32, 4, 32)), (5000, (80, 4, 79)),
                                    (10000, (80, 4, 79))])
def test_baseline_configurations(N, want):
    """the N of BASELINE.json's configurations #2, #4, #3 and #5: all of them run a fitted variant"""
    s, w, tail, live = api.tile_fit(N)
    assert (s, tail, live) == want
    assert w == (2 if N > 5120 else 1)


def test_out_of_range_is_reported():
    for N in (-1, 0, 1, 10241):
        with pytest.raises(api.RelateError):
            api.tile_fit(N)
