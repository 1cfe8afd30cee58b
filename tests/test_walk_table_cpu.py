"""The exact order's hop over a tie lane (relate_amd/csrc/exact_sum.h): the walk reads delta' = (delta >> sh) + U_h,
h = (p0 + delta) & 3, from a table of four int16 that the lane packed during classification (walk_table_pack,
walk_table_hop; U_h = A_h - (B_h >> sh)).  It must be the literal form A_h + ((delta - B_h) >> sh)
(walk_hop_reference) for every entry offset the bracket admits -- integer equality, on the host, through
rl_debug_walk_table."""
import itertools

import numpy as np
import pytest

from relate_amd import api

G4 = 16384  # exact_sum.h WALK_G4: half-width of the bracket
LO, HI = -G4 - 8, G4 + 8
T_VALUES = (-32768, -300, -1, 0, 1, 300, 32767)  # both ends of int16 among them


def entry_offsets(p0):
    """B_h: the entry offsets of the four runs' starts"""
    return np.array([-p0 - G4, 1 - p0, 2 - p0, 3 - p0 + G4], dtype=np.int64)


def literal_hop(A, p0, sh, delta):
    """the literal form in numpy (int64), independent of the library"""
    h = (p0 + delta) & 3
    return A[h] + ((delta - entry_offsets(p0)[h]) >> sh)


@pytest.mark.parametrize("sh", [0, 1])
@pytest.mark.parametrize("p0", [0, 1, 2, 3])
def test_table_hop_is_the_literal_hop(p0, sh):
    """every delta in [-G4 - 8, G4 + 8], every table set A_h = (B_h >> sh) + t_h with t_h drawn independently per h
    (7^4 sets: a tie lane has unequal t_h)"""
    B = entry_offsets(p0)
    delta = np.arange(LO, HI + 1, dtype=np.int64)
    sets = 0
    for n, t in enumerate(itertools.product(T_VALUES, repeat=4)):
        A = (B >> sh) + np.array(t, dtype=np.int64)
        ok, tab, ref = api.walk_table(A, p0, sh, LO, HI)
        assert ok, (p0, sh, t)
        assert np.array_equal(tab, ref), (p0, sh, t, delta[np.nonzero(tab != ref)[0][:4]])
        if n % 97 == 0 or len(set(t)) == 4:  # the library's literal form against numpy's, on a part of the sets
            assert np.array_equal(ref, literal_hop(A, p0, sh, delta)), (p0, sh, t)
        sets += 1
    assert sets == 7 ** 4


@pytest.mark.parametrize("sh", [0, 1])
@pytest.mark.parametrize("p0", [0, 1, 2, 3])
def test_an_entry_beyond_int16_is_not_packable(p0, sh):
    B = entry_offsets(p0)
    for h in range(4):
        for bad in (32768, -32769, 1 << 20, -(1 << 20)):
            t = np.array([5, -7, 300, 0], dtype=np.int64)
            t[h] = bad
            ok, _, ref = api.walk_table((B >> sh) + t, p0, sh, -8, 8)
            assert not ok, (p0, sh, h, bad)
            # (the literal form is still evaluated)
            assert np.array_equal(ref, literal_hop((B >> sh) + t, p0, sh, np.arange(-8, 9, dtype=np.int64)))
        for edge in (32767, -32768):  # the last values that fit
            t = np.zeros(4, dtype=np.int64)
            t[h] = edge
            ok, tab, ref = api.walk_table((B >> sh) + t, p0, sh, -8, 8)
            assert ok and np.array_equal(tab, ref), (p0, sh, h, edge)


def test_bad_arguments():
    A = np.zeros(4, np.int32)
    for args in ((A, 4, 0, 0, 1), (A, -1, 0, 0, 1), (A, 0, 2, 0, 1), (A, 0, 0, 2, 1)):
        with pytest.raises(api.RelateError, match="rl_debug_walk_table"):
            api.walk_table(*args)
