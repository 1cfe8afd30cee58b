"""With one wave per target (n <= 5120) the exact order composes the lanes that stay in their binade without a tie --
translations of the offset -- with one integer add-scan, and walks every other lane: tie lanes, and every lane whose
run crosses a binade (relate_amd/csrc/exact_sum.h walk_enter / walk_leave / walk_head_hop;
tests/test_translation_scan_cpu.py holds the integer identity).  Here the sums run on the GPU, bit for bit against the
sequential numpy sum, on families in which lanes cross a binade: in almost every lane, next to each of the other kinds
of lane, and at the ends of the layout; and on heavy-tailed weighted terms.  The path counters show that the crossing
lanes were walked and that the literal fallback was not taken.

A lane is walked rather than sent to the fallback only where no partial sum comes near a power of two (the bracket of
2 x 16384 ulp must not straddle it), so each family first asserts in numpy that every serial prefix, lane entries and
total included, lies more than 2^17 ulp from a power of two.

Targets of two waves (n > 5120) keep the segmented scan of the lanes' maps (exact_sum.h sum_exact_fast_segmented):
their crossing lanes are not walked, and a sum with more than 20 of them takes the fallback, so the crossing families
run at the one-wave sizes only; the heavy-tailed family runs at all sizes."""
import numpy as np
import pytest

from relate_amd import api
from test_exact_sum_gpu import NTH, TH, assert_bits, check_terms, layout, serial_sums

pytestmark = pytest.mark.gpu

ONE_WAVE = [128, 4993, 5000]  # the smallest tile, and both fitted variants of the largest
SIZES = ONE_WAVE + [5121, 10240]  # ... and two waves
ROWS = 16  # sums back to back on one WaveLink


def ulps_from_a_power_of_two(v):
    """distance of v > 0 to the nearer end of its binade, in ulp of that binade"""
    m, _ = np.frexp(v)  # v = m 2^e, 0.5 <= m < 1
    return np.minimum(m - 0.5, 1.0 - m) * 2.0 ** 53


def exponent(v):
    return np.frexp(v)[1]


def assert_walkable(t):
    """the precondition of `fallbacks == 0`: no serial prefix within 2^17 ulp of a power of two"""
    pre = np.add.accumulate(t, axis=1)
    assert np.all(pre > 2.0 ** -900) and np.all(ulps_from_a_power_of_two(pre) > 2.0 ** 17)
    return pre


def crossing_lanes(t):
    """-> how many lanes of all rows enter in one binade and leave in the next one up, the lanes with an exact entry
    (virtual lanes 0 and 1) left out: each of them is a head of the walk"""
    n = t.shape[1]
    waves, start = layout(n)
    pre = assert_walkable(t)
    lanes = np.arange(2, 64 * waves)
    first = np.array([start(v) for v in lanes])
    last = np.array([start(v + 1) for v in lanes]) - 1
    return int(np.sum(exponent(pre[:, last]) - exponent(pre[:, first - 1]) == 1))


def families(n, rng):
    """-> (name, x [ROWS][n], counter that must be reached at least once per row or None)"""
    waves, start = layout(n)
    assert waves == 1
    V = 64
    mid = lambda v: (start(v) + start(v + 1)) // 2

    # A crossing in almost every lane: the serial prefix at the start of lane l is about 1.5 * 2^(l - 30), each lane's
    # increment spread evenly over its terms, every term with random low bits.  More than 20 single crossings in one
    # sum (a scan that composes crossing lanes has to cap their number; the walk does not).
    x = np.empty((ROWS, n))
    for v in range(V):
        p0 = 0.0 if v == 0 else 1.5 * 2.0 ** (v - 30)
        p1 = 1.5 * 2.0 ** (v + 1 - 30)
        k = start(v + 1) - start(v)
        x[:, start(v):start(v + 1)] = (p1 - p0) / k * (1.0 + 1e-3 * (rng.rand(ROWS, k) - 0.5))
    assert crossing_lanes(x) == ROWS * (V - 2)
    yield "a crossing in almost every lane", x, None

    # The other families: random terms below 1 on a head of 1.5 * 2^20 (no lane crosses by itself, none has a tie),
    # and single terms placed from the serial prefix in front of them, in the order of their positions.
    def base():
        x = rng.rand(ROWS, n)
        x[:, 0] = 1.5 * 2.0 ** 20
        return x

    def cross(x, v):
        """a term in the middle of lane v that takes the prefix to about 1.5 times the next power of two"""
        pos = max(mid(v), 1)
        pre = serial_sums(x[:, :pos])
        x[:, pos] = (1.5 * 2.0 ** exponent(pre) - pre) * (1.0 + 1e-3 * rng.rand(ROWS))

    def tie(x, v):
        """the first term of lane v is (0.5 | 1.5) ulp of the prefix: the lane's four runs disagree"""
        pos = start(v)
        x[:, pos] = (0.5 + rng.randint(0, 2, ROWS)) * np.spacing(serial_sums(x[:, :pos]))

    a = V // 4
    x = base()
    cross(x, a - 1)
    tie(x, a)
    cross(x, a + 1)
    yield "crossing, tie, crossing", x, None

    x = base()
    x[:, mid(a)] = 2.0 ** 40 * (1.4 + 0.2 * rng.rand(ROWS))  # swamps the bracket: a `constant` lane
    cross(x, a + 1)
    yield "a crossing behind a swamping term", x, None

    x = base()
    cross(x, a - 1)
    pos = mid(a)
    x[:, pos] = 3.0 * serial_sums(x[:, :pos]) * (1.0 + 0.01 * rng.rand(ROWS))  # two binades up, c0 != c3: a rerun
    cross(x, a + 1)
    yield "crossings around a multi-binade rerun", x, "reruns"

    x = base()
    cross(x, V - 1)
    yield "a crossing in the last lane", x, None

    x = base()
    cross(x, 2)
    yield "a crossing in lane 2", x, None


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", ONE_WAVE)
def test_crossing_lanes_are_walked(n, masked):
    rng = np.random.RandomState(8000 + n)
    for name, x, counter in families(n, rng):
        assert x.shape == (ROWS, n)
        check_terms(x)
        crossings = crossing_lanes(x)
        assert crossings >= ROWS, name
        ref = serial_sums(x)
        mis = np.zeros(x.shape, bool) if masked else None  # (weight nth = 1.0: the terms stay what they are)
        kinds = [dict(), dict(stash=True), dict(regstash=True)] if masked else [dict()]
        for kind in kinds:
            got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, ROWS, mis, TH, 1.0, **kind)
            what = (n, name, masked, kind, st, crossings)
            assert_bits(got, ref, *what)
            assert st["sums"] == ROWS, what
            assert st["fallbacks"] == 0, what
            assert st["walked"] >= crossings, what
            if counter:
                assert st[counter] >= ROWS, what


@pytest.mark.parametrize("n", SIZES)
def test_wide_dynamic_range_weighted(n):
    """heavy-tailed terms under the painting's weights: whatever the lanes classify as, the sum is the sequential one"""
    rng = np.random.RandomState(8100 + n)
    x = np.exp(6.0 * rng.randn(256, n))
    mis = rng.rand(*x.shape) < 0.3
    t = np.where(mis, TH, NTH) * x
    check_terms(t)
    ref = serial_sums(t)
    for kind in (dict(), dict(stash=True), dict(regstash=True)):
        got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, ROWS, mis, TH, NTH, **kind)
        assert_bits(got, ref, n, kind, st)
    got, st = api.debug_wave_sum(t, api.RL_SUM_EXACT, ROWS)
    assert_bits(got, ref, n, "unmasked", st)
