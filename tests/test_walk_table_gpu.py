"""The exact order's walk reads a tie lane's map from a table of four int16 packed by the lane itself
(relate_amd/csrc/exact_sum.h walk_table_pack / walk_table_hop; tests/test_walk_table_cpu.py holds the integer
identity).  Here the walk runs on the GPU: the sum bit for bit against the sequential sum on families made of rounding
ties, with the path counters showing that table lanes were walked and the literal fallback was not taken, and the
stones bit for bit against the oracle at the smallest shapes of each tile family.

The families are those of tests/test_exact_sum_gpu.py that walk ("ties mid-binade", "tie at the seam"), and three
built by its recipes so that the counters can be asserted exactly: its "ties" and "ties odd head" have a head of 1.0,
prefixes just above a power of two, which is the literal fallback by design and cannot be asked to take none."""
import numpy as np
import pytest

from relate_amd import api
from test_edge_gpu import random_chunk
from test_exact_sum_gpu import NTH, TH, assert_bits, check_terms, layout, seam_cases, serial_sums
from test_paint_gpu import bits_equal, oracle_stones

pytestmark = pytest.mark.gpu

SIZES = [128, 4993, 5000, 5121, 10240]
ROWS = 16  # sums back to back on one WaveLink


def tie_families(n, rng):
    """-> (name, x [ROWS][n], table lanes walked per row or None where only a lower bound of one holds)"""
    waves, start = layout(n)
    V = 64 * waves
    from_seam = {name: x for name, x, _ in seam_cases(n, ROWS, rng)}
    yield "ties mid-binade", from_seam["ties mid-binade"], None
    yield "tie at the seam", from_seam["tie at the seam"], None

    # ties and one binade crossing inside a lane's run: half-ulp multiples on a head of 1.5, and in the middle of
    # the run of the lane at a quarter of the layout one term of 0.75 (1.5 -> 2.25: both prefixes far from 2.0);
    # behind it the same terms are quarters of the new ulp, every fourth a tie
    x = rng.randint(0, 8, (ROWS, n)).astype(np.float64) * 2.0 ** -53
    x[:, 0] = 1.5
    v = V // 4
    x[:, (start(v) + start(v + 1)) // 2] = 0.75
    yield "ties and a crossing", x, None

    # ties, a term that swamps the bracket (a `constant` lane: the walk starts from its exit), then ties at the new
    # scale: quarter-ulp multiples of ulp(2^40) = 2^-12
    x = rng.randint(0, 8, (ROWS, n)).astype(np.float64) * 2.0 ** -53
    x[:, 0] = 1.5
    s = start(V // 2 + 1)
    x[:, s] = 2.0 ** 40 * 1.5
    x[:, s + 1:] = rng.randint(0, 8, (ROWS, n - s - 1)).astype(np.float64) * 2.0 ** -14
    yield "ties, a swamping jump, ties", x, None

    # Exact everywhere (integers on a head of 2^20 + 0.5: no rounding, the total stays in the binade) but for ties
    # of (0.5 | 1.5) ulp in chosen lanes: exactly those lanes are walked.  The first terms of two neighbouring lanes:
    # two walked lanes are adjacent; with two waves the pair is virtual lanes 64 and 65, so wave 1 walks its lane 0
    # (entered at wave 0's exit offset, nothing of its own wave before it) and then its lane 1.
    x = rng.randint(0, 8, (ROWS, n)).astype(np.float64)
    x[:, 0] = 2.0 ** 20 + 0.5
    ulp = 2.0 ** -32
    assert np.all(np.spacing(serial_sums(x)) == ulp)
    va = V // 2
    x[:, start(va) - 1] += rng.randint(0, 4, ROWS) * ulp  # the lane's entry residue mod 4
    for lane in (va, va + 1):
        x[:, start(lane)] = (0.5 + rng.randint(0, 2, ROWS)) * ulp
    yield "adjacent tie lanes", x, 2


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_walked_table_lanes_give_the_serial_sum(n, masked):
    rng = np.random.RandomState(7000 + n)
    waves = 2 if n > 5120 else 1
    for name, x, exact in tie_families(n, rng):
        assert x.shape == (ROWS, n)
        mis = np.zeros(x.shape, bool) if masked else None  # (weight nth = 1.0: the terms stay the ties they are)
        t = x
        check_terms(t)
        ref = serial_sums(t)
        kinds = [dict(regstash=True), dict(stash=True), dict()] if masked else [dict()]
        for kind in kinds:
            got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, ROWS, mis, TH, 1.0, **kind)
            what = (n, name, masked, kind, st)
            assert_bits(got, ref, *what)
            assert st["sums"] == ROWS * waves, what
            assert st["fallbacks"] == 0, what
            table_lanes = st["walked"] - st["reruns"]
            assert table_lanes >= 1, what
            if exact is not None:
                assert st["reruns"] == 0 and st["walked"] == exact * ROWS, what


def test_weighted_tie_families_give_the_serial_sum():
    """weights through the mask panel (th, nth as the painting has them) on the tie families: whatever the lanes
    classify as, the sum is the sequential one"""
    n = 5000
    rng = np.random.RandomState(7100)
    for name, x, _ in tie_families(n, rng):
        mis = rng.rand(*x.shape) < 0.3
        t = np.where(mis, TH, NTH) * x
        check_terms(t)
        got, st = api.debug_wave_sum(x, api.RL_SUM_EXACT, ROWS, mis, TH, NTH, regstash=True)
        assert_bits(got, serial_sums(t), n, name, st)


def painted(ctx, W):
    ctx.paint(api.RL_SUM_EXACT)
    return [ctx.stones(w) for w in range(W)]


# N, (S, waves): the smallest shapes that reach each tile family
@pytest.mark.parametrize("N,tile", [(1000, (16, 1)), (4000, (64, 1)), (5000, (80, 1)), (5121, (48, 2))])
def test_stones_against_the_oracle(N, tile):
    """the unsegmented and the segmented merged launch, targets in the first and the last lane"""
    ch = random_chunk(N, 240, 0.13, seed=N + 23, wb=[0, 100, 240], special="flat_targets")
    if N == 5000:
        assert api.tile_fit(N) == (80, 1, 4, 79)  # tight minus one
    ref = {}
    for k0, k1, picks in ((0, 32, (0, 1, 31)), (N - 32, N, (N - 32, N - 2, N - 1))):
        ctx = api.Context()
        ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
        assert (ctx.tile, ctx.waves) == tile
        ctx.set_target_range(k0, k1)
        for segs in ((1, 1), (3, 2)):
            ctx.set_paint_segments(*segs)
            st = painted(ctx, ch.W)
            assert ctx.paint_launched_segments() == segs
            for k in picks:
                if k not in ref:
                    ref[k] = oracle_stones(ch, k, False)
                bb, be, al, bt, la, lb = ref[k]
                for w in range(ch.W):
                    what = (N, segs, k, w)
                    assert st[w]["bsnp_begin"][k - k0] == bb[w] and st[w]["bsnp_end"][k - k0] == be[w], what
                    assert bits_equal(st[w]["ls_beta"][k - k0], lb[w]), what + ("ls_beta",)
                    assert bits_equal(st[w]["beta"][k - k0], bt[w]), what + ("beta",)
                    assert bits_equal(st[w]["ls_alpha"][k - k0], la[w]), what + ("ls_alpha",)
                    assert bits_equal(st[w]["alpha"][k - k0], al[w]), what + ("alpha",)
        ctx.close()
