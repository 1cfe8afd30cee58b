"""The exact order composes its tie-free, crossing-free lanes -- pure translations delta -> delta + C -- with one
integer add-scan over the wave and walks the other lanes, the heads, from it (relate_amd/csrc/exact_sum.h walk_enter,
walk_leave, walk_head_hop).  The exit offset so computed must be the one obtained lane by lane in the literal form
(walk_hop_reference) -- integer equality, on the host, through rl_debug_walk_lanes."""
import numpy as np
import pytest

from relate_amd import api

TR, TB, CO = api.WALK_TRANSLATION, api.WALK_TABLE, api.WALK_CONSTANT
G4 = 16384  # exact_sum.h WALK_G4


def translation(c):
    return (TR, c, 0, 0, 0, 0, 0)


def table(u, p0, sh):
    return (TB, u[0], u[1], u[2], u[3], p0, sh)


def constant(a0):
    return (CO, a0, 0, 0, 0, 0, 0)


def random_table(rng, crossing=None):
    sh = rng.randint(0, 2) if crossing is None else int(crossing)
    return table(rng.randint(-300, 301, 4), rng.randint(0, 4), sh)


def literal(records, delta):
    """numpy-free restatement (Python integers reduced to int32), independent of the library"""
    def i32(v):
        return (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    for kind, u0, u1, u2, u3, p0, sh in records:
        if kind == TR:
            delta = i32(delta + u0)
        elif kind == CO:
            delta = u0
        else:
            h = (p0 + delta) & 3
            B = (-p0 - G4, 1 - p0, 2 - p0, 3 - p0 + G4)[h]
            A = (u0, u1, u2, u3)[h] + (B >> sh)
            delta = i32(A + ((delta - B) >> sh))
    return delta


def check(records, delta=0):
    records = [tuple(int(v) for v in r) for r in records]
    lit, scan = api.walk_lanes(np.array(records, np.int32), delta)
    assert lit == literal(records, delta), (records, delta)
    assert scan == lit, (records, delta, scan, lit)
    return scan


@pytest.mark.parametrize("seed", range(8))
def test_seeded_lane_mixes(seed):
    rng = np.random.RandomState(9000 + seed)
    for _ in range(300):
        lanes = rng.randint(1, 65)
        p_head, p_const = rng.choice([0.0, 0.05, 0.3, 0.9]), rng.choice([0.0, 0.02])
        recs = []
        for _l in range(lanes):
            r = rng.rand()
            if r < p_const:
                recs.append(constant(rng.randint(-3000, 3001)))
            elif r < p_const + p_head:
                recs.append(random_table(rng))
            else:
                recs.append(translation(rng.randint(-200, 201)))
        check(recs, rng.randint(-G4, G4 + 1))


def test_corner_cases():
    rng = np.random.RandomState(9100)
    tr = lambda: translation(rng.randint(-200, 201))
    for rep in range(50):
        # a head at lane 0 with a non-zero entry offset (wave 1's lane 0), both kinds of shift
        for sh in (0, 1):
            for delta in (-777, -1, 1, 2, 3, 4095, G4):
                check([random_table(rng, sh)] + [tr() for _ in range(63)], delta)
        # a head at lane 63
        check([tr() for _ in range(63)] + [random_table(rng)], rng.randint(-50, 51))
        # adjacent heads, at the front, in the middle and at the end
        for at in (0, 1, 30, 62):
            recs = [tr() for _ in range(64)]
            recs[at], recs[at + 1] = random_table(rng), random_table(rng)
            check(recs, rng.randint(-50, 51))
        # no head at all; all 64 lanes heads
        check([tr() for _ in range(64)], rng.randint(-50, 51))
        check([random_table(rng) for _ in range(64)], rng.randint(-50, 51))
        # a constant lane followed directly by a head (and translations on either side); constant in lanes 0 and 63
        for at in (0, 1, 17, 62):
            recs = [tr() for _ in range(64)]
            recs[max(at - 1, 0)] = random_table(rng)  # (a head in front of it, which the walk skips)
            recs[at], recs[at + 1] = constant(rng.randint(-3000, 3001)), random_table(rng)
            check(recs, rng.randint(-50, 51))
        check([tr() for _ in range(63)] + [constant(rng.randint(-3000, 3001))], 5)
        # two constant lanes: the walk starts behind the last
        recs = [tr() for _ in range(64)]
        recs[5], recs[40], recs[41] = constant(11), constant(-12), random_table(rng)
        check(recs, 7)
    # a single lane of each kind
    for rec in (translation(-9), table((3, -4, 5, 6), 2, 1), constant(-77)):
        check([rec], 13)


def test_running_sum_that_wraps_int32():
    """only differences of the scan are used: C values whose running sum leaves int32 and comes back give the same
    offsets at the heads"""
    rng = np.random.RandomState(9200)
    # three steps of 1.5 * 2^30 up and three down: the running sum goes 1.5, 3 -> -1, 4.5 -> 0.5 (times 2^30) and back,
    # never within 2^29 of the ends of int32, where the literal form's own delta - B_h would leave int32
    big = 3 * 2 ** 29
    for rep in range(100):
        recs = [translation(rng.randint(-200, 201)) for _ in range(64)]
        up = rng.choice(np.arange(0, 30), 3, replace=False)
        down = rng.choice(np.arange(34, 64), 3, replace=False)
        sign = 1 if rep % 2 else -1
        for l in up:
            recs[l] = translation(sign * (big + rng.randint(-200, 201)))
        # heads while the running sum is wrapped, in between: their entry offsets are what they are (modulo 2^32)
        recs[31], recs[32] = random_table(rng), random_table(rng)
        for l in down:
            recs[l] = translation(-sign * (big + rng.randint(-200, 201)))
        recs[rng.randint(45, 64)] = random_table(rng)
        check(recs, rng.randint(-50, 51))
    # the scan passes the end of int32 and comes back in front of each head
    recs = []
    for _ in range(16):
        recs += [translation(2 ** 31 - 1), translation(-(2 ** 31 - 1) + 3), random_table(rng), translation(5)]
    assert abs(check(recs, 0)) < 2 ** 16


def test_bad_arguments():
    good = np.array([translation(1)], np.int32)
    for recs in (np.array([(3, 0, 0, 0, 0, 0, 0)]), np.array([(-1, 0, 0, 0, 0, 0, 0)]),
                 np.array([table((1, 2, 3, 4), 4, 0)]), np.array([table((1, 2, 3, 4), 0, 2)]),
                 np.array([table((1, 2, 3, 40000), 0, 1)]), np.array([constant(-40000)]),
                 np.repeat(good, 65, axis=0), np.zeros((0, 7))):
        with pytest.raises(api.RelateError, match="rl_debug_walk_lanes"):
            api.walk_lanes(recs)
