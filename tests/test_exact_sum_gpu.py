"""RL_SUM_EXACT (relate_amd/csrc/exact_sum.h) must return the reference's
serial left-to-right double sum bit for bit -- on painting-like data and on
adversarial inputs: rounding ties, terms spanning many binades, jumps of
several binades, totals and prefixes next to powers of two, zeros.

The hook (rl_debug_wave_sum_ex) runs the sums at the kernels' geometry: one
wave per array up to n = 5120, above it a workgroup of two waves that meet in
LDS (WaveLink), several arrays back to back on one WaveLink, and the terms
either as registers (RegTerm, forward passes) or as (mismatch ? th : nth) * x
under EXEC masks (MaskTerm, backward passes).  The references are plain numpy
in float64.  Every term is non-negative and finite: the precondition of
exact_sum.h (check_terms)."""
import ctypes as C

import numpy as np
import pytest

import bigtile
from relate_amd import api

pytestmark = pytest.mark.gpu

MODES = ((api.RL_SUM_EXACT, "exact"), (api.RL_SUM_EXACT_SERIAL, "serial"), (api.RL_SUM_LANES, "lanes"))
ONE_WAVE = [64, 999, 5000, 5120]
# both sides of every register-tile switch of the two-wave range (S = 48 | 64 | 80), and config #5's N
TWO_WAVES = [5121, 6144, 6145, 8192, 8193, 10000, 10240]
TH, NTH = 0.001, 0.999


def gpu_sums(x, mode):
    x = np.ascontiguousarray(x, dtype=np.float64)
    batch, n = x.shape
    out = np.empty(batch, np.float64)
    rc = api.lib().rl_debug_wave_sum(x.ctypes.data_as(C.c_void_p), n, batch, mode, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, api.lib().rl_last_error()
    return out


def serial_sums(x):
    return np.add.accumulate(np.asarray(x, np.float64), axis=1)[:, -1]  # sequential IEEE adds


def layout(n):
    """-> (waves, start): the kernels' runs, virtual lane v holds terms start(v) .. start(v + 1) - 1"""
    waves = 2 if n > 80 * 64 else 1  # launch.h target_waves
    q, rem = divmod(n, 64 * waves)
    return waves, lambda v: v * q + min(v, rem)


def lanes_sums(t):
    """RL_SUM_LANES: each lane's serial sum of its run, an xor-butterfly over the 64 lanes of a wave (the value of
    wave_sum_butterfly's DPP steps: IEEE addition is commutative), read in lane 63; two waves add t0 + t1"""
    batch, n = t.shape
    waves, start = layout(n)
    lane = np.zeros((batch, 64 * waves))
    for v in range(64 * waves):
        if start(v + 1) > start(v):
            lane[:, v] = np.add.accumulate(t[:, start(v):start(v + 1)], axis=1)[:, -1]
    idx = np.arange(64)
    tot = None
    for w in range(waves):
        s = lane[:, 64 * w:64 * w + 64]
        for m in (1, 2, 4, 8, 16, 32):
            s = s + s[:, idx ^ m]
        tot = s[:, 63] if tot is None else tot + s[:, 63]
    return tot


def check_terms(t):
    assert np.all(np.isfinite(t)) and not np.any(np.signbit(t)), "exact_sum.h needs non-negative finite terms"


def assert_bits(got, ref, *what):
    bad = np.nonzero(got.view(np.uint64) != ref.view(np.uint64))[0]
    assert len(bad) == 0, what + (len(bad), bad[:3], got[bad[:3]], ref[bad[:3]])


def check(x, rows_per_group=1, mismatch=None, what=()):
    """all three modes against their references, bit for bit -> path counters of RL_SUM_EXACT"""
    t = x if mismatch is None else np.where(mismatch, TH, NTH) * x  # one IEEE multiply per term, as weighted4
    check_terms(t)
    serial, lanes = serial_sums(t), lanes_sums(t)
    stats = None
    for mode, mname in MODES:
        got, st = api.debug_wave_sum(x, mode, rows_per_group, mismatch, TH, NTH)
        assert_bits(got, lanes if mode == api.RL_SUM_LANES else serial, *(what + (mname,)))
        if mode == api.RL_SUM_EXACT:
            stats = st
    return stats


def cases(n, batch, rng):
    u = rng.rand(batch, n)
    yield "uniform", u
    yield "lognormal wide", np.exp(rng.randn(batch, n) * 8.0)
    yield "painting-like", np.where(rng.rand(batch, n) < 0.02, rng.rand(batch, n), 1e-7 * rng.rand(batch, n))
    # many exact ties: small integers times a power of two against a big head
    t = rng.randint(0, 8, (batch, n)).astype(np.float64) * 2.0 ** -53
    t[:, 0] = 1.0
    yield "ties", t
    t2 = rng.randint(1, 4, (batch, n)).astype(np.float64) * 2.0 ** -52
    t2[:, 0] = 1.0 + 2.0 ** -52
    yield "ties odd head", t2
    j = 1e-12 * rng.rand(batch, n)
    for b in range(batch):
        j[b, rng.randint(0, n)] = 10.0 ** rng.randint(-3, 6)
        j[b, rng.randint(0, n)] = 10.0 ** rng.randint(-3, 6)
    yield "big jumps", j
    p = rng.rand(batch, n)
    p *= (2.0 ** rng.randint(-3, 4, (batch, 1))) / p.sum(axis=1, keepdims=True)  # totals ~ powers of two
    yield "total near power of two", p
    z = rng.rand(batch, n)
    z[:, : n // 3] = 0.0
    yield "leading zeros", z
    yield "all equal", np.full((batch, n), 0.1)
    yield "powers of two", 2.0 ** rng.randint(-30, 30, (batch, n)).astype(np.float64)


def seam_cases(n, batch, rng):
    """families aimed at the seam: two waves, the first term of wave 1 (virtual lane 64); one wave, lane 32.  "Before"
    and "after" are the terms on either side of it (wave 0 / wave 1).  -> (name, x, counter the family must reach)"""
    waves, start = layout(n)
    V = 64 * waves
    s = start(V // 2)
    col = lambda v: v[:, None]
    u = rng.rand(batch, n)

    x = u.copy()
    x[:, :s] = 0.0
    yield "before zero", x, None  # (two waves: the bracket of wave 0's total +0.0 has no lower end, a fallback)
    x = u.copy()
    x[:, s:] = 0.0
    yield "after zero", x, None
    # a two-binade jump (sh >= 2) that the 2^15-ulp bracket does not collapse (c0 != c3): a multi-binade rerun,
    # at the seam lane and at the last term of the lane before it
    x = u.copy()
    x[:, s] = 3.0 * serial_sums(x[:, :s]) * (1.0 + 0.01 * rng.rand(batch))
    yield "jump at the seam", x, "reruns"
    x = u.copy()
    x[:, s - 1] = 3.0 * serial_sums(x[:, :s - 1]) * (1.0 + 0.01 * rng.rand(batch))
    yield "jump at the end of the lane before", x, "reruns"
    # ties throughout (the head 1.5, not 1.0: prefixes just above a power of two would take the fallback), then a
    # term that swamps the bracket in mid-wave 1: a "constant" lane restarts the walk
    x = rng.randint(0, 8, (batch, n)).astype(np.float64) * 2.0 ** -53
    x[:, 0] = 1.5
    yield "ties mid-binade", x.copy(), "walked"
    x[:, start(3 * V // 4)] = 2.0 ** 40 * (1.0 + rng.rand(batch))
    yield "swamping jump after ties", x, "walked"
    # a rounding tie in the seam lane's run: half-integer prefixes before it (exact, and never a power of two), its
    # low bits set to j ulp (the lane's entry residue mod 4), then (0.5 | 1.5) ulp: the four runs of the lane
    # disagree; random terms after it, so the lanes behind the seam lane compose to a non-trivial map
    x = u.copy()
    x[:, :s] = rng.randint(0, 8, (batch, s))
    x[:, 0] += 0.5
    x[:, s - 1] += 1.0
    ulp = np.spacing(serial_sums(x[:, :s]))
    x[:, s - 1] += rng.randint(0, 4, batch) * ulp
    t0 = serial_sums(x[:, :s])
    assert np.array_equal(t0, x[:, :s].sum(axis=1)) and np.all(np.spacing(t0) == ulp)  # exact, same binade
    x[:, s] = (0.5 + rng.randint(0, 2, batch)) * ulp
    yield "tie at the seam", x, "walked"
    # a prefix within a few ulp of a power of two (the bracket of 2 x 16384 ulp straddles it): the serial fallback.
    # Two waves: at lane 32 only wave 0 flags it, at the seam both do (wave 0's total is wave 1's entry), at the
    # end (the full total, not wave 0's) only wave 1 does -- and both waves must take the linked fallback
    for name, m in (("prefix near 2^k before the seam", V // 4), ("prefix near 2^k at the seam", V // 2),
                    ("total near 2^k, not the prefix at the seam", V)):
        x = u.copy()
        sm = start(m)
        x[:, :sm] /= col(serial_sums(x[:, :sm]))
        if sm < n:
            x[:, sm:] *= col(0.4 / x[:, sm:].sum(axis=1))
        assert np.all(np.abs(serial_sums(x[:, :sm]) - 1.0) < 2.0 ** -40)
        if sm < n:
            assert np.all(np.abs(serial_sums(x) - 1.4) < 0.01)
        yield name, x * col(2.0 ** rng.randint(-40, 40, batch)), "fallbacks"
    # exponent fields <= 64 (below 2^-959), subnormals among them: entry_ok fails, the serial fallback
    x = u * 2.0 ** -1000
    sub = rng.rand(batch, n) < 0.3
    x[sub] = rng.randint(0, 2 ** 20, sub.sum()) * 2.0 ** -1074
    yield "tiny and subnormal", x, "fallbacks"


def assert_path(stats, counter, what):
    if counter:
        assert stats[counter] > 0, (what, counter, stats)


@pytest.mark.parametrize("n", [5, 63, 64, 200, 999, 3100, 4999, 5120])
def test_exact_sum_is_the_serial_sum(n):
    rng = np.random.RandomState(n)
    batch = 256 if n <= 1000 else 64
    for name, x in cases(n, batch, rng):
        ref = serial_sums(x)
        for mode, mname in ((api.RL_SUM_EXACT, "exact"), (api.RL_SUM_EXACT_SERIAL, "serial")):
            got = gpu_sums(x, mode)
            bad = np.nonzero(got.view(np.uint64) != ref.view(np.uint64))[0]
            assert len(bad) == 0, (n, name, mname, len(bad), got[bad[:3]], ref[bad[:3]])
        assert_bits(gpu_sums(x, api.RL_SUM_LANES), lanes_sums(x), n, name, "lanes")


@pytest.mark.parametrize("n", ONE_WAVE + TWO_WAVES)
def test_exact_sum_at_the_seam(n):
    """the seam families (and, at two waves, the ten families above), one sum per workgroup; each family reaches the
    path it is named for"""
    rng = np.random.RandomState(1000 + n)
    paths = {}
    if n > 5120:
        for name, x in cases(n, 64, rng):
            paths[name] = st = check(x, what=(n, name))
            if name == "painting-like":
                assert st["fallbacks"] == 0, (n, name, st)
    for name, x, counter in seam_cases(n, 32, rng):
        paths[name] = st = check(x, what=(n, name))
        assert_path(st, counter, (n, name))
    bigtile.record("exact_sum_paths/n=%d" % n, paths)


@pytest.mark.parametrize("n", ONE_WAVE + TWO_WAVES)
def test_exact_sum_masked_terms(n):
    """MaskTerm: terms (mismatch ? th : nth) * x recomputed under EXEC masks, at mismatch densities 0 .. 1"""
    rng = np.random.RandomState(2000 + n)
    families = [(name, x) for name, x, _ in seam_cases(n, 16, rng)]
    families += [(name, x[:16]) for name, x in cases(n, 16, rng)]
    paths = {}
    for density in (0.0, 0.02, 0.5, 1.0):
        for name, x in families:
            mis = rng.rand(*x.shape) < density
            st = check(x, mismatch=mis, what=(n, name, density))
            paths["%s, density %g" % (name, density)] = st
            if name == "tiny and subnormal":
                assert st["fallbacks"] > 0, (n, name, density, st)
    bigtile.record("exact_sum_paths_masked/n=%d" % n, paths)


@pytest.mark.parametrize("n", [999, 5120, 5121, 8193, 10240])
@pytest.mark.parametrize("masked", [False, True])
def test_exact_sum_many_rows_per_workgroup(n, masked):
    """16 sums back to back in one workgroup, a seeded mix of rows from fast-path and fallback families: the WaveLink
    slots (result, delta, bad) and its phase are reused across both paths"""
    rng = np.random.RandomState(3000 + n)
    rows = [x for _, x, _ in seam_cases(n, 8, rng)] + [x[:8] for _, x in cases(n, 8, rng)]
    x = np.concatenate(rows)
    x = x[rng.permutation(len(x))[: len(x) // 16 * 16]]
    mis = rng.rand(*x.shape) < 0.3 if masked else None
    st = check(x, rows_per_group=16, mismatch=mis, what=(n, masked))
    assert st["fallbacks"] > 0 and st["sums"] == x.shape[0] * (2 if n > 5120 else 1), st
    if not masked:
        assert st["walked"] > 0 and st["reruns"] > 0, st
    bigtile.record("exact_sum_paths_grouped/n=%d%s" % (n, " masked" if masked else ""), st)
