"""CopyingMatrix without a GPU: the host twin of the device's reduction (rl_copying_rows_host) and the row weights
(rl_copying_weights_host) against the numpy restatement of the definition on the oracle's posterior rows
(copying_cases.py), bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import copying_cases as cc
import rlutil
from relate_amd import api

_cache = {}


def oracle_case(tmp_path_factory, N, L, budget, seed, flat=None):
    """chunk + the oracle's windows, painted once per shape; flat = (s0, s1): rpos constant over those SNPs"""
    key = (N, L, budget, seed, flat)
    if key not in _cache:
        o = rlutil.oracle()
        ch = rlutil.synth_chunk(N, L, seed=seed, budget=budget)
        if flat:
            ch.rpos[flat[0]:flat[1]] = ch.rpos[flat[0]]
        d = ch.ro()
        pdir = str(tmp_path_factory.mktemp("copying_%d" % N))
        assert o.ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), ch.W, pdir.encode(), 4, 0, None, None) == 0
        _cache[key] = (ch, [cc.OracleWindow(ch, os.path.join(pdir, "relate_%d.bin" % w), w) for w in range(ch.W)])
    return _cache[key]


SHAPES = [(8, 600, 3000, 3), (65, 1200, 30000, 2), (300, 500, 400000, 6)]


@pytest.mark.parametrize("N,L,budget,seed", SHAPES)
def test_host_twin_equals_the_restatement(tmp_path_factory, N, L, budget, seed):
    ch, wins = oracle_case(tmp_path_factory, N, L, budget, seed)
    assert ch.W >= 2
    want = np.zeros((N, N), np.float64)
    got = np.zeros((N, N), np.float64)
    for ow in wins:  # the windows rising, every target's rows rising
        cc.add_window(ow, want)
        for n in range(N):
            rows, site, wt = cc.window_inputs(ow, n)
            wt_lib = api.copying_weights_host(site, ch.rpos, ch.wb[ow.w], ch.wb[ow.w + 1])
            assert np.array_equal(cc.bits(wt_lib), cc.bits(wt)), (ow.w, n)
            api.copying_rows_host(rows, wt_lib, got[n])
    assert np.array_equal(cc.bits(got), cc.bits(want))
    assert not np.diag(got).any()
    # every recipient copies each SNP from somebody: rows sum to the SNP count (bound ~ (L + N) 2^-53 <= 3e-13 here)
    rel = np.abs(np.array([sum(float(v) for v in got[n]) for n in range(N)]) / ch.L - 1.0)
    assert rel.max() <= 1e-10, rel.max()


@pytest.mark.parametrize("N,L,budget,seed", SHAPES)
def test_weights_sum_to_the_snp_count(tmp_path_factory, N, L, budget, seed):
    ch, wins = oracle_case(tmp_path_factory, N, L, budget, seed)
    for ow in wins:
        snps = int(ch.wb[ow.w + 1] - ch.wb[ow.w])
        for n in range(N):
            _, site, _ = cc.window_inputs(ow, n)
            wt = api.copying_weights_host(site, ch.rpos, ch.wb[ow.w], ch.wb[ow.w + 1])
            total = 0.0
            for v in wt:
                total += float(v)
            assert abs(total / snps - 1.0) <= 1e-10, (ow.w, n, total, snps)


def test_zero_recombination_stretch_takes_the_half_half_rule(tmp_path_factory):
    N, L = 65, 1200
    ch, wins = oracle_case(tmp_path_factory, N, L, 30000, 2, flat=(100, 400))
    hit = 0
    for ow in wins:
        for n in range(N):
            rows, site, wt = cc.window_inputs(ow, n)
            for p in range(len(site) - 1):  # a SNP of the window strictly between two rows at one genetic position
                a, b = site[p], site[p + 1]
                if ch.rpos[a] == ch.rpos[b] and max(a + 1, ch.wb[ow.w]) < min(b, ch.wb[ow.w + 1]):
                    hit += 1
            wt_lib = api.copying_weights_host(site, ch.rpos, ch.wb[ow.w], ch.wb[ow.w + 1])
            assert np.array_equal(cc.bits(wt_lib), cc.bits(wt)), (ow.w, n)
            assert np.isfinite(wt_lib).all()
            got = api.copying_rows_host(rows, wt_lib)
            want = cc.reduce_rows(rows, wt, np.zeros(N, np.float64))
            assert np.array_equal(cc.bits(got), cc.bits(want)), (ow.w, n)
    assert hit > 0


def test_half_half_rule_by_hand():
    site = [0, 4, 9]
    rpos = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 5.0])
    wt = api.copying_weights_host(site, rpos, 0, 10)
    # SNPs 0, 4, 9 on their rows; 1..3 interpolate between rows 0 and 1; 5..8 lie in the flat stretch: 0.5 each side
    assert wt.tolist() == [1.0 + 0.75 + 0.5 + 0.25, 1.0 + 0.25 + 0.5 + 0.75 + 4 * 0.5, 1.0 + 4 * 0.5]


def test_zero_row_with_a_weight_is_refused():
    rows = np.zeros((3, 40), np.float32)
    rows[0, 1:] = 0.5
    rows[2, 1:] = 0.25
    with pytest.raises(api.RelateError) as e:
        api.copying_rows_host(rows, [1.0, 2.0, 1.0])
    assert "error -6" in str(e.value) and "row 1" in str(e.value)  # RL_ESTATE
    c = api.copying_rows_host(rows, [1.0, 0.0, 1.0])  # without a weight the row is never looked at
    assert abs(sum(float(v) for v in c) - 2.0) < 1e-12
    rows[1, 3] = np.inf
    with pytest.raises(api.RelateError):
        api.copying_rows_host(rows, [1.0, 2.0, 1.0])


def test_weights_refuse_a_window_the_rows_do_not_cover():
    rpos = np.arange(12, dtype=np.float64)
    with pytest.raises(api.RelateError):
        api.copying_weights_host([2, 5, 9], rpos, 0, 8)   # rows begin behind the window's first SNP
    with pytest.raises(api.RelateError):
        api.copying_weights_host([0, 3, 6], rpos, 0, 9)   # SNPs 7, 8 behind the last row
