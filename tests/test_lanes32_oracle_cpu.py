"""RO_SUM_LANES32 -- the oracle's restatement of the packed-FP32 stepping-stone kernels (oracle/relate_oracle.c
paint_target_lanes32; relate_amd/csrc/paint32_kernels.hip) -- checked on the CPU, before any kernel is held to it
(tests/test_lanes32_gpu.py):

  * against the FP64 oracle in the `lanes` order: same boundaries, zeros in the same places, and an error that stays at
    a few float ulps whatever the number of steps.  MEASURED below is what the order gave on these cases; the asserted
    bounds are four times the maximum over the cases, rounded up to one digit -- a margin of 4 and no more, because the
    cases are a sample of panels and the error does not grow with the number of steps.  FP32_STATE is the plausibility
    check: the same figures of the oracle built with -DRO_FP32_STATE (the state rounded to float after every update,
    every sum in double), which lacks the kernel's float partial sums, its float constants and its reciprocal.
  * against a second restatement, MODEL below: numpy arrays of shape (register, lane) as the kernel holds the state,
    slots past a run included, with the fused multiply-add done exactly.  It shares no code with the C; the two agree
    bit for bit at the layouts' edges: empty runs (N < 64), N = 64, 65, 129, the target in the last live register,
    the target at the first donor of the second wave's runs.
  * ro_paint_chunk in the new order: the same files on 1 and 4 threads, which decode to the stones of
    ro_paint_stepping_stones."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import rlutil
from rlutil import RO_SUM_LANES, RO_SUM_LANES32
from test_edge_gpu import random_chunk
from test_paint_gpu import bits_equal, oracle_stones
from test_tile_fit_gpu import last_live_target

# ---- error against the FP64 oracle ---------------------------------------------------------------------------------
# (error of a stone relative to its largest entry, error per non-zero entry relative to that entry, log scale absolute;
#  the maximum over targets 0, 1, N/2, N-1, both passes, all windows)
CHUNKS = {
    "long_700": lambda: random_chunk(700, 6000, 0.12, seed=77, wb=[0, 1500, 4000, 6000]),
    "tile_5000": lambda: random_chunk(5000, 420, 0.13, seed=5000, wb=[0, 130, 300, 420], special="flat_targets"),
    "two_waves_10240": lambda: random_chunk(10240, 90, 0.15, seed=10240, wb=[0, 40, 90], special="flat_targets"),
    "dense_389": lambda: random_chunk(389, 400, 0.5, seed=5, wb=[0, 100, 250, 400]),
    "synth_300": lambda: rlutil.synth_chunk(300, 2000, seed=5, budget=400000),
}
#                    per stone max, per entry, log scale
MEASURED = {
    "long_700":        (6.43e-6, 1.85e-5, 6.10e-5),
    "tile_5000":       (1.79e-6, 1.71e-5, 6.10e-5),
    "two_waves_10240": (4.27e-6, 4.47e-6, 0.0),
    "dense_389":       (1.12e-6, 2.21e-6, 7.63e-6),
    "synth_300":       (2.22e-6, 2.37e-6, 7.63e-6),
}
FP32_STATE = {
    "long_700":        (2.2e-7, 2.3e-7, 1.2e-4),
    "tile_5000":       (3.6e-7, 4.1e-7, 0.0),
    "two_waves_10240": (1.2e-7, 2.1e-7, 0.0),
    "dense_389":       (2.1e-7, 3.1e-7, 0.0),
    "synth_300":       (4.7e-7, 5.3e-7, 7.6e-6),
}
# The order's stone figures are 5 to 80 times the float state's.  One of the kernel's extra roundings does it: the
# backward sum's float chains.  The lane's weighted sum is ntheta * sum_all + (theta - ntheta) * sum_mis, a difference:
# with a share m of the lane's beta on donors that mismatch at the site it comes to (ntheta - (ntheta - theta) m)
# sum_all, and the float rounding of the two chains (a few 2^-24 of sum_all each, not common to both) is magnified by
# 1 / (ntheta - (ntheta - theta) m) -- 1 at m = 0, 1 / theta = 1000 at m = 1.  The sum is the next step's b1, added to
# every entry.  With the two chains kept in double and nothing else changed the figures fall to the float state's
# (6.43e-6 -> 2.2e-7, 1.85e-5 -> 3.0e-7 on long_700; 4.27e-6 -> 1.2e-7 on two_waves_10240; 1.71e-5 -> 5.1e-7 on
# tile_5000); the forward chains in double, the division in place of the reciprocal and double constants each leave
# them where they are ("Packed-FP32 painting").
BOUND = (3e-5, 8e-5, 3e-4)  # 4 x the column maxima of MEASURED (6.43e-6, 1.85e-5, 6.10e-5), rounded up to one digit
FLOOR = (2e-4, None, 1e-3)  # what tests/test_lanes32_gpu.py::compare accepts against the `lanes` kernel


def error_figures(ch):
    N = ch.N
    worst = [0.0, 0.0, 0.0]
    for k in sorted(set([0, 1, N // 2, N - 1])):
        bb, be, al, bt, la, lb = oracle_stones(ch, k, RO_SUM_LANES)
        bb32, be32, al32, bt32, la32, lb32 = oracle_stones(ch, k, RO_SUM_LANES32)
        assert np.array_equal(bb, bb32) and np.array_equal(be, be32), k
        for x64, x32 in ((al, al32), (bt, bt32)):
            assert np.isfinite(x32).all()
            assert np.array_equal(x64 == 0, x32 == 0), k
            d = np.abs(x32.astype(np.float64) - x64)
            worst[0] = max(worst[0], float((d.max(axis=1) / np.abs(x64).max(axis=1)).max()))
            nz = x64 != 0
            worst[1] = max(worst[1], float((d[nz] / np.abs(x64[nz])).max()))
        for l64, l32 in ((la, la32), (lb, lb32)):
            worst[2] = max(worst[2], float(np.abs(l32.astype(np.float64) - l64).max()))
    return tuple(worst)


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_error_against_fp64_lanes(name):
    got = error_figures(CHUNKS[name]())
    print("lanes32 against FP64 `lanes`, %s: stone max %.2e, entry %.2e, log scale %.2e" % ((name,) + got))
    assert got[0] <= FLOOR[0] and got[2] <= FLOOR[2], got
    for g, b in zip(got, BOUND):
        assert g <= b, (got, BOUND)


def test_bounds_are_four_times_the_measured_maxima():
    for col in range(3):
        m = max(v[col] for v in MEASURED.values())
        assert 4 * m <= BOUND[col] < 4 * m + 10 ** math.floor(math.log10(4 * m)), (col, m, BOUND[col])
        assert FLOOR[col] is None or BOUND[col] < FLOOR[col]


# ---- the second restatement ----------------------------------------------------------------------------------------
F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """RN32(a * b + c) of float32 arrays: the product is exact in double, the sum is rounded to odd (the error of the
    double addition is exact: TwoSum), and a round-to-odd double rounds to the float a single rounding gives"""
    p = a.astype(F64) * F64(b)
    c = np.broadcast_to(F64(c), p.shape)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    other = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    odd = (s.view(np.int64) & 1) == 1
    return np.where((e != 0) & ~odd, other, s).astype(F32)


def butterfly(lane):
    nl = lane.shape[0]
    m = 1
    while m < nl:
        lane = lane + lane[np.arange(nl) ^ m]
        m <<= 1
    return float(lane[0])


def model_stones(ch, k):
    """paint32_forward / paint32_backward on arrays [register][lane]"""
    o = rlutil.oracle()
    N, L, W = ch.N, ch.L, ch.W
    d = ch.ro()
    site = np.zeros(L + 1, np.int32)
    rp = np.zeros(L + 2, F64)
    nxt = np.zeros(L + 1, F64)
    bb = np.zeros(W, np.int32)
    be = np.zeros(W, np.int32)
    D = o.ro_plan_target(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), W, k, site.ctypes.data_as(C.c_void_p),
                         rp.ctypes.data_as(C.c_void_p), nxt.ctypes.data_as(C.c_void_p), bb.ctypes.data_as(C.c_void_p),
                         be.ctypes.data_as(C.c_void_p))
    theta = ch.theta
    ntheta = 1.0 - theta
    Nm1 = N - 1.0
    prior_theta = theta / Nm1 - ntheta / Nm1
    prior_ntheta = ntheta / Nm1
    K1d = (theta / (1.0 - theta) - 1.0) + 1.0
    K1, init0, init1 = F32(K1d), F32(prior_ntheta), F32(prior_theta + prior_ntheta)
    inv_theta, inv_ntheta = 1.0 / theta, 1.0 / ntheta
    cf = [float(rp[i]) / ((1.0 - float(rp[i])) * Nm1) for i in range(D)]

    nl = 128 if N > 5120 else 64
    q, rem = divmod(N, nl)
    R = q + 2  # two registers more than any run needs: slots past a run change nothing
    lanes = np.arange(nl)
    start = lanes * q + np.minimum(lanes, rem)
    length = q + (lanes < rem)
    reg = np.arange(R)[:, None]
    valid = reg < length[None, :]
    donor = np.where(valid, start[None, :] + reg, 0)
    kslot = np.argwhere(valid & (donor == k))
    assert len(kslot) == 1
    kslot = tuple(kslot[0])
    der = ch.seq == ord("1")

    def mismatch(s):  # target derived, donor ancestral
        return valid & (der[s, k] & ~der[s][donor])

    def stone(x, self_value):
        out = np.zeros(N, F32)
        out[donor[valid]] = x[valid]
        out[k] = self_value
        return out

    def forward_sum(a):
        sa, sb = np.zeros((2, nl), F32), np.zeros((2, nl), F32)
        for i in range(R):
            t = sb if (i >> 1) & 1 else sa
            t[i & 1] = t[i & 1] + a[i]
        sa = sa + sb
        return butterfly(sa[0].astype(F64) + sa[1].astype(F64))

    al, bt = np.zeros((W, N), F32), np.zeros((W, N), F32)
    la, lb = np.zeros(W, F32), np.zeros(W, F32)
    a = np.where(mismatch(0), init1, init0).astype(F32)
    a[~valid] = 0
    a[kslot] = 0
    ssum = forward_sum(a)
    ls, wa = 0.0, 0
    while wa < W and bb[wa] == 0:
        al[wa], la[wa] = stone(a, 0.0), F32(ls)
        wa += 1
    cfac = cf[0] * ssum
    for i in range(1, D):
        c32 = F32(cfac)
        a[kslot] = -c32
        a = np.where(valid, a + c32, a)
        a = np.where(mismatch(site[i]), a * K1, a)
        ssum = forward_sum(a)
        ls += float(nxt[i - 1])
        cfac = ssum
        if cfac < 1e-10 or cfac > 1.0 / 1e-10:
            a = a * F32(1.0 / ssum)
            ls += math.log(ssum)
            cfac = 1.0
        cfac *= cf[i]
        while wa < W and bb[wa] == site[i]:
            al[wa], la[wa] = stone(a, 0.0), F32(ls)
            wa += 1
    assert wa == W

    ls = math.log(Nm1) - D * math.log(ntheta)
    b = np.where(valid, F32(1), F32(0)).astype(F32)
    b[kslot] = 0
    bsum = 0.0
    for n in range(N):
        bsum += theta if (der[L - 1, k] and not der[L - 1, n]) else ntheta
    bsum -= ntheta
    we = W - 1
    while we >= 0 and be[we] == L - 1:
        bt[we], lb[we] = stone(b, 1.0), F32(ls)
        we -= 1
    cfac = cf[D - 1] * bsum
    for j in range(D - 2, -1, -1):
        b1d = cfac * inv_ntheta
        btd = cfac * inv_theta - b1d
        b1, btK = F32(b1d), F32(btd * K1d)
        b[kslot] = -b1
        b = np.where(valid, b + b1, b)
        b = np.where(mismatch(site[j + 1]), fma32(b, K1, btK), b)
        mh = mismatch(site[j])
        sall, smis = np.zeros((2, nl), F32), np.zeros((2, nl), F32)
        for i in range(R):
            smis[i & 1] = np.where(mh[i], smis[i & 1] + b[i], smis[i & 1])
            sall[i & 1] = sall[i & 1] + b[i]
        lane_all = sall[0].astype(F64) + sall[1].astype(F64)
        lane_mis = smis[0].astype(F64) + smis[1].astype(F64)
        bsum = butterfly(ntheta * lane_all + (theta - ntheta) * lane_mis)
        ls += float(nxt[j + 1])
        cfac = bsum
        if cfac < 1e-10 or cfac > 1.0 / 1e-10:
            b = b * F32(1.0 / bsum)
            ls += float(o.ro_fast_log(C.c_float(bsum)))
            cfac = 1.0
        cfac *= cf[j]
        while we >= 0 and be[we] == site[j]:
            bt[we], lb[we] = stone(b, 0.0), F32(ls)
            we -= 1
    assert we == -1
    return bb, be, al, bt, la, lb


def check_model(ch, targets):
    for k in targets:
        got = oracle_stones(ch, k, RO_SUM_LANES32)
        want = model_stones(ch, k)
        for name, g, w in zip(("bsnp_begin", "bsnp_end", "alpha", "beta", "ls_alpha", "ls_beta"), got, want):
            assert bits_equal(g, w), (ch.N, k, name)
        assert not np.signbit(got[2][:, k]).any() and not np.signbit(got[3][:, k]).any()  # the own slot: +0.0 (1.0)


def test_fma32_is_one_rounding():
    rng = np.random.RandomState(1)
    a = rng.rand(20000).astype(F32)
    k, c = F32(0.0010010010), F32(3.3e-5)
    got = fma32(a, k, c)
    from fractions import Fraction
    for i in range(0, 20000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(k)) + Fraction(float(c))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert (int(got[i].view(np.uint32)) & 1) == 0  # a tie goes to even


@pytest.mark.parametrize("N", [8, 37, 64, 65, 129])
def test_small_layouts_match_the_model(N):
    """N < 64: runs of one donor and empty runs; N = 64: one donor a lane; 65, 129: one lane longer than the rest"""
    ch = random_chunk(N, 300, 0.2, seed=N, wb=[0, 90, 210, 300], special="flat_targets")
    check_model(ch, sorted(set([0, 1, last_live_target(N), N // 2, N - 2, N - 1])))


def test_many_rescales_match_the_model():
    ch = random_chunk(389, 400, 0.5, seed=5, wb=[0, 100, 250, 400])
    check_model(ch, [0, last_live_target(389), 388])


def test_target_in_the_last_live_register_matches_the_model():
    N = 453  # q = 7, rem = 5: register 7 is live in five lanes, the target's slot among them
    ch = random_chunk(N, 300, 0.13, seed=N, wb=[0, 90, 210, 300], special="flat_targets")
    check_model(ch, [last_live_target(N), last_live_target(N) + 1])


def test_first_donor_of_the_second_wave_matches_the_model():
    N = 5121  # 128 runs, q = 40, rem = 1: run 64 -- lane 0 of the second wave -- begins at donor 64 * 40 + 1
    ch = random_chunk(N, 90, 0.15, seed=N, wb=[0, 40, 90], special="flat_targets")
    first = 64 * 40 + 1
    check_model(ch, [last_live_target(N), first - 1, first, N - 1])


# ---- the paint files -----------------------------------------------------------------------------------------------
def test_paint_chunk_threads_and_decode(tmp_path):
    o = rlutil.oracle()
    ch = random_chunk(130, 400, 0.15, seed=130, wb=[0, 150, 400])
    N, W = ch.N, ch.W
    d = ch.ro()
    order = rlutil.RoSumOrder(RO_SUM_LANES32, 0, 0)
    dirs = []
    for threads in (1, 4):
        p = tmp_path / ("t%d" % threads)
        p.mkdir()
        assert o.ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), W, str(p).encode(), threads, 0,
                                C.byref(order), None) == 0
        dirs.append(p)
    files = [[open(os.path.join(str(p), "relate_%d.bin" % w), "rb").read() for w in range(W)] for p in dirs]
    assert files[0] == files[1]
    # ... and they are not the files of the FP64 orders
    p = tmp_path / "lanes"
    p.mkdir()
    o64 = rlutil.RoSumOrder(RO_SUM_LANES, 0, 0)
    assert o.ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), W, str(p).encode(), 2, 0, C.byref(o64),
                            None) == 0
    assert open(os.path.join(str(p), "relate_0.bin"), "rb").read() != files[0][0]

    v = np.zeros(N, np.float32)
    bsnp, ls = C.c_int(0), C.c_float(0)
    enc = (C.c_ubyte * o.ro_stone_max_bytes(N))()
    stones = [oracle_stones(ch, k, RO_SUM_LANES32) for k in range(N)]
    for w in range(W):
        buf = files[0][w]
        pos = 0
        for k in range(N):
            bb, be, al, bt, la, lb = stones[k]
            assert np.frombuffer(buf, np.int32, 2, pos).tolist() == [int(ch.wb[w]), int(ch.wb[w + 1]) - 1]
            pos += 8
            for stone, b, l in ((al[w], bb[w], la[w]), (bt[w], be[w], lb[w])):
                # the file holds the run-length form of the stone (collapsed_matrix.hpp:228-265), which merges entries
                # within 1e-3 of a run's first: the record is, byte for byte, the encoding of the stone of
                # ro_paint_stepping_stones, with its boundary and log scale, and decodes to the runs it holds
                n = o.ro_decode_stone(C.c_char_p(buf[pos:]), C.c_size_t(len(buf) - pos), N, v.ctypes.data_as(C.c_void_p),
                                      C.byref(bsnp), C.byref(ls))
                assert n > 0
                m = o.ro_encode_stone(stone.ctypes.data_as(C.c_void_p), N, int(b), C.c_float(l), enc)
                assert m == n and bytes(enc[:m]) == buf[pos:pos + n], (w, k)
                assert bsnp.value == b and bits_equal(np.float32(ls.value), np.float32(l)), (w, k)
                assert bits_equal(v, np.repeat(*_runs(buf, pos))), (w, k)
                assert bits_equal(v[:1], stone[:1]) and np.array_equal(v == 0, stone == 0), (w, k)
                pos += n
        assert pos == len(buf)


def _runs(buf, pos):
    n = int(np.frombuffer(buf, np.int32, 1, pos + 24)[0])
    return np.frombuffer(buf, np.float32, n, pos + 28), np.frombuffer(buf, np.int32, n, pos + 28 + 4 * n)
