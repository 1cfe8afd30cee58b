"""Paint of a window range (rl_set_window_range) against the fixtures of the unmodified reference.

A section reads its own window's stepping stones alone (DistanceMeasure::GetTopologyWithRepaint,
anc_builder.cpp:49-78), so a context told a range [w_first, w_last] keeps those windows' stones only and ends each pass
at its last stone.  Whatever it keeps must be what a Paint of the whole chunk keeps for those windows:

  * config #2 (full_c2.npz: md5 of every paint file of the reference's `--mode Paint`), four ranges, `exact` mode:
    the paint files written from a range-painted context byte for byte, windows outside the range refused, the steps
    and the stone bytes of rl_paint_account against their closed forms;
  * config #3 (c3_ends.npz / c3_full.npz): windows 0, 133 and 266 each painted alone -- the one-wave tile of 80
    registers at full length from both ends of the chunk;
  * `lanes` and `lanes32`: a range paint against the SAME mode's paint of the whole chunk, bit for bit (two runs of one
    code with different ranges: the modes are tolerance modes against the reference by design, no tolerance is added);
  * with rl_set_target_range, two waves per target (N > 5120): 192 targets of config #5, window 0 (c5_first.npz);
  * the fused stage on config #2's pinned sections with rl_stage_opts.paint_windows = 1 and = 0."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import rlutil
from bigtile import md5
from relate_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def synth_bits(z):
    """the seeded panel of a fixture, bit-packed, and the reference's windows (asserted to be the fixture's)"""
    N, L, W, seed = [int(x) for x in z["meta"]]
    lib = api.lib()
    rw = (N + 31) // 32
    bits = np.zeros((L, rw), dtype=np.uint32)
    bp = np.zeros(L, dtype=np.int32)
    r = np.zeros(L)
    rpos = np.zeros(L + 1)
    assert lib.rl_synth_panel(N, L, C.c_uint64(seed), 100, 1, None, bits.ctypes.data_as(C.c_void_p), rw,
                              bp.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                              rpos.ctypes.data_as(C.c_void_p)) == 0
    budget = float(z["mem"][0]) * 1e9 / 4.0 - (2.0 * N * N + 3.0 * N)
    wb = np.zeros(L + 2, dtype=np.int32)
    assert lib.rl_synth_windows_bits(N, L, bits.ctypes.data_as(C.c_void_p), rw, C.c_double(budget),
                                     wb.ctypes.data_as(C.c_void_p), 499) == W
    wb = wb[:W + 1].copy()
    assert np.array_equal(wb, z["wb"])
    return (N, L, W), bits, bp, r, rpos, wb


def stone_tables(N, L, bits, wb):
    """the plan's stone tables from the panel (fast_painting.cpp:41-157): a target visits SNP 0, the SNPs 1 .. L-2 at
    which it is derived and SNP L-1 -- D sites; its stone of window w's begin boundary is written at visited index
    ia[w] = (sites visited before wb[w]) - 1 (0 for w = 0), that of its end boundary at ie[w] = sites visited before
    wb[w+1] (D - 1 for the last window).  -> D [N], ia [W][N], ie [W][N]"""
    W = len(wb) - 1
    der = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :N]
    before = np.zeros((W + 1, N), dtype=np.int64)  # sites visited before wb[w], 1 <= w <= W-1
    acc = np.zeros(N, dtype=np.int64)
    for w in range(1, W):
        lo, hi = max(1, int(wb[w - 1])), min(int(wb[w]), L - 1)
        acc = acc + der[lo:hi].sum(axis=0, dtype=np.int64)
        before[w] = acc + 1  # SNP 0
    D = 2 + der[1:L - 1].sum(axis=0, dtype=np.int64)
    ia = np.vstack([np.zeros((1, N), np.int64), before[1:W] - 1])
    ie = np.vstack([before[1:W], (D - 1)[None, :]])
    return D, ia, ie


def closed_form(D, ia, ie, a, b, k0=0, k1=None):
    """(forward steps, backward steps) of a Paint of windows a .. b: every step of both passes for the whole chunk;
    else the forward loop runs visited indices 1 .. ia[b], the backward loop D-2 down to ie[a]"""
    k1 = len(D) if k1 is None else k1
    W = ia.shape[0]
    if a == 0 and b == W - 1:
        return int((D[k0:k1] - 1).sum()), int((D[k0:k1] - 1).sum())
    return int(ia[b, k0:k1].sum()), int((D[k0:k1] - 1 - ie[a, k0:k1]).sum())


def refused(ctx, w, a, b, tmp_path):
    """every entry point that takes a window refuses one outside the painted range, naming the range"""
    calls = (lambda: ctx.write_paint_file(w, str(tmp_path / "outside.bin")), lambda: ctx.paint_record(w, 0),
             lambda: ctx.stones(w), lambda: ctx.open_window(w, None, None))
    for call in calls:
        with pytest.raises(api.RelateError) as e:
            call()
        assert "[%d, %d]" % (a, b) in str(e.value) and "window %d" % w in str(e.value), str(e.value)
    assert not os.path.exists(str(tmp_path / "outside.bin"))


# ------------------------------------------------------------------------------------------------ config #2
@pytest.fixture(scope="module")
def c2():
    z = np.load(os.path.join(GOLD, "full_c2.npz"))
    dims, bits, bp, r, rpos, wb = synth_bits(z)
    N, L, W = dims
    ctx = api.Context()
    ctx.set_chunk_bits(N, bits, r, rpos, wb)
    ctx.prepare()
    yield z, ctx, dims, stone_tables(N, L, bits, wb), (bits, bp, r, rpos, wb)
    ctx.close()


def test_bad_ranges_are_refused_and_the_default_is_the_whole_chunk(c2):
    z, ctx, (N, L, W), _, _ = c2
    assert ctx.window_range() == (0, W - 1)
    for a, b in ((-1, 0), (0, W), (3, 2), (W, W)):
        with pytest.raises(api.RelateError) as e:
            ctx.set_window_range(a, b)
        assert "error -1" in str(e.value) and "%d windows" % W in str(e.value), str(e.value)  # RL_EINVAL
    assert ctx.window_range() == (0, W - 1)


@pytest.mark.parametrize("which", ["first", "last", "interior", "span"])
def test_range_paint_writes_the_references_paint_files(c2, tmp_path, which):
    z, ctx, (N, L, W), (D, ia, ie), _ = c2
    assert W >= 7
    a, b = {"first": (0, 0), "last": (W - 1, W - 1), "interior": (W // 2, W // 2), "span": (2, 4)}[which]
    ctx.set_window_range(a, b)
    assert ctx.window_range() == (a, b)
    with pytest.raises(api.RelateError):  # a new range: what was painted before is gone
        ctx.paint_record(a, 0)
    ms = ctx.paint(api.RL_SUM_EXACT)
    fwd, bwd, nbytes = ctx.paint_account()
    print("C2 windows %d-%d: %.1f ms, %d forward + %d backward steps, %d bytes of stones" % (a, b, ms, fwd, bwd, nbytes))
    assert (fwd, bwd) == closed_form(D, ia, ie, a, b)
    assert nbytes == 2 * (b - a + 1) * N * N * 4
    for w in range(a, b + 1):
        fn = str(tmp_path / ("relate_%d.bin" % w))
        ctx.write_paint_file(w, fn)
        assert os.path.getsize(fn) == int(z["paint_size"][w]), "window %d" % w
        assert np.array_equal(md5(open(fn, "rb").read()), z["paint_md5"][w]), "window %d" % w
    for w in (a - 1, b + 1, 0, W - 1):
        if 0 <= w < W and not a <= w <= b:
            refused(ctx, w, a, b, tmp_path)
    with pytest.raises(api.RelateError) as e:  # every window's file: not from a range
        ctx.write_paint_files(str(tmp_path / "all"))
    assert "[%d, %d]" % (a, b) in str(e.value)
    assert not os.listdir(str(tmp_path / "all"))


def test_the_default_range_is_the_paint_of_the_whole_chunk(c2, tmp_path):
    """back from a range to all windows on the same context (the plan is not made again): every file, every step"""
    z, ctx, (N, L, W), (D, ia, ie), _ = c2
    ctx.set_window_range(1, 1)
    ctx.paint(api.RL_SUM_EXACT)
    ctx.set_window_range(0, W - 1)
    ctx.paint(api.RL_SUM_EXACT)
    total = int((D - 1).sum())
    assert total == ctx.total_sites() - N
    assert ctx.paint_account() == (total, total, 2 * W * N * N * 4)
    out = str(tmp_path / "paint")
    ctx.write_paint_files(out)
    bad = [w for w in range(W) if not np.array_equal(md5(open(os.path.join(out, "relate_%d.bin" % w), "rb").read()),
                                                     z["paint_md5"][w])]
    assert not bad, "paint files of windows %s differ from the reference's" % bad


def md5_file(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return np.frombuffer(h.digest(), dtype=np.uint8)


@pytest.mark.parametrize("paint_windows", [1, 0])
def test_fused_stage_with_and_without_the_range_writes_the_references_sections(c2, tmp_path, paint_windows):
    """rl_stage_paint_build_topology_ex for each pinned section alone: Paint of that window (1) or of every window (0)"""
    z, ctx, (N, L, W), _, (bits, bp, r, rpos, wb) = c2
    d = str(tmp_path / "out")
    os.makedirs(d)
    seq = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :N]
    seq = np.ascontiguousarray(seq + ord("0"), dtype=np.uint8)
    lib = api.lib()
    lib.rl_write_chunk_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
    wbf = np.zeros(L + 2, dtype=np.int32)
    wbf[:W + 1] = wb
    assert lib.rl_write_chunk_files(d.encode(), 0, N, L, seq.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p),
                                    r.ctypes.data_as(C.c_void_p), rpos.ctypes.data_as(C.c_void_p),
                                    wbf.ctypes.data_as(C.c_void_p), W) == 0
    del seq
    for key in z.files:  # the chunk files the reference was given
        if key.startswith("in_md5/"):
            assert np.array_equal(md5_file(os.path.join(d, key[7:])), z[key]), key
    for s in (int(x) for x in z["sections"]):
        api.stage_build_topology_ex(d, 0, s, s, api.stage_opts(paint_windows=paint_windows), fused=True)
        anc = os.path.join(d, "chunk_0", "out_%d.anc" % s)
        mut = open(os.path.join(d, "chunk_0", "out_%d.mut" % s), "rb").read()
        _, trees = rlutil.parse_anc(anc)
        assert [t[0] for t in trees] == list(z["s%d/tree_pos" % s]), "tree positions of section %d" % s
        for t, (tr, want) in enumerate(zip(trees, z["s%d/tree_parent_md5" % s])):
            assert np.array_equal(md5(tr[1].astype("<i4").tobytes()), want), "section %d, tree %d" % (s, t)
        assert mut == z["s%d/mut" % s].tobytes(), "section %d: .mut" % s
        assert os.path.getsize(anc) == int(z["s%d/anc_size" % s][0])
        assert np.array_equal(md5_file(anc), z["s%d/anc_md5" % s]), "section %d: .anc" % s


# ------------------------------------------------------------------------------------------------ config #3
@pytest.fixture(scope="module")
def c3():
    z = np.load(os.path.join(GOLD, "c3_full.npz"))
    ends = np.load(os.path.join(GOLD, "c3_ends.npz"))
    assert [int(x) for x in ends["meta"]] == [int(x) for x in z["meta"]] and np.array_equal(ends["wb"], z["wb"])
    (N, L, W), bits, bp, r, rpos, wb = synth_bits(z)
    ctx = api.Context()
    ctx.set_chunk_bits(N, bits, r, rpos, wb)
    ctx.prepare()
    assert (ctx.N, ctx.L, ctx.W, ctx.tile, ctx.waves) == (5000, 500000, 267, 80, 1)
    yield z, ends, ctx
    ctx.close()


@pytest.mark.parametrize("w", [0, 133, 266])
def test_one_window_of_config_3_painted_alone_is_the_references(c3, tmp_path, w):
    z, ends, ctx = c3
    N, W = ctx.N, ctx.W
    ctx.set_window_range(w, w)
    ms = ctx.paint(api.RL_SUM_EXACT)
    fwd, bwd, nbytes = ctx.paint_account()
    print("C3 window %d alone: %.1f ms, %d forward + %d backward steps of %d, %d bytes of stones"
          % (w, ms, fwd, bwd, ctx.total_sites() - N, nbytes))
    assert nbytes == 2 * N * N * 4
    fn = str(tmp_path / "relate_w.bin")
    ctx.write_paint_file(w, fn)
    if w in (0, W - 1):  # c3_ends.npz: the reference's complete paint file of the boundary windows
        assert w in [int(x) for x in ends["sections"]]
        assert os.path.getsize(fn) == int(ends["s%d/paint_size" % w][0])
        assert np.array_equal(md5_file(fn), ends["s%d/paint_md5" % w])
    else:  # c3_full.npz: the records of 16 pinned targets in every window, and this window's complete file
        assert w == int(z["pin_window"][0])
        for ti, k in enumerate(int(x) for x in z["targets"]):
            rec = ctx.paint_record(w, k)
            assert len(rec) == int(z["record_len"][ti, w]), k
            assert np.array_equal(md5(rec), z["record_md5"][ti, w]), "record of target %d" % k
        assert os.path.getsize(fn) == int(z["w/paint_size"][0])
        assert np.array_equal(md5_file(fn), z["w/paint_md5"])
    other = 0 if w else 1
    with pytest.raises(api.RelateError) as e:
        ctx.paint_record(other, 0)
    assert "[%d, %d]" % (w, w) in str(e.value)


# ------------------------------------------------------------------------------------------ lanes and lanes32
@pytest.mark.parametrize("mode", [api.RL_SUM_LANES, api.RL_SUM_LANES32])
def test_range_paint_in_the_lanes_modes_is_the_same_modes_full_paint(mode):
    ch = rlutil.synth_chunk(300, 6000, seed=11, budget=120000)
    W = ch.W
    assert W >= 6
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(mode)
    full = [ctx.stones(w) for w in range(W)]
    # (windows of a dozen SNPs: many targets are derived nowhere in a window, so neighbouring stones share a visited index)
    for a, b in ((0, 0), (W - 1, W - 1), (W // 2, W // 2), (1, 3), (W // 3, W // 3 + 40), (0, W - 1)):
        ctx.set_window_range(a, b)
        ctx.paint(mode)
        for w in range(a, b + 1):
            got = ctx.stones(w)
            for key in ("alpha", "beta", "ls_alpha", "ls_beta"):
                assert np.array_equal(got[key].view(np.uint32), full[w][key].view(np.uint32)), (a, b, w, key)
            assert np.array_equal(got["bsnp_begin"], full[w]["bsnp_begin"])
            assert np.array_equal(got["bsnp_end"], full[w]["bsnp_end"])
    ctx.close()


# ------------------------------------------------------------ with a target range, two waves per target (N > 5120)
def test_range_and_target_range_together_at_two_waves():
    z = np.load(os.path.join(GOLD, "c5_first.npz"))
    (N, L, W), bits, bp, r, rpos, wb = synth_bits(z)
    k0 = 5120
    ctx = api.Context()
    ctx.set_chunk_bits(N, bits, r, rpos, wb)
    ctx.set_target_range(k0, k0 + 192)
    ctx.set_window_range(0, 0)
    ctx.prepare()
    ms = ctx.paint(api.RL_SUM_EXACT)
    assert (ctx.N, ctx.L, ctx.W, ctx.waves) == (N, L, W, 2)
    fwd, bwd, nbytes = ctx.paint_account()
    print("C5, 192 targets, window 0 alone: %.1f ms, %d forward + %d backward steps, %d bytes" % (ms, fwd, bwd, nbytes))
    assert fwd == 0 and nbytes == 2 * 192 * N * 4  # window 0 begins at the first SNP: no forward step feeds its stone
    bad = []
    for k in range(k0, k0 + 192):
        rec = ctx.paint_record(0, k)
        if len(rec) != int(z["s0/record_len"][k]) or hashlib.md5(rec).digest() != z["s0/record_md5"][k].tobytes():
            bad.append(k)
    with pytest.raises(api.RelateError):
        ctx.paint_record(1, k0)
    ctx.close()
    assert not bad, "records of window 0 differ from the reference's for targets %s" % bad[:8]
