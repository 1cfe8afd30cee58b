"""The census of tests/repaint_cases.py, asserted with the CPU oracle alone: every case of
test_repaint_geometry_gpu.py reaches what its family demands, so the GPU test never fails for lack of an input.
The stones are the oracle's own Paint of the compared targets (ro_paint_stepping_stones per target)."""
import ctypes as C
import os

import numpy as np
import pytest

import repaint_cases as rc
import rlutil


def test_tiles_and_targets_of_family_a():
    """both edges of every (S, waves): q = S with rem = 0 and the first N of the next tile, 5000 and 10240"""
    seen = {}
    for case in rc.A_CASES:
        seen.setdefault(rc.tile_of(case.N), []).append(case.N)
    assert sorted(seen) == sorted(rc.INSTANCES)
    for (S, waves), Ns in seen.items():
        assert any(N == S * 64 * waves for N in Ns), (S, waves, Ns)  # q = S, rem = 0
    for N in (513, 1025, 2049, 3073, 4097, 5121, 6145, 8193):
        q, rem = divmod(N - 1, 64 * rc.tile_of(N - 1)[1])
        assert rem == 0 and rc.tile_of(N) != rc.tile_of(N - 1) and N in rc.A_SIZES
    for case in rc.A_CASES:
        N, t = case.N, case.targets()
        S, waves = rc.tile_of(N)
        q, rem = divmod(N, 64 * waves)
        kl = rc.last_live_target(N)
        assert {0, 1, N // 2, N - 2, N - 1, kl} <= set(t)
        assert kl == q + (rem > 0) - 1 and kl < q + (rem > 0)  # lane 0, its last register
        if waves == 2:
            k1 = rc.wave1_target(N)
            assert k1 in t and k1 == sum(q + (l < rem) for l in range(64))  # donor 0 of virtual lane 64
        ch = case.chunk()
        assert not (ch.seq[:, 0] == ord("1")).any() and (ch.seq[:, N - 1] == ord("1")).all()  # flat, saturated


@pytest.mark.parametrize("tile", rc.INSTANCES, ids=lambda t: "S%d-w%d" % t)
@pytest.mark.parametrize("order", ["exact", "lanes"])  # (the serial order is the exact order's oracle)
def test_rescale_census_of_every_tile(tile, order):
    """families A and C together reach every cell of the rescale census at every (S, waves) in both oracle orders"""
    cells = rc.tile_cells(tile, order)
    missing = [c for c in rc.RESCALE_CELLS if c not in cells]
    assert not missing, (tile, order, missing)
    # ... and family C's own case of the tile reaches the two cells a random panel leaves out
    own = [c for c in rc.C_CASES if rc.tile_of(c.N) == tile and c.N != 130]
    assert len(own) == 1
    assert ("two-in-a-block",) in rc.case_cells(own[0], order)


def open_windows(tmp_path, case):
    o = rlutil.oracle()
    ch = case.chunk()
    d = ch.ro()
    assert o.ro_paint_chunk(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), ch.W, str(tmp_path).encode(), 4, 0, None,
                            None) == 0
    for w in range(ch.W):
        pf = os.path.join(str(tmp_path), "relate_%d.bin" % w)
        ow = o.ro_window_open(C.byref(d), pf.encode(), int(ch.wb[w]), 4)
        assert ow
        yield ch, w, ow, d
        o.ro_window_free(C.c_void_p(ow))


def test_degenerate_windows_census(tmp_path):
    """family B: targets with 2, 3 and 4 rows in a window are there, D - 1 takes every residue mod 6, and the oracle
    gives finite matrices on all of it (N = 2 and 3 included)"""
    o = rlutil.oracle()
    Ds = {}
    for case in rc.B_CASES:
        sub = tmp_path / case.name
        sub.mkdir()
        for ch, w, ow, d in open_windows(sub, case):
            for n in range(ch.N):
                Ds.setdefault(o.ro_window_rows(C.c_void_p(ow), n), []).append((case.name, w, n))
            M = np.full((ch.N, ch.N), np.nan, np.float32)
            o.ro_window_matrix(C.c_void_p(ow), int(ch.wb[w]), M.ctypes.data_as(C.c_void_p))
            assert np.isfinite(M).all(), (case.name, w)
    assert {2, 3, 4} <= set(Ds), sorted(Ds)
    assert set((D - 1) % rc.CK for D in Ds) == set(range(rc.CK)), sorted(Ds)
    # K1's dense-window chunk as the issue counted it: D = 2 / 3 / 4 / 5 in 391 / 212 / 52 / 5 (target, window)s
    dense = {D: sum(1 for x in v if x[0] == "B-dense-33") for D, v in Ds.items()}
    assert [dense.get(D, 0) for D in (2, 3, 4, 5)] == [391, 212, 52, 5], dense
    assert any(x[0] == "B-flat-20" for x in Ds[2])


def test_matrix_ways_census(tmp_path):
    """family E: the cases whose matrices are compared at every SNP (N <= 130 of families B and C) have direct rows,
    interpolated rows on both sides of ls_prev <= ls_next, and a row whose minimum one target alone shares with the
    diagonal"""
    o = rlutil.oracle()
    tot = np.zeros(3, np.int64)
    single = 0
    for case in rc.B_CASES + [c for c in rc.C_CASES if c.N <= 130]:
        sub = tmp_path / case.name
        sub.mkdir()
        for ch, w, ow, d in open_windows(sub, case):
            def logs(n):
                D = o.ro_window_rows(C.c_void_p(ow), n)
                return np.ctypeslib.as_array(C.cast(o.ro_window_log(C.c_void_p(ow), n), C.POINTER(C.c_float)), (D,))
            ways = np.array(rc.matrix_ways(ch, w, None, logs))
            tot += ways
            if case.N >= 3:
                M = np.zeros((ch.N, ch.N), np.float32)
                o.ro_window_matrix(C.c_void_p(ow), int(ch.wb[w]), M.ctypes.data_as(C.c_void_p))
                single += int(((M == 0).sum(axis=1) == 2).sum())
    assert (tot > 0).all(), tot
    assert single > 0
