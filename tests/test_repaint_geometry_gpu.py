"""K2 (RePaintSection) and K3 (GetMatrix) against the oracle at every geometry of their own: every (S, waves)
instantiation at both edges of its range of N, degenerate windows, rescales at every offset of a checkpoint block, part
launches with kept forward and backward states, K3's three ways.  All comparisons are equality of bits.

The inputs and their census are tests/repaint_cases.py (asserted without a GPU by test_repaint_cases_cpu.py).  The
stepping stones come from a device Paint (K1 is held separately: test_edge_gpu.py, test_tile_fit_gpu.py,
test_paint_segments_gpu.py) through the paint files, which both sides read.
"""
import contextlib
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import repaint_cases as rc
import rlutil
from relate_amd import api

pytestmark = pytest.mark.gpu

MODES = {"exact": api.RL_SUM_EXACT, "serial": api.RL_SUM_EXACT_SERIAL, "lanes": api.RL_SUM_LANES}
# one oracle run serves the device orders it is the reference of; one Paint of a case (and one set of paint files,
# gigabytes at the large N) serves both groups
GROUPS = {"reference": ("exact", "serial"), "lanes": ("lanes",)}
THREADS = 4


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(u32(a), u32(b))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@contextlib.contextmanager
def painted(case, tmp_path):
    """-> (chunk, context with the chunk painted, directory of its paint files); the files (gigabytes at the large N)
    go when the test is through"""
    ch = case.chunk()
    ctx = api.Context()
    pdir = os.path.join(str(tmp_path), "paint")
    try:
        ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
        assert (ctx.tile, ctx.waves) == rc.tile_of(case.N), case
        ctx.paint(api.RL_SUM_EXACT)
        os.makedirs(pdir, exist_ok=True)
        for w in case.compared_windows():
            ctx.write_paint_file(w, os.path.join(pdir, "relate_%d.bin" % w))
        yield ch, ctx, pdir
    finally:
        ctx.close()
        shutil.rmtree(pdir, ignore_errors=True)


class OracleWindow:
    """ro_window of some targets (None: all) in an oracle order"""

    def __init__(self, ch, pf, s0, group, targets=None):
        self.o, self.ch, self.d = rlutil.oracle(), ch, ch.ro()
        od = rc.ro_order("lanes" if group == "lanes" else "exact")
        t = None if targets is None else np.ascontiguousarray(targets, np.int32)
        self.h = self.o.ro_window_open_targets(C.byref(self.d), pf.encode(), s0, THREADS, C.byref(od),
                                               None if t is None else vp(t), 0 if t is None else len(t))
        assert self.h

    def rows(self, n):
        D = self.o.ro_window_rows(C.c_void_p(self.h), n)
        top = np.ctypeslib.as_array(C.cast(self.o.ro_window_top(C.c_void_p(self.h), n), C.POINTER(C.c_float)),
                                    (D, self.ch.N))
        ls = np.ctypeslib.as_array(C.cast(self.o.ro_window_log(C.c_void_p(self.h), n), C.POINTER(C.c_float)), (D,))
        return top, ls

    def advance(self, s):
        self.o.ro_window_advance(C.c_void_p(self.h), s)

    def matrix(self, s):
        M = np.zeros((self.ch.N, self.ch.N), np.float32)
        self.o.ro_window_matrix(C.c_void_p(self.h), s, vp(M))
        return M

    def matrix_rows(self, s, targets):
        M = np.zeros((len(targets), self.ch.N), np.float32)
        for i, n in enumerate(targets):
            assert self.o.ro_window_matrix_row(self.h, s, int(n), vp(M[i])) == 0
        return M

    def close(self):
        self.o.ro_window_free(C.c_void_p(self.h))


def check_window(ctx, ch, w, pf, group, targets, whole, snps):
    """window w in every device order of the group against one oracle window: every posterior row and logscale of
    `targets` (None: all), then the matrices at `snps` (rising; the cursors advance as BuildTopology's do): the whole
    matrix if `whole`, else the targets' rows"""
    s0 = int(ch.wb[w])
    tg = list(range(ch.N)) if targets is None else list(targets)
    ow = OracleWindow(ch, pf, s0, group, None if whole else tg)
    wins = {m: ctx.open_window(w, pf, s0, MODES[m]) for m in GROUPS[group]}
    try:
        for n in tg:
            top, ls = ow.rows(n)
            for m, win in wins.items():
                assert win.rows(n) == len(ls), (w, n, m)
                gtop, gls = win.topology(n)
                assert same(gls, ls), (w, n, m, "logscales")
                assert same(gtop, top), (w, n, m, "posterior rows", np.flatnonzero((u32(gtop) != u32(top)).any(axis=1)))
        cur = s0
        for s in snps:
            for t in range(cur + 1, s + 1):
                ow.advance(t)
                for win in wins.values():
                    win.advance(t)
            cur = s
            M = ow.matrix(s) if whole else ow.matrix_rows(s, tg)
            for m, win in wins.items():
                G = win.matrix(s)
                assert same(G if whole else G[tg], M), (w, s, m)
    finally:
        for win in wins.values():
            win.close()
        ow.close()


def five_snps(ch, w):
    s0, s1 = int(ch.wb[w]), int(ch.wb[w + 1]) - 1
    return sorted(set([s0, s0 + (s1 - s0) // 4, s0 + (s1 - s0) // 2, s0 + 3 * (s1 - s0) // 4, s1]))


def every_snp(ch, w):
    return list(range(int(ch.wb[w]), int(ch.wb[w + 1])))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("case", rc.A_CASES, ids=repr)
def test_every_instantiation_at_both_edges(tmp_path, case):
    """family A: q = S with rem = 0 and the first N of the next tile for every (S, waves), N = 5000 and the layout's
    maximum N = 10240.  Every row of the flat and the saturated target, of the last live register's, of wave 1's first,
    of 1, N // 2 and N - 2; matrices at five SNPs of both windows (whole up to N = 5121, the targets' rows above)"""
    with painted(case, tmp_path) as (ch, ctx, pdir):
        for w in range(ch.W):
            for group in sorted(GROUPS):
                check_window(ctx, ch, w, os.path.join(pdir, "relate_%d.bin" % w), group, case.targets(),
                             whole=case.N <= 5121, snps=five_snps(ch, w))


# ------------------------------------------------------------------ B (and E: the matrix at every SNP)
@pytest.mark.parametrize("case", rc.B_CASES, ids=repr)
def test_degenerate_windows(tmp_path, case):
    """family B: windows in which targets have 2, 3, 4 rows (jtop = 0, D - 1 < 6, a first block that is the last),
    N = 2 .. 9, L = 2 and 3: every target, every row, the matrix at every SNP"""
    with painted(case, tmp_path) as (ch, ctx, pdir):
        for w in range(ch.W):
            for group in sorted(GROUPS):
                check_window(ctx, ch, w, os.path.join(pdir, "relate_%d.bin" % w), group, None, whole=True,
                             snps=every_snp(ch, w))


# ------------------------------------------------------------------ C (and E at N = 130)
@pytest.mark.parametrize("case", rc.C_CASES, ids=repr)
def test_rescales_at_every_block_offset(tmp_path, case):
    """family C: a dense chunk with a run of singletons per tile.  The rows compared here and in family A reach every
    cell of the rescale census of the tile (asserted from the stones the device painted): a forward and a backward
    rescale at each of the six offsets of a checkpoint block, two rescales in one block, a rescale in the step into
    the window's last row.  N = 130: every target and the matrix at every SNP."""
    small = case.N <= 130
    cells = {group: set() for group in GROUPS}
    with painted(case, tmp_path) as (ch, ctx, pdir):
        for w in case.compared_windows():
            pf = os.path.join(pdir, "relate_%d.bin" % w)
            recs = None if small else rlutil.parse_paint_file(pf, case.N)
            for group in sorted(GROUPS):
                check_window(ctx, ch, w, pf, group, None if small else case.targets(), whole=small,
                             snps=every_snp(ch, w) if small else [])
                for k in ([] if small else case.targets()):
                    _, _, fwd, bwd = rc.oracle_repaint(ch, recs[k], k, GROUPS[group][0])
                    cells[group] |= rc.rescale_cells(fwd, bwd)
    for group in ([] if small else sorted(GROUPS)):
        for a in rc.A_CASES:  # (family A's share of the tile: from the oracle's own Paint, as the CPU census has it)
            if rc.tile_of(a.N) == rc.tile_of(case.N):
                cells[group] |= set(rc.case_cells(a, GROUPS[group][0]))
        missing = [c for c in rc.RESCALE_CELLS if c not in cells[group]]
        assert not missing, (case, group, missing)


# ------------------------------------------------------------------ D
PLACES = {}  # (tile, device order) -> what the launches of family D did, for test_part_launch_census


def probe(win, N, seen):
    """what the window's last launch did, by rl_debug_window_place over a sample of targets"""
    for n in range(0, N, max(1, N // 256)):
        p = win.place(n)
        assert 0 <= p["row_lo"] <= p["row_hi"] <= win.rows(n), (n, p)
        if p["partial"]:
            assert p["nostrip"] == 1, p  # a part launch runs the strip-less backward kernel
            seen["lo"].add(p["row_lo"] % rc.CK)
            seen["hi"].add((p["row_hi"] - 1) % rc.CK)
            seen["bstart"] += p["start_row"] >= 0
            seen["fstart"] += p["fstart_row"] > 0
        else:
            assert p["nostrip"] == 0 and p["start_row"] < 0 and p["fstart_row"] < 0, p
        seen["bsave"] += p["save_row"] >= 0
        seen["fsave"] += p["fsave_row"] >= 0


@pytest.mark.parametrize("case", rc.D_CASES, ids=repr)
def test_part_launches(tmp_path, case):
    """family D: a bounded window walked SNP by SNP beside the whole window of the same context, in every order.  After
    each of its launches (the first ten) its matrix is the whole window's, and up to N = 5120 the oracle's."""
    with painted(case, tmp_path) as (ch, ctx, pdir):
        for group in sorted(GROUPS):
            walk_parts(case, group, ch, ctx, os.path.join(pdir, "relate_0.bin"))


def walk_parts(case, group, ch, ctx, pf):
    N, s0, s1 = case.N, 0, case.L - 1
    ow = OracleWindow(ch, pf, s0, group) if N <= 5120 else None
    full = {m: ctx.open_window(0, pf, s0, MODES[m]) for m in GROUPS[group]}
    part = {m: ctx.open_window(0, pf, s0, MODES[m], max_rows=case.max_rows) for m in GROUPS[group]}
    seen = {m: dict(lo=set(), hi=set(), bstart=0, fstart=0, bsave=0, fsave=0, launches=0) for m in part}
    try:
        for m in part:
            assert full[m].place(0)["partial"] == 0 and full[m].place(0)["row_hi"] == full[m].rows(0)
            for t in (-1, N):  # the probe's refusal of a target outside the window's range
                with pytest.raises(api.RelateError, match="rl_debug_window_place"):
                    part[m].place(t)
            probe(part[m], N, seen[m])
        launches = {m: 1 for m in part}
        compared = 0
        for s in range(s0, s1 + 1):
            if s > s0:
                for win in list(full.values()) + list(part.values()) + ([ow] if ow else []):
                    win.advance(s)
            M = None
            for m in part:
                # (the matrix stays on the device: asking for it is what moves a bounded window on)
                assert api.lib().rl_window_matrix(C.c_void_p(part[m]._h), s, None, None) == 0, (m, s)
                if part[m].repaints == launches[m]:
                    continue
                launches[m] = part[m].repaints
                probe(part[m], N, seen[m])
                if launches[m] > 11:
                    continue
                A, B = full[m].matrix(s), part[m].matrix(s)
                assert same(A, B), (m, s, launches[m])
                compared += 1
                if ow:
                    M = ow.matrix(s) if M is None else M
                    assert same(A, M), (m, s, "oracle")
        for m in part:
            assert full[m].repaints == 1 and launches[m] >= 3, (m, launches[m])
            seen[m]["launches"] = launches[m]
            PLACES.setdefault((rc.tile_of(N), m), []).append(seen[m])
        assert compared >= 2 * len(part)
    finally:
        for win in list(full.values()) + list(part.values()):
            win.close()
        if ow:
            ow.close()


def test_part_launch_census():
    """what family D's launches reached, by the probe: per (S, waves) and order a launch that started from a kept
    backward state, one from a kept forward state, one that saved each; over the family the first and the last resident
    row at every offset of a checkpoint block.  (It counts what test_part_launches recorded: run the file whole.)"""
    lo, hi = set(), set()
    for tile in rc.INSTANCES:
        for m in rc.ORDERS:
            got = PLACES.get((tile, m), [])
            assert got, (tile, m, "no part-launch case ran")
            for key in ("bstart", "fstart", "bsave", "fsave"):
                assert sum(g[key] for g in got) > 0, (tile, m, key)
            for g in got:
                lo |= g["lo"]
                hi |= g["hi"]
    assert lo == set(range(rc.CK)) and hi == set(range(rc.CK)), (lo, hi)
