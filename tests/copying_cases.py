"""The yardstick of the CopyingMatrix tests (test_copying_cpu.py, test_copying_gpu.py): the definition of
include/relate_amd.h restated in numpy on top of the ORACLE's posterior rows (ro_window_open / ro_window_top) and
boundary SNPs (ro_plan_target).  Nothing here calls the library under test.

Every sum is written in the stated order: the weights SNP by SNP in Python floats; the 256 partial sums by a loop over
k (partial t takes donor t + 256 k, k rising: one IEEE addition per element and step, all t at once); the halving by
a loop over h; the accumulation row by row, the product formed first and then added.  np.sum, which sums pairwise,
is not used."""
import ctypes as C

import numpy as np

import rlutil


def plan_bounds(o, ch, n):
    """-> (bsnp_begin[W], bsnp_end[W]) of target n (ro_plan_target)"""
    d = ch.ro()
    L, W = ch.L, ch.W
    site = np.zeros(L + 2, np.int32)
    rp = np.zeros(L + 3, np.float64)
    nx = np.zeros(L + 2, np.float64)
    bb = np.zeros(W + 1, np.int32)
    be = np.zeros(W + 1, np.int32)
    D = o.ro_plan_target(C.byref(d), ch.wb.ctypes.data_as(C.c_void_p), W, n, site.ctypes.data_as(C.c_void_p),
                         rp.ctypes.data_as(C.c_void_p), nx.ctypes.data_as(C.c_void_p),
                         bb.ctypes.data_as(C.c_void_p), be.ctypes.data_as(C.c_void_p))
    assert D >= 2
    return bb[:W].copy(), be[:W].copy()


def row_sites(ch, n, bsnp_begin, bsnp_end):
    """the sites of target n's posterior rows in a window with these boundary SNPs"""
    inner = [s for s in range(int(bsnp_begin) + 1, int(bsnp_end)) if ch.seq[s, n] == ord("1")]
    return [int(bsnp_begin)] + inner + [int(bsnp_end)]


def row_weights(site, rpos, s_begin, s_end):
    """step 1: Wt[D], Python floats, s rising"""
    D = len(site)
    wt = [0.0] * D
    p = 0
    for s in range(int(s_begin), int(s_end)):
        while p + 1 < D and site[p + 1] <= s:
            p += 1
        assert site[p] <= s
        if s == site[p]:
            wt[p] += 1.0
            continue
        a, b = float(rpos[site[p]]), float(rpos[site[p + 1]])
        if a == b:
            wl = wr = 0.5
        else:
            wl = (b - float(rpos[s])) / (b - a)
            wr = (float(rpos[s]) - a) / (b - a)
        wt[p] += wl
        wt[p + 1] += wr
    return np.array(wt, np.float64)


def row_sum(row):
    """step 2: Z of one float32 row"""
    N = len(row)
    K = (N + 255) // 256
    pad = np.zeros(K * 256, np.float64)  # (+0.0 behind the last donor: adding it changes no bit of a sum >= 0)
    pad[:N] = row.astype(np.float64)
    x = np.zeros(256, np.float64)
    for k in range(K):
        x = x + pad[256 * k:256 * (k + 1)]
    h = 128
    while h >= 1:
        x[:h] = x[:h] + x[h:2 * h]
        h //= 2
    return float(x[0])


def reduce_rows(rows, wt, c_row):
    """steps 2 and 3: rows [D][N] float32, wt [D]; c_row [N] float64 is added to, p rising"""
    for p in range(len(wt)):
        if wt[p] == 0.0:
            continue
        Z = row_sum(rows[p])
        assert np.isfinite(Z) and Z > 0.0, (p, Z)
        c = np.float64(wt[p]) / np.float64(Z)
        prod = c * rows[p].astype(np.float64)
        c_row += prod
    return c_row


class OracleWindow:
    """posterior rows of one window from the oracle (paint file -> RePaintSection of every target)"""

    def __init__(self, ch, paint_file, w, threads=4):
        self.o = rlutil.oracle()
        self.ch, self.w = ch, w
        self._d = ch.ro()
        self.h = self.o.ro_window_open(C.byref(self._d), paint_file.encode(), int(ch.wb[w]), threads)
        assert self.h

    def rows(self, n):
        D = self.o.ro_window_rows(C.c_void_p(self.h), n)
        return np.ctypeslib.as_array(C.cast(self.o.ro_window_top(C.c_void_p(self.h), n), C.POINTER(C.c_float)),
                                     (D, self.ch.N))

    def close(self):
        if self.h:
            self.o.ro_window_free(C.c_void_p(self.h))
            self.h = None


def window_inputs(ow, n):
    """-> (rows [D][N], sites, weights) of target n in the oracle window"""
    ch, w = ow.ch, ow.w
    bb, be = plan_bounds(ow.o, ch, n)
    site = row_sites(ch, n, bb[w], be[w])
    rows = ow.rows(n)
    assert rows.shape[0] == len(site), (n, rows.shape, len(site))
    assert site[0] <= ch.wb[w] and (site[-1] >= ch.wb[w + 1] or site[-1] == ch.L - 1)
    return rows, site, row_weights(site, ch.rpos, ch.wb[w], ch.wb[w + 1])


def add_window(ow, Cm, targets=None):
    """the window's share added to Cm [len(targets)][N] (targets: all by default)"""
    targets = range(ow.ch.N) if targets is None else targets
    for i, n in enumerate(targets):
        rows, _, wt = window_inputs(ow, n)
        reduce_rows(rows, wt, Cm[i])
    return Cm


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)
