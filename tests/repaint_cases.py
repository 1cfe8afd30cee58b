"""The inputs of test_repaint_geometry_gpu.py (K2 RePaintSection / K3 GetMatrix at every geometry) and what the oracle
says about them: pure numpy and the CPU oracle, no GPU.  test_repaint_cases_cpu.py asserts here, with the oracle alone,
that every case reaches the census its family demands, so the GPU test never fails for lack of an input.

Families (the issue's letters):
  A  every (S, waves) instantiation at both edges of its range of N, three sum orders
  B  degenerate windows: 2..5 rows per target and window, N < 8, L of 2 and 3
  C  dense chunks that rescale often: with A's rows they fill the rescale census of every (S, waves) and order
  D  part launches (bounded windows)
"""
import ctypes as C
import functools

import numpy as np

import rlutil

CK = 6  # REPAINT_CHECKPOINT (relate_amd/csrc/device_types.h): rows per checkpoint block of K2
TILES = (8, 16, 32, 48, 64, 80)
INSTANCES = ((8, 1), (16, 1), (32, 1), (48, 1), (64, 1), (80, 1), (48, 2), (64, 2), (80, 2))
ORDERS = ("exact", "serial", "lanes")  # RL_SUM_EXACT, RL_SUM_EXACT_SERIAL, RL_SUM_LANES


def tile_of(N):
    """(S, waves) the kernels run N at (launch.h target_waves, choose_S)"""
    waves = 2 if N > 5120 else 1
    q, rem = divmod(N, 64 * waves)
    need = q + (1 if rem else 0)
    return min(s for s in TILES if s >= need), waves


def last_live_target(N):
    """the target whose pinned slot lies in the last register any lane uses (test_tile_fit_gpu.last_live_target)"""
    q, rem = divmod(N, 64 * tile_of(N)[1])
    return q + (1 if rem else 0) - 1


def wave1_target(N):
    """two waves: the first target whose slot is in wave 1 (donor 0 of virtual lane 64)"""
    q, rem = divmod(N, 128)
    return 64 * q + min(rem, 64)


def base_targets(N):
    """the targets family A compares at every N: 0 and N - 1 (flat and saturated under flat_targets), 1, the last
    live register's, wave 1's first with two waves, N // 2, N - 2"""
    t = [0, N - 1, 1, last_live_target(N), N // 2, N - 2]
    if tile_of(N)[1] == 2:
        t.append(wave1_target(N))
    return sorted(set(k for k in t if 0 <= k < N))


class Case:
    def __init__(self, name, N, L, wb, density, seed, special=None, extra=(), windows=None, run=None):
        self.name, self.N, self.L, self.wb, self.density, self.seed = name, N, L, list(wb), density, seed
        self.special, self.extra, self.windows, self.run = special, tuple(extra), windows, run

    def chunk(self):
        from test_edge_gpu import random_chunk
        ch = random_chunk(self.N, self.L, self.density, seed=self.seed, wb=self.wb, special=self.special)
        if self.run is not None:
            # a run of SNPs at which target k alone is derived: every donor mismatches, the sums fall by 1 / theta a
            # step and rescale every fourth row (lower = 1e-10, theta = 1e-3): two rescales in one checkpoint block,
            # which a random panel does not give (its sums fall by ~1 / density a step: one rescale in ~12 rows)
            k, first, length = self.run
            ch.seq[first:first + length, :] = ord("0")
            ch.seq[first:first + length, k] = ord("1")
        return ch

    def compared_windows(self):
        return list(self.windows) if self.windows is not None else list(range(len(self.wb) - 1))

    def targets(self):
        """the targets whose every row is compared"""
        return sorted(set(base_targets(self.N)) | set(self.extra))

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------- family A
# q = S with rem = 0, and the first N of the next tile; N = 5000 is the headline configuration's, 10240 the layout's
# maximum.  K1's chunk of these sizes (test_edge_gpu.test_two_wavefronts_per_target).
A_SIZES = (512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5000, 5120, 5121, 6144, 6145, 8192, 8193, 10240)


def case_a(N):
    return Case("A-%d" % N, N, 90, [0, 40, 90], 0.15, seed=N, special="flat_targets")


A_CASES = [case_a(N) for N in A_SIZES]

# ---------------------------------------------------------------- family C
# K1's dense chunk (density 0.5, three windows): N = 389 and one N per remaining tile.
# L = 400 at N = 389 as K1's test has it, 150 elsewhere: the shortest of 400 / 240 / 150 tried at which every tile's
# census is complete.  N = 130 carries no census: it is there for the matrices of every SNP (family E).
# C_EXTRA: targets beyond base_targets, the first of 2, 3, .. that add a missing cell (oracle flags, both orders).
C_EXTRA = {389: (4,), 1500: (2,), 3600: (4,)}
# C_WINDOWS: the windows compared at the two-wave N (the others' paint files, over a gigabyte each, are not written):
# the fewest with which the tile's census stays complete; window 1 holds the run of singletons.
C_WINDOWS = {5800: (1, 2), 7000: (1,), 9000: (1,)}
C_SIZES = {130: 150, 389: 400, 700: 150, 1500: 150, 2500: 150, 3600: 150, 4500: 150, 5800: 150, 7000: 150, 9000: 150}


def case_c(N):
    L = C_SIZES[N]
    if N == 389:  # K1's dense chunk itself (test_paint_segments_gpu.py, test_tile_fit_gpu.py)
        return Case("C-389", N, L, [0, 100, 250, 400], 0.5, seed=5, extra=C_EXTRA.get(N, ()), run=(N // 2, 120, 16))
    return Case("C-%d" % N, N, L, [0, L // 3, 2 * L // 3, L], 0.5, seed=N + 7, extra=C_EXTRA.get(N, ()),
                windows=C_WINDOWS.get(N), run=(N // 2, L // 3 + 20, 16))


# ---------------------------------------------------------------- family B
def b_cases():
    # the chunks K1 is held on (test_edge_gpu.py): twenty 12-SNP windows, a 12-SNP window among long ones, tiny N, tiny L
    out = [Case("B-dense-33", 33, 240, list(range(0, 241, 12)), 0.04, seed=4, special="mono_rows"),
           Case("B-flat-20", 20, 300, [0, 50, 120, 132, 300], 0.2, seed=3, special="flat_targets")]
    for N in (2, 3, 5, 9):
        out.append(Case("B-%d-one" % N, N, 40, [0, 40], 0.3, seed=N))
        out.append(Case("B-%d-two" % N, N, 40, [0, 17, 40], 0.3, seed=N))
    out.append(Case("B-6-L2", 6, 2, [0, 2], 0.5, seed=1))
    out.append(Case("B-6-L3", 6, 3, [0, 3], 0.5, seed=2))
    return out


B_CASES = b_cases()


# ---------------------------------------------------------------- the oracle on a case
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def ro_order(order):
    """the oracle's order of a device order: the exact orders are the reference's serial sum"""
    return rlutil.RoSumOrder(rlutil.RO_SUM_LANES if order == "lanes" else rlutil.RO_SUM_SERIAL, 0, 0)


def quantise(v, N):
    """decode(encode(v)): a stone as the paint file hands it on (collapsed_matrix.hpp:228-296)"""
    o = rlutil.oracle()
    o.ro_encode_stone.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    buf = (C.c_ubyte * o.ro_stone_max_bytes(N))()
    n = o.ro_encode_stone(_vp(v), N, 0, C.c_float(0.0), buf)
    out = np.zeros(N, np.float32)
    bs, ls = C.c_int(), C.c_float()
    assert o.ro_decode_stone(buf, C.c_size_t(n), N, _vp(out), C.byref(bs), C.byref(ls)) == n
    return out


def oracle_records(ch, k, order):
    """target k's records of all windows from the oracle's own Paint: list over windows of dicts like
    rlutil.parse_paint_file's (bb, la, alpha, be, lb, beta)"""
    o = rlutil.oracle()
    N, W = ch.N, ch.W
    bb, be = np.zeros(W, np.int32), np.zeros(W, np.int32)
    al, bt = np.zeros((W, N), np.float32), np.zeros((W, N), np.float32)
    la, lb = np.zeros(W, np.float32), np.zeros(W, np.float32)
    d = ch.ro()
    od = ro_order(order)
    assert o.ro_paint_stepping_stones(C.byref(d), _vp(ch.wb), W, k, C.byref(od), _vp(bb), _vp(be), _vp(al), _vp(bt),
                                      _vp(la), _vp(lb)) > 0
    return [dict(bb=int(bb[w]), be=int(be[w]), la=float(la[w]), lb=float(lb[w]), alpha=quantise(al[w], N),
                 beta=quantise(bt[w], N)) for w in range(W)]


def oracle_repaint(ch, rec, k, order):
    """ro_repaint_section_flags -> (topology [D][N], logscales [D], fwd [D], bwd [D])"""
    o = rlutil.oracle()
    N = ch.N
    cap = rec["be"] - rec["bb"] + 2
    top, ls = np.zeros((cap, N), np.float32), np.zeros(cap, np.float32)
    fwd, bwd = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    d = ch.ro()
    od = ro_order(order)
    ab, be = np.ascontiguousarray(rec["alpha"], np.float32), np.ascontiguousarray(rec["beta"], np.float32)
    D = o.ro_repaint_section_flags(C.byref(d), _vp(ab), _vp(be), rec["bb"], rec["be"], C.c_float(rec["la"]),
                                   C.c_float(rec["lb"]), k, C.byref(od), _vp(top), _vp(ls), _vp(fwd), _vp(bwd))
    assert 2 <= D <= cap
    return top[:D], ls[:D], fwd[:D].astype(bool), bwd[:D].astype(bool)


# ---------------------------------------------------------------- census of rescales (family C's table)
RESCALE_CELLS = ([("fwd", r) for r in range(CK)] + [("bwd", r) for r in range(CK)] + [("two-in-a-block",),
                                                                                     ("last-row",)])


def rescale_cells(fwd, bwd):
    """the cells one target's rows of one window reach: a forward rescale in the step into row i at i % 6 (the divisor
    of the side record at offset i % 6 of its block: the tested walk of product_steps), a backward rescale at row j
    at j % 6, a checkpoint block with two forward rescales, a rescale in the step into the window's last row"""
    D = len(fwd)
    cells = set(("fwd", int(i) % CK) for i in np.flatnonzero(fwd))
    cells |= set(("bwd", int(j) % CK) for j in np.flatnonzero(bwd))
    for b in range(0, D, CK):
        if fwd[b:b + CK].sum() >= 2:
            cells.add(("two-in-a-block",))
    if fwd[D - 1]:
        cells.add(("last-row",))
    return cells


@functools.lru_cache(maxsize=None)
def case_cells(case, order, targets=None):
    """{cell: [(window, target), ..]} over the compared rows of a case in an order, from the oracle's own Paint"""
    ch = case.chunk()
    out = {}
    for k in (targets if targets is not None else case.targets()):
        recs = oracle_records(ch, k, order)
        for w in case.compared_windows():
            _, _, fwd, bwd = oracle_repaint(ch, recs[w], k, order)
            for c in rescale_cells(fwd, bwd):
                out.setdefault(c, []).append((w, k))
    return out


C_CASES = [case_c(N) for N in sorted(C_SIZES)]


def tile_cells(tile, order):
    """the rescale census of one (S, waves) in an order: families A and C together"""
    out = {}
    for case in A_CASES + C_CASES:
        if tile_of(case.N) == tile:
            for c, where in case_cells(case, order).items():
                out.setdefault(c, []).extend((case.name,) + x for x in where)
    return out


# ---------------------------------------------------------------- windows of every target (families B and E)
def cursor_rows(ch, w, n):
    """v_snp_prev of target n at every SNP of window w for a walk that opens the window at its first SNP and advances
    SNP by SNP (anc_builder.cpp:81-101, 487-495): {snp: row}"""
    s0, s1 = int(ch.wb[w]), int(ch.wb[w + 1]) - 1
    der = ch.seq[:, n] == ord("1")
    p = int(der[s0]) if s0 > 0 else 0
    out = {s0: p}
    for s in range(s0 + 1, s1 + 1):
        p += int(der[s])
        out[s] = p
    return out


def matrix_ways(ch, w, rows_of, logs_of):
    """K3's three ways over every SNP and target of window w: counts of direct rows, of interpolated rows with
    ls_prev <= ls_next and with ls_prev > ls_next (anc_builder.cpp:116-178); logs_of(n) -> logscales of target n"""
    s0, s1 = int(ch.wb[w]), int(ch.wb[w + 1]) - 1
    n_direct = n_le = n_gt = 0
    for n in range(ch.N):
        cur, ls = cursor_rows(ch, w, n), logs_of(n)
        for s in range(s0, s1 + 1):
            if ch.seq[s, n] == ord("1") or s == 0 or s == ch.L - 1:
                n_direct += 1
            elif ls[cur[s]] <= ls[cur[s] + 1]:
                n_le += 1
            else:
                n_gt += 1
    return n_direct, n_le, n_gt


# ---------------------------------------------------------------- family D: part launches
# (name, N, L, max_rows): one window of a 0.15 chunk walked SNP by SNP in a bounded window.  The small N sweep the cap,
# and with it where the parts begin and end; each large N (one per tile) has the smallest cap the library takes
# (3 N + 64 rows: max_rows = 1), about seven SNPs a part: nine launches in 64 SNPs, the first of which leave their
# backward states at an anchor (last_snp - part_last >= 24).
D_SMALL = [(130, 400, m) for m in (500, 800, 1300, 2100)] + [(200, 300, m) for m in (700, 1100, 1900)]
D_LARGE = [(N, 64, 1) for N in (700, 1500, 2500, 3600, 4500, 5800, 7000, 9000)]


def case_d(N, L, max_rows):
    c = Case("D-%d-%d" % (N, max_rows), N, L, [0, L], 0.15, seed=N + 3)
    c.max_rows = max_rows
    return c


D_CASES = [case_d(*x) for x in D_SMALL + D_LARGE]
