"""ctypes binding of librelate_amd.so (include/relate_amd.h).

This is the Python-side mirror of the C ABI: thin wrappers, numpy in / numpy
out.  There is no CPU fallback: if the shared library is missing, or no GPU is
visible when a GPU entry point is called, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librelate_amd.so")

RL_SUM_EXACT = 0
RL_SUM_LANES = 1
RL_SUM_EXACT_SERIAL = 2
RL_SUM_LANES32 = 3
RL_DEBUG_SUM_STASH = 0x100  # rl_debug_wave_sum_ex: or-ed into RL_SUM_EXACT, the terms go through the LDS stash
RL_DEBUG_SUM_REGSTASH = 0x200  # ... split three ways: LDS stash, registers, recomputed (K1's exact backward pass)

_lib = None


class RelateError(RuntimeError):
    pass


def lib():
    """the loaded shared library (raises if it has not been built)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RelateError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C relate_amd/csrc)" % LIB_PATH)
        # (RELATE_AMD_LIB: another build of the library, tools/bench_builder_variants.py)
        L = C.CDLL(os.environ.get("RELATE_AMD_LIB") or LIB_PATH)
        L.rl_last_error.restype = C.c_char_p
        L.rl_version.restype = C.c_char_p
        L.rl_create.restype = C.c_void_p
        L.rl_create.argtypes = [C.c_int]
        L.rl_destroy.argtypes = [C.c_void_p]
        L.rl_total_sites.restype = C.c_longlong
        L.rl_total_sites.argtypes = [C.c_void_p]
        L.rl_window_open.restype = C.c_void_p
        L.rl_window_open.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        L.rl_window_open_bounded.restype = C.c_void_p
        L.rl_window_open_bounded.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_longlong,
                                             C.c_void_p]
        L.rl_window_close.argtypes = [C.c_void_p]
        L.rl_stage_paint.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
        L.rl_stage_build_topology.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                              C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        L.rl_quickbuild.argtypes = [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
        L.rl_set_painting.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.rl_window_matrix_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rl_optimize_section.restype = C.c_int
        L.rl_optimize_section.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int)]
        L.rl_stage_optimize_parameters.restype = C.c_int
        L.rl_stage_optimize_parameters.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int,
                                                   C.POINTER(C.c_float), C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.rl_debug_map_mutation.restype = C.c_int
        L.rl_debug_map_mutation.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rl_debug_cancel_rowmin.restype = C.c_int
        L.rl_debug_cancel_rowmin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        L.rl_compare_trees.restype = C.c_int
        L.rl_compare_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rl_compare_anc.restype = C.c_int
        L.rl_compare_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_char_p]
        L.rl_pairwise_trees.restype = C.c_int
        L.rl_pairwise_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.POINTER(C.c_longlong)]
        L.rl_pairwise_anc.restype = C.c_int
        L.rl_pairwise_anc.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        L.rl_coalrate_batch_trees.argtypes = [C.c_int]
        L.rl_coalrate_epochs.argtypes = [C.c_float, C.c_char_p, C.c_void_p, C.POINTER(C.c_int)]
        L.rl_coalrate_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p]
        L.rl_coalrate_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.POINTER(C.c_int)]
        L.rl_coalrate_write_bin.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.rl_coalrate_read_bin.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int)]
        L.rl_coalrate_finalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rl_coalrate_finalize_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        L.rl_frequency_batch_trees.argtypes = [C.c_int]
        L.rl_frequency_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int)]
        L.rl_frequency_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                       C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        L.rl_mutrate_batch_trees.argtypes = [C.c_int]
        L.rl_mutrate_epochs.argtypes = [C.c_float, C.c_char_p, C.c_void_p, C.POINTER(C.c_int)]
        L.rl_mutrate_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rl_mutrate_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_longlong)]
        L.rl_mutrate_write.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rl_mutctx_category_names.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        L.rl_mutctx_category.argtypes = [C.c_char_p]
        L.rl_mutctx_count_bases.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                            C.c_longlong, C.c_void_p]
        L.rl_mutctx_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong,
                                      C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rl_mutctx_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rl_mutctx_write.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rl_mutctx_read.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.rl_mutctx_sum.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        L.rl_mutctx_finalize.argtypes = [C.c_char_p, C.c_char_p]
        L.rl_coaltree_batch_trees.argtypes = [C.c_int]
        L.rl_coaltree_num_blocks.argtypes = [C.c_longlong, C.c_int]
        L.rl_coaltree_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.rl_coaltree_anc.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_int)]
        L.rl_coaltree_rates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rl_coaltree_write.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rl_subtrees_batch_trees.argtypes = [C.c_int]
        L.rl_subtrees_trees.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rl_subtrees_poplabels.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                            C.POINTER(C.c_int), C.c_char_p, C.POINTER(C.c_int)]
        L.rl_subtrees_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
        L.rl_subtrees_rewrite.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
        L.rl_selection_logp.argtypes = [C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(C.c_float)]
        L.rl_selection_files.argtypes = [C.c_char_p, C.c_char_p]
        L.rl_window_copying.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rl_window_copying_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rl_copying_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
        L.rl_copying_weights_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rl_copying_rows_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rl_stage_copying_matrix.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_char_p]
        _lib = L
    return _lib


class PaintTimeout(RelateError):
    """RL_ETIMEOUT: a segmented paint() gave up waiting for a hand-off"""


RL_ETIMEOUT = -8


def _check(rc):
    if rc == RL_ETIMEOUT:
        raise PaintTimeout("librelate_amd error %d: %s" % (rc, lib().rl_last_error().decode()))
    if rc != 0:
        raise RelateError("librelate_amd error %d: %s" % (rc, lib().rl_last_error().decode()))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().rl_device_count()


def debug_wave_sum(x, sum_mode, rows_per_group=1, mismatch=None, th=0.001, nth=0.999, stash=False, regstash=False):
    """rl_debug_wave_sum_ex: the kernels' sum of each row of x [batch][n] (terms (mismatch ? th : nth) * x if
    mismatch is given; stash: computed once into the LDS stash of K1's exact backward pass and read back from it;
    regstash: split as that pass splits them, term_split(S): the first through the stash, the last held in registers,
    the rest recomputed) -> (sums [batch], stats), stats = the RL_SUM_EXACT path counters, counted per wave"""
    if stash:
        sum_mode |= RL_DEBUG_SUM_STASH
    if regstash:
        sum_mode |= RL_DEBUG_SUM_REGSTASH
    x = np.ascontiguousarray(x, dtype=np.float64)
    batch, n = x.shape
    if mismatch is not None:
        mismatch = np.ascontiguousarray(mismatch, dtype=np.uint8)
        assert mismatch.shape == x.shape
    out = np.empty(batch, np.float64)
    st = np.zeros(8, np.uint64)
    f = lib().rl_debug_wave_sum_ex
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                  C.c_void_p]
    _check(f(_p(x), n, batch, rows_per_group, sum_mode, _p(mismatch), th, nth, _p(out), _p(st)))
    return out, {"sums": int(st[0]), "fallbacks": int(st[1]), "walked": int(st[2]), "reruns": int(st[3])}


def debug_alloc_peek(nbytes, fill=None):
    """rl_debug_alloc_peek: the bytes of the device block the library's memory cache hands out for a request of
    nbytes, all of the block (it may be larger than asked for) -> uint8 array; fill (0..255): the block is then
    overwritten with that byte on the device before it goes back to the cache"""
    nbytes = int(nbytes)
    out = np.empty(nbytes + nbytes // 8 + 4096, np.uint8)
    got = C.c_size_t()
    f = lib().rl_debug_alloc_peek
    f.argtypes = [C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    _check(f(nbytes, -1 if fill is None else int(fill), _p(out), C.byref(got)))
    return out[:got.value].copy()


def term_split(S):
    """rl_debug_term_split: -> (KS, R): of the S weighted terms of a backward step of tile S the exact order keeps
    the first KS in LDS and the last R in registers (host code, no GPU)"""
    ks, r = C.c_int(), C.c_int()
    _check(lib().rl_debug_term_split(int(S), C.byref(ks), C.byref(r)))
    return ks.value, r.value


def walk_table(A4, p0, sh, delta_lo, delta_hi):
    """rl_debug_walk_table: the exact order's hop over a tie lane for delta_lo .. delta_hi -> (packable, through the
    packed table [int32], the literal form [int32]) (host code, no GPU)"""
    A4 = np.ascontiguousarray(A4, dtype=np.int32)
    assert A4.shape == (4,)
    n = int(delta_hi) - int(delta_lo) + 1
    tab, ref = np.empty(max(n, 0), np.int32), np.empty(max(n, 0), np.int32)
    ok = C.c_int()
    f = lib().rl_debug_walk_table
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    _check(f(_p(A4), int(p0), int(sh), int(delta_lo), int(delta_hi), C.byref(ok), _p(tab), _p(ref)))
    return bool(ok.value), tab, ref


WALK_TRANSLATION, WALK_TABLE, WALK_CONSTANT = 0, 1, 2


def walk_lanes(records, entry_delta=0):
    """rl_debug_walk_lanes: the exact order's walk over one wave's lanes, records [lanes][7] int32 = (kind, U_0, U_1,
    U_2, U_3, p0, sh) with kind WALK_TRANSLATION (delta -> delta + U_0), WALK_TABLE (a head with a hop table) or
    WALK_CONSTANT (a head that exits at U_0) -> (exit offset lane by lane in the literal form, exit offset from the
    add-scan of the translations and the walk over the heads) (host code, no GPU)"""
    records = np.ascontiguousarray(records, dtype=np.int32)
    assert records.ndim == 2 and records.shape[1] == 7
    lit, scan = C.c_int(), C.c_int()
    f = lib().rl_debug_walk_lanes
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _check(f(_p(records), int(records.shape[0]), int(entry_delta), C.byref(lit), C.byref(scan)))
    return lit.value, scan.value


def paint_segment_range(lo, hi, seg, s):
    """rl_paint_segment_range: -> (first, last): segment s of seg walks [first, last) of the step range [lo, hi)
    (host code, no GPU; the kernels run the same function)"""
    a, b = C.c_int(), C.c_int()
    _check(lib().rl_paint_segment_range(int(lo), int(hi), int(seg), int(s), C.byref(a), C.byref(b)))
    return a.value, b.value


def tile_fit(N):
    """rl_tile_fit: -> (S, waves, tail, live) of K1's register tile for N haplotypes (host code, no GPU)"""
    s, w, t, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _check(lib().rl_tile_fit(int(N), C.byref(s), C.byref(w), C.byref(t), C.byref(l)))
    return s.value, w.value, t.value, l.value


class Context:
    """One chunk on one GPU (rl_ctx)."""

    def __init__(self, device=0):
        self._h = lib().rl_create(device)
        if not self._h:
            raise RelateError(lib().rl_last_error().decode())
        self.N = self.L = self.W = 0

    def close(self):
        if self._h:
            lib().rl_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _dims(self):
        n, l, w = C.c_int(), C.c_int(), C.c_int()
        _check(lib().rl_chunk_dims(C.c_void_p(self._h), C.byref(n), C.byref(l), C.byref(w)))
        self.N, self.L, self.W = n.value, l.value, w.value

    def load_chunk(self, out_dir, chunk_index=0):
        _check(lib().rl_load_chunk(C.c_void_p(self._h), out_dir.encode(), chunk_index))
        self._dims()

    def set_chunk(self, seq, r, rpos, wb):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        L, N = seq.shape
        r = np.ascontiguousarray(r, dtype=np.float64)
        rpos = np.ascontiguousarray(rpos, dtype=np.float64)
        wb = np.ascontiguousarray(wb, dtype=np.int32)
        assert len(r) == L and len(rpos) == L + 1
        _check(lib().rl_set_chunk(C.c_void_p(self._h), N, L, _p(seq), _p(r), _p(rpos), _p(wb), len(wb) - 1))
        self._dims()

    def set_chunk_bits(self, N, bits, r, rpos, wb):
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        L, rw = bits.shape
        r = np.ascontiguousarray(r, dtype=np.float64)
        rpos = np.ascontiguousarray(rpos, dtype=np.float64)
        wb = np.ascontiguousarray(wb, dtype=np.int32)
        _check(lib().rl_set_chunk_bits(C.c_void_p(self._h), N, L, _p(bits), rw, _p(r), _p(rpos), _p(wb),
                                       len(wb) - 1))
        self._dims()

    def set_painting(self, theta, rho):
        _check(lib().rl_set_painting(C.c_void_p(self._h), theta, rho))

    def set_target_range(self, k_begin, k_end):
        """shard ONE chunk by target haplotype: this context handles targets k_begin .. k_end-1"""
        _check(lib().rl_set_target_range(C.c_void_p(self._h), int(k_begin), int(k_end)))

    def target_range(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().rl_target_range(C.c_void_p(self._h), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_window_range(self, w_first, w_last):
        """paint() keeps the stepping stones of windows w_first .. w_last only (rl_set_window_range)"""
        _check(lib().rl_set_window_range(C.c_void_p(self._h), int(w_first), int(w_last)))

    def window_range(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().rl_window_range(C.c_void_p(self._h), C.byref(a), C.byref(b)))
        return a.value, b.value

    def paint_account(self):
        """-> (forward steps, backward steps, stone bytes) of the last paint() (rl_paint_account)"""
        f, b, n = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(lib().rl_paint_account(C.c_void_p(self._h), C.byref(f), C.byref(b), C.byref(n)))
        return f.value, b.value, n.value

    def total_sites(self):
        v = lib().rl_total_sites(C.c_void_p(self._h))
        if v < 0:
            _check(int(v))
        return v

    def prepare(self):
        """plan + uploads + allocations, so that paint() times only the kernels"""
        _check(lib().rl_prepare(C.c_void_p(self._h)))

    def paint(self, sum_mode=RL_SUM_EXACT):
        """-> kernel milliseconds"""
        ms = C.c_float(0)
        _check(lib().rl_paint(C.c_void_p(self._h), sum_mode, C.byref(ms)))
        return ms.value

    def set_paint_split(self, split):
        """one launch per direction (so that paint_times() has something to report) instead of one for both"""
        _check(lib().rl_set_paint_split(C.c_void_p(self._h), int(split)))

    def set_paint_segments(self, backward, forward):
        """segments per backward / forward pass of the merged launch: 0 automatic, 1 off (rl_set_paint_segments)"""
        _check(lib().rl_set_paint_segments(C.c_void_p(self._h), int(backward), int(forward)))

    def paint_segments(self):
        """-> (backward, forward) segments per pass that the next exact / lanes paint() will use"""
        b, f = C.c_int(), C.c_int()
        _check(lib().rl_paint_segments(C.c_void_p(self._h), C.byref(b), C.byref(f)))
        return b.value, f.value

    def paint_launched_segments(self):
        """-> (backward, forward) segments per pass that the last paint() launched (rl_paint_launched_segments)"""
        b, f = C.c_int(), C.c_int()
        _check(lib().rl_paint_launched_segments(C.c_void_p(self._h), C.byref(b), C.byref(f)))
        return b.value, f.value

    def set_paint_fit(self, fit):
        """K1 runs the variant of the register tile fitted to N (True, the default) or always the loose one"""
        _check(lib().rl_set_paint_fit(C.c_void_p(self._h), int(fit)))

    @property
    def tile(self):
        s, w = C.c_int(), C.c_int()
        _check(lib().rl_register_tile(C.c_void_p(self._h), C.byref(s), C.byref(w)))
        return s.value

    @property
    def waves(self):
        s, w = C.c_int(), C.c_int()
        _check(lib().rl_register_tile(C.c_void_p(self._h), C.byref(s), C.byref(w)))
        return w.value

    def paint_times(self):
        """-> (forward kernel ms, backward kernel ms) of the last paint()"""
        f, b = C.c_float(0), C.c_float(0)
        _check(lib().rl_paint_times(C.c_void_p(self._h), C.byref(f), C.byref(b)))
        return f.value, b.value

    def stones(self, w):
        """stepping stones of window w: one row per target of the context (all N by default)"""
        N = self.N
        k0, k1 = self.target_range()
        n = k1 - k0
        out = dict(alpha=np.empty((n, N), np.float32), beta=np.empty((n, N), np.float32),
                   ls_alpha=np.empty(n, np.float32), ls_beta=np.empty(n, np.float32),
                   bsnp_begin=np.empty(n, np.int32), bsnp_end=np.empty(n, np.int32))
        _check(lib().rl_get_stones(C.c_void_p(self._h), w, _p(out["alpha"]), _p(out["beta"]),
                                   _p(out["ls_alpha"]), _p(out["ls_beta"]), _p(out["bsnp_begin"]),
                                   _p(out["bsnp_end"])))
        return out

    def write_paint_files(self, paint_dir):
        os.makedirs(paint_dir, exist_ok=True)
        _check(lib().rl_write_paint_files(C.c_void_p(self._h), paint_dir.encode()))

    def write_paint_file(self, w, path):
        """window w's paint file alone (rl_write_paint_file)"""
        _check(lib().rl_write_paint_file(C.c_void_p(self._h), int(w), path.encode()))

    def paint_record(self, w, k):
        """-> bytes: target k's record of window w's paint file (rl_paint_record)"""
        n = C.c_size_t(0)
        _check(lib().rl_paint_record(C.c_void_p(self._h), int(w), int(k), None, C.c_size_t(0), C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().rl_paint_record(C.c_void_p(self._h), int(w), int(k), buf, C.c_size_t(n.value), C.byref(n)))
        return buf.raw[:n.value]

    def optimize_section(self, section, theta, rec_factor):
        """rl_optimize_section: SNPs of `section` that do not map onto the tree built at them, for one grid point of
        `--mode OptimizeParameters` (the context must be painted)"""
        n = C.c_int(0)
        _check(lib().rl_optimize_section(C.c_void_p(self._h), int(section), float(theta), float(rec_factor),
                                         C.byref(n)))
        return n.value

    def copying_matrix(self, w_first=0, w_last=None, sum_mode=RL_SUM_EXACT):
        """rl_copying_matrix: the coancestry matrix of windows w_first .. w_last (default: the last) of the painted
        context -> (C [targets of the context][N] float64, W = SNPs covered)"""
        k0, k1 = self.target_range()
        Cm = np.zeros((k1 - k0, self.N), np.float64)
        W = C.c_longlong(0)
        _check(lib().rl_copying_matrix(C.c_void_p(self._h), int(w_first), self.W - 1 if w_last is None else int(w_last),
                                       sum_mode, _p(Cm), C.byref(W)))
        return Cm, W.value

    def open_window(self, w, paint_file=None, first_snp=None, sum_mode=RL_SUM_EXACT, max_rows=0):
        """max_rows > 0: keep at most that many posterior rows resident (rl_window_open_bounded)"""
        return Window(self, w, paint_file, first_snp, sum_mode, max_rows)


class Window:
    """DistanceMeasure for one window (rl_window): topology resident in HBM."""

    def __init__(self, ctx, w, paint_file, first_snp, sum_mode, max_rows=0):
        self.ctx = ctx
        ms = C.c_float(0)
        fs = -1 if first_snp is None else int(first_snp)
        self._h = lib().rl_window_open_bounded(C.c_void_p(ctx._h), w, paint_file.encode() if paint_file else None,
                                               fs, sum_mode, int(max_rows), C.byref(ms))
        if not self._h:
            raise RelateError(lib().rl_last_error().decode())
        self.repaint_ms = ms.value
        s, e = C.c_int(), C.c_int()
        _check(lib().rl_window_bounds(C.c_void_p(self._h), C.byref(s), C.byref(e)))
        self.start, self.end = s.value, e.value

    def close(self):
        if self._h:
            lib().rl_window_close(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.close()

    def rows(self, n):
        return lib().rl_window_rows(C.c_void_p(self._h), n)

    @property
    def repaints(self):
        """times RePaintSection has run for this window (> 1 only for a bounded one)"""
        return lib().rl_window_repaints(C.c_void_p(self._h))

    def place(self, n):
        """rl_debug_window_place: where the last RePaint launch put target n -> dict(row_lo, row_hi, start_row,
        save_row, fstart_row, fsave_row, partial, nostrip); host bookkeeping, nothing is launched"""
        out = np.zeros(8, np.int32)
        _check(lib().rl_debug_window_place(C.c_void_p(self._h), int(n), _p(out)))
        keys = ("row_lo", "row_hi", "start_row", "save_row", "fstart_row", "fsave_row", "partial", "nostrip")
        return dict(zip(keys, (int(x) for x in out)))

    def topology(self, n):
        D, N = self.rows(n), self.ctx.N
        top = np.empty((D, N), np.float32)
        ls = np.empty(D, np.float32)
        _check(lib().rl_window_get_topology(C.c_void_p(self._h), n, _p(top), _p(ls)))
        return top, ls

    def advance(self, snp):
        _check(lib().rl_window_advance(C.c_void_p(self._h), snp))

    def matrix(self, snp):
        """distance matrix at snp: the rows of the context's targets (the whole N x N matrix by default)"""
        N = self.ctx.N
        k0, k1 = self.ctx.target_range()
        d = np.empty((k1 - k0, N), np.float32)
        ms = C.c_float(0)
        _check(lib().rl_window_matrix(C.c_void_p(self._h), snp, _p(d), C.byref(ms)))
        self.matrix_ms = ms.value
        return d

    def copying(self, Cm=None, device_ptr=None):
        """rl_window_copying: this window's share of the coancestry matrix, ADDED to Cm ([targets of the context][N]
        float64, zeros by default) and returned; with device_ptr (a device buffer of that shape, e.g. a torch tensor's
        data_ptr()) it is added there and nothing crosses PCIe.  copying_ms: the reduce kernels."""
        ms = C.c_float(0)
        if device_ptr is not None:
            _check(lib().rl_window_copying(C.c_void_p(self._h), C.c_void_p(device_ptr), C.byref(ms)))
            self.copying_ms = ms.value
            return None
        k0, k1 = self.ctx.target_range()
        if Cm is None:
            Cm = np.zeros((k1 - k0, self.ctx.N), np.float64)
        assert Cm.dtype == np.float64 and Cm.shape == (k1 - k0, self.ctx.N) and Cm.flags.c_contiguous
        _check(lib().rl_window_copying_host(C.c_void_p(self._h), _p(Cm), C.byref(ms)))
        self.copying_ms = ms.value
        return Cm

    def matrix_rows_into(self, snp, device_ptr):
        """the same rows written to a device buffer ((k_end-k_begin)*N floats), e.g. a torch tensor's
        data_ptr(): the send buffer of relate_amd.dist.all_gather_rows"""
        ms = C.c_float(0)
        _check(lib().rl_window_matrix_rows_device(C.c_void_p(self._h), snp, C.c_void_p(device_ptr), C.byref(ms)))
        self.matrix_ms = ms.value


def quickbuild(d, theta=0.001, prior=None):
    """MinMatch::QuickBuild on an N x N float matrix -> parent array (2N-1)"""
    d = np.array(d, dtype=np.float32, order="C")
    N = d.shape[0]
    parent = np.empty(2 * N - 1, np.int32)
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
    _check(lib().rl_quickbuild(N, theta, _p(d), _p(pr), _p(parent), None, None))
    return parent


class Builder:
    """One MinMatch for a sequence of trees (rl_builder): device=None builds on the host, an int on that GPU."""

    def __init__(self, N, theta=0.001, device=None):
        L = lib()
        L.rl_builder_create.restype = C.c_void_p
        L.rl_builder_create.argtypes = [C.c_int, C.c_double, C.c_int]
        L.rl_builder_build.argtypes = [C.c_void_p] * 6
        L.rl_builder_last_on_gpu.argtypes = [C.c_void_p]
        L.rl_builder_destroy.argtypes = [C.c_void_p]
        self.N = N
        self._h = L.rl_builder_create(N, theta, -1 if device is None else int(device))
        if not self._h:
            raise RelateError(L.rl_last_error().decode())

    def build(self, d, prior=None):
        """-> (parent[2N-1], child_left[N-1], child_right[N-1])"""
        N = self.N
        d = np.array(d, dtype=np.float32, order="C")
        pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
        parent = np.empty(2 * N - 1, np.int32)
        cl = np.empty(N - 1, np.int32)
        cr = np.empty(N - 1, np.int32)
        _check(lib().rl_builder_build(C.c_void_p(self._h), _p(d), _p(pr), _p(parent), _p(cl), _p(cr)))
        return parent, cl, cr

    def set_sample_ages(self, ages):
        ages = np.ascontiguousarray(ages, dtype=np.float64)
        _check(lib().rl_builder_set_sample_ages(C.c_void_p(self._h), _p(ages), len(ages)))

    @property
    def last_on_gpu(self):
        return lib().rl_builder_last_on_gpu(C.c_void_p(self._h)) == 1

    CENSUS = ("max_rebuilt", "merges_rebuilt_tail", "max_draws", "merges_draws_global", "merges_draws_bucketed",
              "init_draws", "max_partners", "first_sym_merge", "sym_merges")

    def census(self):
        """rl_builder_census: what the lists of the last tree this builder's HOST code built had to hold"""
        out = np.zeros(len(self.CENSUS), np.int64)
        L = lib()
        L.rl_builder_census.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        n = L.rl_builder_census(C.c_void_p(self._h), _p(out), len(out))
        if n != len(out):
            raise RelateError("rl_builder_census: %d counts, %d expected" % (n, len(out)))
        return dict(zip(self.CENSUS, (int(x) for x in out)))

    def close(self):
        if self._h:
            lib().rl_builder_destroy(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.close()


def builder_kind(N, ages=False):
    """rl_debug_builder_kind (needs a device) -> (layout, register slots per thread, workgroups per CU)"""
    layout, slots, per_cu = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L = lib()
    L.rl_debug_builder_kind.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _check(L.rl_debug_builder_kind(N, 1 if ages else 0, C.byref(layout), C.byref(slots), C.byref(per_cu)))
    return layout.value, slots.value, per_cu.value


def copying_weights_host(site, rpos, s_begin, s_end):
    """rl_copying_weights_host: the row weights of one target in the window that owns the SNPs [s_begin, s_end)"""
    site = np.ascontiguousarray(site, dtype=np.int32)
    rpos = np.ascontiguousarray(rpos, dtype=np.float64)
    wt = np.zeros(len(site), np.float64)
    _check(lib().rl_copying_weights_host(_p(site), len(site), _p(rpos), int(s_begin), int(s_end), _p(wt)))
    return wt


def copying_rows_host(rows, weights, c_row=None):
    """rl_copying_rows_host: the host twin of the device's reduction; rows [D][N] float32 -> c_row [N] (added to)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    D, N = rows.shape
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    assert len(weights) == D
    c_row = np.zeros(N, np.float64) if c_row is None else c_row
    _check(lib().rl_copying_rows_host(_p(rows), _p(weights), D, N, _p(c_row)))
    return c_row


def read_cpy(path):
    """a .cpy file of `Relate --mode CopyingMatrix` -> dict(N, chunk, first_snp, end_snp, W, C [N][N] float64)"""
    with open(path, "rb") as f:
        N, chunk, first_snp, end_snp = np.frombuffer(f.read(16), "<i4")
        W = int(np.frombuffer(f.read(8), "<i8")[0])
        Cm = np.frombuffer(f.read(), "<f8")
    if Cm.size != int(N) * int(N):
        raise RelateError("%s: %d doubles behind the header, %d x %d expected" % (path, Cm.size, N, N))
    return dict(N=int(N), chunk=int(chunk), first_snp=int(first_snp), end_snp=int(end_snp), W=W,
                C=Cm.reshape(int(N), int(N)).copy())


MATRIX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)  # rl_matrix_fn / rl_matrix_dev_fn


class Shard:
    """One rank's share of a chunk sharded by target haplotype (rl_shard, BASELINE.json config #5): the chunk loaded
    for targets [k_begin, k_end), their stepping stones painted and resident (from_paint_files=False) or read from
    the Paint stage's files.  rows(): this shard's rows of a section's distance matrix, to a device buffer;
    build_section(): the tree-sequence loop of a section this rank owns, its matrices supplied by callbacks."""

    def __init__(self, out_dir, chunk_index, k_begin, k_end, painting=None, sum_mode=RL_SUM_EXACT, device=0,
                 from_paint_files=False):
        L = lib()
        L.rl_shard_open.restype = C.c_void_p
        L.rl_shard_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.c_int, C.c_int]
        L.rl_shard_close.argtypes = [C.c_void_p]
        L.rl_shard_dims.argtypes = [C.c_void_p] * 6
        L.rl_shard_section_bounds.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rl_shard_set_window_rows.argtypes = [C.c_void_p, C.c_longlong]
        L.rl_shard_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rl_shard_release_section.argtypes = [C.c_void_p, C.c_int]
        L.rl_shard_expect_builders.argtypes = [C.c_void_p, C.c_int]
        L.rl_shard_build_section.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, MATRIX_FN, MATRIX_FN,
                                             C.c_void_p, C.c_void_p]
        L.rl_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        th, rho = painting if painting else (0.001, 1.0)
        self.device = device
        self._h = L.rl_shard_open(out_dir.encode(), chunk_index, k_begin, k_end, 1 if painting else 0, th, rho,
                                  sum_mode, device, 1 if from_paint_files else 0)
        if not self._h:
            raise RelateError(L.rl_last_error().decode())
        v = [C.c_int() for _ in range(5)]
        _check(L.rl_shard_dims(C.c_void_p(self._h), *[C.byref(x) for x in v]))
        self.N, self.L, self.W, self.k_begin, self.k_end = [x.value for x in v]

    def close(self):
        if self._h:
            lib().rl_shard_close(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.close()

    def section_bounds(self, section):
        a, b = C.c_int(), C.c_int()
        _check(lib().rl_shard_section_bounds(C.c_void_p(self._h), section, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_window_rows(self, rows):
        _check(lib().rl_shard_set_window_rows(C.c_void_p(self._h), int(rows)))

    def rows(self, section, snp, device_ptr):
        """rows k_begin..k_end-1 of the section's distance matrix at snp -> (k_end-k_begin)*N floats at device_ptr"""
        _check(lib().rl_shard_rows(C.c_void_p(self._h), section, snp, C.c_void_p(device_ptr)))

    def release_section(self, section):
        _check(lib().rl_shard_release_section(C.c_void_p(self._h), section))

    def expect_builders(self, n):
        _check(lib().rl_shard_expect_builders(C.c_void_p(self._h), int(n)))

    def copy_on_device(self, dst_ptr, src_ptr, nbytes):
        _check(lib().rl_device_copy(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), nbytes, self.device))

    def build_section(self, section, matrix, matrix_dev=None, build_device=None, no_consistency=False, fb=0):
        """matrix(snp, host_ptr) / matrix_dev(snp, device_ptr): fill the N x N float matrix of `snp` (return None or 0;
        an exception fails the section).  -> number of trees.  Blocks; releases the GIL while the trees are built."""
        errors = []

        def wrap(fn):
            def cb(_user, snp, ptr):
                try:
                    return int(fn(snp, ptr) or 0)
                except BaseException as e:  # (must not propagate through the C frames)
                    errors.append(e)
                    return -1
            return MATRIX_FN(cb)

        c_host = wrap(matrix)
        c_dev = wrap(matrix_dev) if matrix_dev is not None else C.cast(None, MATRIX_FN)
        n = C.c_int(0)
        rc = lib().rl_shard_build_section(C.c_void_p(self._h), section, 1 if no_consistency else 0, fb,
                                          -1 if build_device is None else int(build_device), c_host, c_dev, None,
                                          C.byref(n))
        if errors:
            raise errors[0]
        _check(rc)
        return n.value


def stage_paint(out_dir, chunk_index=0, painting=None, sum_mode=RL_SUM_EXACT, device=0):
    th, rho = painting if painting else (0.001, 1.0)
    _check(lib().rl_stage_paint(out_dir.encode(), chunk_index, 1 if painting else 0, th, rho, sum_mode, device))


def stage_build_topology(out_dir, chunk_index, first_section, last_section, painting=None, no_consistency=False,
                         fb=0, sum_mode=RL_SUM_EXACT, device=0):
    th, rho = painting if painting else (0.001, 1.0)
    _check(lib().rl_stage_build_topology(out_dir.encode(), chunk_index, first_section, last_section,
                                         1 if painting else 0, th, rho, 1 if no_consistency else 0, fb,
                                         sum_mode, device))


# this module's stage_paint_build_topology takes find_equivalent_branches=True (relate_amd.dist.run_chunks asks)
FUSED_FEB = True


def stage_paint_build_topology(out_dir, chunk_index, first_section, last_section, painting=None,
                               no_consistency=False, fb=0, sum_mode=RL_SUM_EXACT, device=0,
                               find_equivalent_branches=False):
    """Paint + BuildTopology of a chunk with the stepping stones kept in HBM (no paint files);
    find_equivalent_branches: the stage downstream fused in (every .anc written once, as that stage leaves it)"""
    if find_equivalent_branches:
        o = stage_opts(painting=painting, flags=1 if no_consistency else 0, fb=fb, sum_mode=sum_mode, device=device,
                       find_equivalent_branches=1)
        return stage_build_topology_ex(out_dir, chunk_index, first_section, last_section, o, fused=True)
    th, rho = painting if painting else (0.001, 1.0)
    f = lib().rl_stage_paint_build_topology
    f.argtypes = lib().rl_stage_build_topology.argtypes
    _check(f(out_dir.encode(), chunk_index, first_section, last_section, 1 if painting else 0, th, rho,
             1 if no_consistency else 0, fb, sum_mode, device))


class StageOpts(C.Structure):
    """rl_stage_opts (include/relate_amd.h): every option of a stage call, per call"""
    _fields_ = [("size", C.c_size_t), ("sum_mode", C.c_int), ("device", C.c_int), ("use_painting", C.c_int),
                ("theta", C.c_double), ("rho", C.c_double), ("flags", C.c_int), ("fb", C.c_int),
                ("sample_ages_path", C.c_char_p), ("gpu_build", C.c_int), ("window_rows", C.c_longlong),
                ("window_parts", C.c_int), ("section_threads", C.c_int), ("workers", C.c_int),
                ("repaint_lanes", C.c_int), ("park_stones", C.c_int), ("pin_threads", C.c_int),
                ("find_equivalent_branches", C.c_int), ("paint_windows", C.c_int)]


def stage_opts(**kw):
    """-> StageOpts with rl_stage_opts_init's defaults and the given fields (painting=(theta, rho) sets three)"""
    o = StageOpts()
    lib().rl_stage_opts_init.argtypes = [C.c_void_p]
    lib().rl_stage_opts_init(C.byref(o))
    assert o.size == C.sizeof(StageOpts), "StageOpts is out of step with include/relate_amd.h"
    painting = kw.pop("painting", None)
    if painting:
        o.use_painting, o.theta, o.rho = 1, painting[0], painting[1]
    for k, v in kw.items():
        if k == "sample_ages_path" and v is not None:
            v = v.encode()
        setattr(o, k, v)
    return o


def stage_build_topology_ex(out_dir, chunk_index, first_section, last_section, opts, fused=False):
    """rl_stage_build_topology_ex / rl_stage_paint_build_topology_ex (fused=True) with a StageOpts"""
    f = lib().rl_stage_paint_build_topology_ex if fused else lib().rl_stage_build_topology_ex
    f.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    _check(f(out_dir.encode(), chunk_index, first_section, last_section, C.byref(opts)))


# the grid `Relate --mode OptimizeParameters` tries without --input (pipeline/OptimizeParameters.cpp:76-77)
OPTIMIZE_THETAS = (1e-4, 1e-3, 1e-2, 1e-1)
OPTIMIZE_FACTORS = (0.001, 0.1, 1, 10, 100)


def optimize_parameters(out_dir, chunk, thetas=OPTIMIZE_THETAS, factors=OPTIMIZE_FACTORS, opts=None):
    """rl_stage_optimize_parameters on one chunk of a MakeChunks directory: the chunk is painted once, every
    (theta, recombination factor) pair re-paints and builds a tree at every SNP of every section
    -> int array [len(thetas)][len(factors)]: SNPs that do not map onto their tree (sum over chunks for the
    reference's .opt).  opts: a StageOpts (painting, sum_mode, device, the stage's knobs)."""
    th = np.ascontiguousarray(thetas, dtype=np.float32)
    fa = np.ascontiguousarray(factors, dtype=np.float32)
    counts = np.zeros((len(th), len(fa)), np.int32)
    _check(lib().rl_stage_optimize_parameters(out_dir.encode(), int(chunk), th.ctypes.data_as(C.POINTER(C.c_float)),
                                              len(th), fa.ctypes.data_as(C.POINTER(C.c_float)), len(fa),
                                              C.byref(opts) if opts is not None else None,
                                              counts.ctypes.data_as(C.POINTER(C.c_int))))
    return counts


def map_mutation(parent, carriers):
    """rl_debug_map_mutation: 1 / 2 / 3 (maps / maps flipped / does not map) for a tree given by its parent array"""
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    carriers = np.ascontiguousarray(carriers, dtype=np.uint8)
    N = len(carriers)
    assert len(parent) == 2 * N - 1
    r = lib().rl_debug_map_mutation(N, _p(parent), _p(carriers))
    if r < 0:
        _check(r)
    return r


STAGE_PLAN_INTS = ("nthreads", "concurrent", "cap_rows", "wants_second_lane", "lane2_bytes", "min_block")
STAGE_PLAN_DOUBLES = ("max_rows", "row_bytes", "fixed_bytes", "builder_bytes", "bstate_bytes", "window_bytes")


def debug_stage_plan(N, nloc, S, waves, rows_of, first_section, last_section, stones_per_window, gpu_build, room_known,
                     room, host_threads, window_rows_set, window_rows, window_parts, section_threads_set,
                     section_threads, repaint_lanes, probe):
    """rl_debug_stage_plan: the stage's sizing (stage_plan.h plan_sections) for plain numbers -> dict of the plan's
    fields, window_bytes and min_block those of section `probe`"""
    rows_of = np.ascontiguousarray(rows_of, dtype=np.float64)
    ints = np.zeros(len(STAGE_PLAN_INTS), np.int64)
    doubles = np.zeros(len(STAGE_PLAN_DOUBLES), np.float64)
    f = lib().rl_debug_stage_plan
    f.restype = C.c_int
    f.argtypes = ([C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 6 + [C.c_double, C.c_int, C.c_int, C.c_longlong, C.c_longlong,
                  C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p])
    _check(f(N, nloc, S, waves, _p(rows_of), len(rows_of), first_section, last_section, int(stones_per_window),
             int(gpu_build), int(room_known), float(room), host_threads, int(window_rows_set), window_rows, window_parts,
             int(section_threads_set), section_threads, repaint_lanes, probe, _p(ints), _p(doubles)))
    out = {k: int(v) for k, v in zip(STAGE_PLAN_INTS, ints)}
    out.update({k: float(v) for k, v in zip(STAGE_PLAN_DOUBLES, doubles)})
    return out


def debug_cancel_rowmin(d, carriers, log_ratio):
    """rl_debug_cancel_rowmin: cancel_rowmin_kernel on a copy of the N x N float32 matrix d -> (matrix, row minima)"""
    d = np.array(d, dtype=np.float32, order="C")
    N = d.shape[0]
    carriers = np.ascontiguousarray(carriers, dtype=np.uint8)
    assert d.shape == (N, N) and len(carriers) == N
    rowmin = np.empty(N, np.float32)
    _check(lib().rl_debug_cancel_rowmin(_p(d), N, _p(carriers), float(np.float32(log_ratio)), _p(rowmin)))
    return d, rowmin


class CompareSummary(C.Structure):
    """rl_compare_summary (include/relate_amd.h)"""
    _fields_ = [("N", C.c_int), ("trees_a", C.c_int), ("trees_b", C.c_int), ("intervals", C.c_int),
                ("snp_begin", C.c_int), ("snp_end", C.c_int), ("max_distance", C.c_int),
                ("snps_identical", C.c_longlong), ("mean_normalised", C.c_double), ("share_identical", C.c_double)]


def compare_trees(parents_a, parents_b, pairs=None, device=None):
    """rl_compare_trees: clade (rooted Robinson-Foulds) distance of pairs of trees given as parent arrays.
    parents_a, parents_b: [trees][2N-1] (or one tree each); pairs: [npairs][2] indices (tree of A, tree of B), default
    tree k of A with tree k of B; device: None = the host implementation, an int = that GPU.  -> int32 [npairs]"""
    pa = np.ascontiguousarray(np.atleast_2d(parents_a), dtype=np.int32)
    pb = np.ascontiguousarray(np.atleast_2d(parents_b), dtype=np.int32)
    if pa.shape[1] != pb.shape[1] or pa.shape[1] % 2 == 0:
        raise RelateError("compare_trees: parent arrays of %d and %d nodes" % (pa.shape[1], pb.shape[1]))
    N = (pa.shape[1] + 1) // 2
    if pairs is None:
        if len(pa) != len(pb):
            raise RelateError("compare_trees: %d and %d trees and no pairs given" % (len(pa), len(pb)))
        pairs = np.repeat(np.arange(len(pa)), 2)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if len(pairs) and (pairs[:, 0].max() >= len(pa) or pairs[:, 1].max() >= len(pb)):
        raise RelateError("compare_trees: a pair names a tree that was not given")
    out = np.zeros(len(pairs), np.int32)
    _check(lib().rl_compare_trees(_p(pa), _p(pb), N, len(pairs), _p(pairs), -1 if device is None else int(device),
                                  _p(out)))
    return out


def compare_anc(anc_a, anc_b, device=None, per_interval_path=None):
    """rl_compare_anc: two .anc files position by position -> dict of the summary's fields plus "per_interval": int
    array [intervals][5] of (snp_begin, snp_end, tree of A, tree of B, d), read back from the text file the library
    writes (per_interval_path, or a temporary file)"""
    import tempfile
    s = CompareSummary()
    tmp = None
    if per_interval_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".cmp")
        os.close(fd)
    try:
        path = per_interval_path or tmp
        _check(lib().rl_compare_anc(os.fsencode(anc_a), os.fsencode(anc_b), -1 if device is None else int(device),
                                    C.byref(s), os.fsencode(path)))
        rows = np.loadtxt(path, dtype=np.int64, ndmin=2).reshape(-1, 5)
    finally:
        if tmp:
            os.remove(tmp)
    out = {k: getattr(s, k) for k, _ in CompareSummary._fields_}
    out["per_interval"] = rows
    return out


PAIRWISE_METRICS = {"size": 0, "time": 1}  # RL_PAIRWISE_SIZE, RL_PAIRWISE_TIME


def _pairwise_metric(metric):
    if metric not in PAIRWISE_METRICS:
        raise RelateError("pairwise: metric %r is neither 'size' nor 'time'" % (metric,))
    return PAIRWISE_METRICS[metric], np.float64 if metric == "time" else np.uint64


def pairwise_trees(parents, weights, branch_length=None, metric="size", device=None):
    """rl_pairwise_trees: S(i,j) = sum over the trees of weight * (leaves below the MRCA of i and j: metric "size";
    its height: metric "time", which needs branch_length).  parents, branch_length: [trees][2N-1] (or one tree);
    weights: [trees] integers >= 0; device: None = the host implementation, an int = that GPU.
    -> (S [N][N] uint64 or float64, W = the sum of the weights)"""
    m, dtype = _pairwise_metric(metric)
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    w = np.ascontiguousarray(np.atleast_1d(weights), dtype=np.int64)
    if pa.shape[1] % 2 == 0 or len(w) != len(pa):
        raise RelateError("pairwise_trees: %d parent arrays of %d nodes, %d weights" % (len(pa), pa.shape[1], len(w)))
    bl = None
    if branch_length is not None:
        bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
        if bl.shape != pa.shape:
            raise RelateError("pairwise_trees: branch lengths %s for parents %s" % (bl.shape, pa.shape))
    N = (pa.shape[1] + 1) // 2
    S = np.zeros((N, N), dtype)
    W = C.c_longlong(0)
    _check(lib().rl_pairwise_trees(_p(pa), _p(bl), _p(w), N, len(pa), m, -1 if device is None else int(device), _p(S),
                                   C.byref(W)))
    return S, W.value


def pairwise_anc(paths, metric="size", device=None):
    """rl_pairwise_anc: the same sum over the trees of .anc files (one path or a list, in that order), a tree's weight
    the SNPs it covers -> (S [N][N] uint64 or float64, W = the SNPs covered)"""
    m, dtype = _pairwise_metric(metric)
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    dev = -1 if device is None else int(device)
    N, W = C.c_int(0), C.c_longlong(0)
    _check(lib().rl_pairwise_anc(arr, len(paths), m, dev, None, None, C.byref(N)))
    S = np.zeros((N.value, N.value), dtype)
    _check(lib().rl_pairwise_anc(arr, len(paths), m, dev, _p(S), C.byref(W), C.byref(N)))
    return S, W.value


def coalrate_batch_trees(N):
    """trees per batch of the device path of coalrate_trees / coalrate_anc at N leaves"""
    return lib().rl_coalrate_batch_trees(int(N))


def coalrate_epochs(years_per_gen=28.0, bins=None):
    """rl_coalrate_epochs: the reference's default 31 epoch boundaries (generations), or those of
    `--bins lower,upper,step` -> float32 [E]"""
    ep = np.zeros(4096, np.float32)
    n = C.c_int(len(ep))
    _check(lib().rl_coalrate_epochs(float(years_per_gen), None if bins is None else str(bins).encode(), _p(ep),
                                    C.byref(n)))
    return ep[:n.value].copy()


def coalrate_trees(parents, branch_length, factors, epochs, device=None):
    """rl_coalrate_trees: the epoch-binned counts (D[e][i][j], i < j) and opportunities (D[e][j][i]) of
    CoalescentRateForSection.  parents, branch_length: [trees][2N-1] (or one tree); factors: [trees] floats; epochs:
    [E] floats, epochs[0] = 0, rising; device: None = the host implementation, an int = that GPU.
    -> D [E][N][N] float32"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    f = np.ascontiguousarray(np.atleast_1d(factors), dtype=np.float32)
    ep = np.ascontiguousarray(epochs, dtype=np.float32)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or len(f) != len(pa) or ep.ndim != 1:
        raise RelateError("coalrate_trees: parents %s, branch lengths %s, %d factors" % (pa.shape, bl.shape, len(f)))
    N = (pa.shape[1] + 1) // 2
    D = np.empty((len(ep), N, N), np.float32)
    _check(lib().rl_coalrate_trees(_p(pa), _p(bl), _p(f), N, len(pa), _p(ep), len(ep),
                                   -1 if device is None else int(device), _p(D)))
    return D


def coalrate_anc(anc_path, mut_path, epochs, device=None):
    """rl_coalrate_anc: the same over the trees of a text .anc with the factors of its .mut, the reference's loop
    (its trailing pass included) -> D [E][N][N] float32"""
    ep = np.ascontiguousarray(epochs, dtype=np.float32)
    dev = -1 if device is None else int(device)
    a, m = os.fsencode(anc_path), os.fsencode(mut_path)
    N = C.c_int(0)
    _check(lib().rl_coalrate_anc(a, m, _p(ep), len(ep), dev, None, C.byref(N)))
    D = np.empty((len(ep), N.value, N.value), np.float32)
    _check(lib().rl_coalrate_anc(a, m, _p(ep), len(ep), dev, _p(D), C.byref(N)))
    return D


def coalrate_write_bin(path, epochs, D):
    ep = np.ascontiguousarray(epochs, dtype=np.float32)
    D = np.ascontiguousarray(D, dtype=np.float32)
    if D.ndim != 3 or D.shape[0] != len(ep) or D.shape[1] != D.shape[2]:
        raise RelateError("coalrate_write_bin: %d epochs, planes %s" % (len(ep), D.shape))
    _check(lib().rl_coalrate_write_bin(os.fsencode(path), _p(ep), len(ep), _p(D), D.shape[1]))


def coalrate_read_bin(path):
    """-> (epochs [E] float32, D [E][N][N] float32)"""
    E, N = C.c_int(0), C.c_int(0)
    _check(lib().rl_coalrate_read_bin(os.fsencode(path), None, C.byref(E), None, C.byref(N)))
    ep, D = np.empty(E.value, np.float32), np.empty((E.value, N.value, N.value), np.float32)
    _check(lib().rl_coalrate_read_bin(os.fsencode(path), _p(ep), C.byref(E), _p(D), C.byref(N)))
    return ep, D


def coalrate_finalize(D, group_of_haplotype=None, ngroups=1):
    """rl_coalrate_finalize -> rates [ngroups][ngroups][E] float64 (count over opportunity per group pair and epoch)"""
    D = np.ascontiguousarray(D, dtype=np.float32)
    g = None if group_of_haplotype is None else np.ascontiguousarray(group_of_haplotype, dtype=np.int32)
    if g is not None and len(g) != D.shape[1]:
        raise RelateError("coalrate_finalize: %d groups of haplotypes for %d haplotypes" % (len(g), D.shape[1]))
    rates = np.empty((ngroups, ngroups, D.shape[0]), np.float64)
    _check(lib().rl_coalrate_finalize(_p(D), D.shape[1], D.shape[0], _p(g), int(ngroups), _p(rates)))
    return rates


def coalrate_finalize_files(bin_path, coal_path, poplabels=None):
    """rl_coalrate_finalize_files: out.bin -> out.coal, as FinalizePopulationSize writes it"""
    _check(lib().rl_coalrate_finalize_files(os.fsencode(bin_path), None if poplabels is None else os.fsencode(poplabels),
                                            os.fsencode(coal_path)))


def frequency_batch_trees(N):
    """trees per batch of the device path of frequency_trees / frequency_anc at N leaves"""
    return lib().rl_frequency_batch_trees(int(N))


def frequency_trees(parents, branch_length, snp_tree, snp_branch, epochs, device=None):
    """rl_frequency_trees: the rows of Frequency for SNPs on the branches snp_branch of the trees snp_tree (rising).
    parents, branch_length: [trees][2N-1] (or one tree); epochs: [E] floats, epochs[0] = 0, rising; device: None = the
    host walk, an int = that GPU.
    -> (freq [snps][E+1] int32: carriers per boundary from the oldest to 0, TreeFreq; lin [snps][E+2] int32: lineages
    per boundary, when_DAF_is_half, when_mutation_has_freq2; marks [snps] bool: the row is there (the branch is
    neither -1 nor the root); root_time [trees] float32; host_trees: trees walked on the host)"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    st = np.ascontiguousarray(np.atleast_1d(snp_tree), dtype=np.int32)
    sb = np.ascontiguousarray(np.atleast_1d(snp_branch), dtype=np.int32)
    ep = np.ascontiguousarray(epochs, dtype=np.float32)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or st.shape != sb.shape or st.ndim != 1 or ep.ndim != 1:
        raise RelateError("frequency_trees: parents %s, branch lengths %s, SNP trees %s, SNP branches %s"
                          % (pa.shape, bl.shape, st.shape, sb.shape))
    N, E = (pa.shape[1] + 1) // 2, len(ep)
    freq, lin = np.zeros((len(st), E + 1), np.int32), np.zeros((len(st), E + 2), np.int32)
    marks, root_time, host_trees = np.zeros(len(st), np.uint8), np.zeros(len(pa), np.float32), C.c_int(0)
    _check(lib().rl_frequency_trees(_p(pa), _p(bl), N, len(pa), _p(st), _p(sb), len(st), _p(ep), E,
                                    -1 if device is None else int(device), _p(freq), _p(lin), _p(marks), _p(root_time),
                                    C.byref(host_trees)))
    return freq, lin, marks.astype(bool), root_time, host_trees.value


def frequency_anc(anc_path, mut_path, epochs, freq_path, lin_path, device=None):
    """rl_frequency_anc: out.freq and out.lin of `RelateSelection --mode Frequency` from a text .anc and its .mut
    -> (rows written, trees walked on the host)"""
    ep = np.ascontiguousarray(epochs, dtype=np.float32)
    rows, host_trees = C.c_longlong(0), C.c_int(0)
    _check(lib().rl_frequency_anc(os.fsencode(anc_path), os.fsencode(mut_path), _p(ep), len(ep),
                                  -1 if device is None else int(device), os.fsencode(freq_path), os.fsencode(lin_path),
                                  C.byref(rows), C.byref(host_trees)))
    return rows.value, host_trees.value


def selection_logp(k, fk, N, fN):
    """rl_selection_logp: the reference's log_pvalue(k, fk, N, fN) -> float32"""
    out = C.c_float(0.0)
    _check(lib().rl_selection_logp(int(k), float(fk), int(N), float(fN), C.byref(out)))
    return np.float32(out.value)


def selection_files(in_prefix, out_path):
    """rl_selection_files: in_prefix.freq + in_prefix.lin -> out_path (.sele), as `RelateSelection --mode Selection`"""
    _check(lib().rl_selection_files(os.fsencode(in_prefix), os.fsencode(out_path)))


def mutrate_batch_trees(N):
    """trees per batch of the device path of mutrate_trees / mutrate_anc at N leaves"""
    return lib().rl_mutrate_batch_trees(int(N))


def mutrate_epochs(years_per_gen=28.0, bins=None):
    """rl_mutrate_epochs: the epoch boundaries of `RelateMutationRate --mode Avg` -> [E] float64 (31 by default;
    bins: "lower,upper,step" in log10 years)"""
    ep = np.empty(4096, np.float64)
    E = C.c_int(len(ep))
    _check(lib().rl_mutrate_epochs(float(years_per_gen), None if bins is None else bins.encode(), _p(ep), C.byref(E)))
    return ep[:E.value].copy()


def mutrate_trees(parents, branch_length, epochs, device=None):
    """rl_mutrate_trees: the total branch length of every tree in every epoch.  parents, branch_length: [trees][2N-1]
    (or one tree); epochs: [E] float64, epochs[0] = 0, rising; device: None = the reference's walk on the host, an
    int = that GPU.  -> [trees][E] float64, entry E-1 equal to 0"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or ep.ndim != 1:
        raise RelateError("mutrate_trees: parents %s, branch lengths %s, epochs %s" % (pa.shape, bl.shape, ep.shape))
    out = np.zeros((len(pa), len(ep)), np.float64)
    _check(lib().rl_mutrate_trees(_p(pa), _p(bl), (pa.shape[1] + 1) // 2, len(pa), _p(ep), len(ep),
                                  -1 if device is None else int(device), _p(out)))
    return out


def mutrate_anc(anc_path, mut_path, epochs, dist_path=None, device=None):
    """rl_mutrate_anc: the sums of `RelateMutationRate --mode Avg` over the one-branch SNPs of a text .anc and its
    .mut (dist_path: the --dist file) -> (mutation [E] float64, opportunity [E] float64, mapped SNPs)"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    mutation, opportunity, mapped = np.zeros(len(ep)), np.zeros(len(ep)), C.c_longlong(0)
    _check(lib().rl_mutrate_anc(os.fsencode(anc_path), os.fsencode(mut_path),
                                None if dist_path is None else os.fsencode(dist_path), _p(ep), len(ep),
                                -1 if device is None else int(device), _p(mutation), _p(opportunity), C.byref(mapped)))
    return mutation, opportunity, mapped.value


def mutrate_write(path, epochs, mutation, opportunity):
    """rl_mutrate_write: the _avg.rate file, `epoch rate` per line with rate = (mutation / opportunity) / 1e9"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    m = np.ascontiguousarray(mutation, dtype=np.float64)
    o = np.ascontiguousarray(opportunity, dtype=np.float64)
    if not ep.shape == m.shape == o.shape or ep.ndim != 1:
        raise RelateError("mutrate_write: epochs %s, mutation %s, opportunity %s" % (ep.shape, m.shape, o.shape))
    _check(lib().rl_mutrate_write(os.fsencode(path), _p(ep), len(ep), _p(m), _p(o)))


MUTCTX_CATEGORIES = 96  # the trinucleotide categories of MutationRateWithContext
MUTCTX_DEPTH = 16       # kMutctxDepth: SNPs whose operands a lane of the chains kernel holds at a time
MUTCTX_SNP_CHUNK = 1 << 15  # kMutctxSnpChunk: qualifying SNPs per launch of the chains kernel


def mutctx_category_names():
    """rl_mutctx_category_names: the 96 category names (`AC/AT`: upstream, ancestral/derived, downstream) in index order"""
    buf = C.create_string_buffer(1024)
    n = C.c_int(len(buf))
    _check(lib().rl_mutctx_category_names(buf, C.byref(n)))
    return buf.value.decode().split("\n")[:-1]


def mutctx_category(key):
    """rl_mutctx_category: the index of `upstream downstream ancestral derived` (4 letters), -1 for a key the table lacks"""
    return lib().rl_mutctx_category(key.encode())


def mutctx_count_bases(ancestor_path, mask_path, pos, snp_pos, one_branch):
    """rl_mutctx_count_bases: the bases counted for every SNP and category.  pos: the position list (the --dist file's
    or the .mut's); snp_pos, one_branch: [L] of the .mut -> [L][96] uint32"""
    p = np.ascontiguousarray(pos, dtype=np.int32)
    sp = np.ascontiguousarray(snp_pos, dtype=np.int32)
    ob = np.ascontiguousarray(one_branch, dtype=np.uint8)
    if p.ndim != 1 or sp.ndim != 1 or ob.shape != sp.shape:
        raise RelateError("mutctx_count_bases: pos %s, snp_pos %s, one_branch %s" % (p.shape, sp.shape, ob.shape))
    out = np.zeros((len(sp), MUTCTX_CATEGORIES), np.uint32)
    _check(lib().rl_mutctx_count_bases(os.fsencode(ancestor_path), os.fsencode(mask_path), _p(p), len(p), _p(sp), _p(ob),
                                       len(sp), _p(out)))
    return out


def mutctx_trees(parents, branch_length, snp_tree, snp_counts, epochs, device=None, details=False):
    """rl_mutctx_trees: the opportunity of every epoch and category.  parents, branch_length: [trees][2N-1]; snp_tree
    [S] (not falling) and snp_counts [S][96] uint32: the qualifying SNPs in the .mut's order; device: None = the
    reference's loop on the host, an int = that GPU.  -> [E][96] float64; details: (that, root times [trees] float32,
    seconds [3]: trees | SNP copies | chains kernel, zeros on the host)"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    st = np.ascontiguousarray(snp_tree, dtype=np.int32)
    sc = np.ascontiguousarray(snp_counts, dtype=np.uint32).reshape(-1, MUTCTX_CATEGORIES)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or ep.ndim != 1 or st.ndim != 1 or len(sc) != len(st):
        raise RelateError("mutctx_trees: parents %s, branch lengths %s, epochs %s, SNP trees %s, counts %s"
                          % (pa.shape, bl.shape, ep.shape, st.shape, sc.shape))
    out = np.zeros((len(ep), MUTCTX_CATEGORIES), np.float64)
    roots, seconds = np.zeros(len(pa), np.float32), np.zeros(3, np.float64)
    _check(lib().rl_mutctx_trees(_p(pa), _p(bl), (pa.shape[1] + 1) // 2, len(pa), _p(st), _p(sc), len(st), _p(ep), len(ep),
                                 -1 if device is None else int(device), _p(out), _p(roots), _p(seconds)))
    return (out, roots, seconds) if details else out


def mutctx_anc(anc_path, mut_path, mask_path, ancestor_path, epochs, dist_path=None, device=None):
    """rl_mutctx_anc: `RelateMutationRate --mode WithContextForChromosome` on a text .anc and its .mut -> (mutation
    [E][96], opportunity [E][96], (SNPs read, with one branch, qualifying))"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    mutation, opportunity = np.zeros((len(ep), MUTCTX_CATEGORIES)), np.zeros((len(ep), MUTCTX_CATEGORIES))
    snps = np.zeros(3, np.int64)
    _check(lib().rl_mutctx_anc(os.fsencode(anc_path), os.fsencode(mut_path), os.fsencode(mask_path), os.fsencode(ancestor_path),
                               None if dist_path is None else os.fsencode(dist_path), _p(ep), len(ep),
                               -1 if device is None else int(device), _p(mutation), _p(opportunity), _p(snps)))
    return mutation, opportunity, tuple(int(x) for x in snps)


def mutctx_write(prefix, epochs, mutation, opportunity):
    """rl_mutctx_write: prefix_mut.bin and prefix_opp.bin, the reference's bytes"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    m = np.ascontiguousarray(mutation, dtype=np.float64)
    o = np.ascontiguousarray(opportunity, dtype=np.float64)
    if ep.ndim != 1 or m.shape != (len(ep), MUTCTX_CATEGORIES) or o.shape != m.shape:
        raise RelateError("mutctx_write: epochs %s, mutation %s, opportunity %s" % (ep.shape, m.shape, o.shape))
    _check(lib().rl_mutctx_write(os.fsencode(prefix), _p(ep), len(ep), _p(m), _p(o)))


def mutctx_read(prefix):
    """rl_mutctx_read: prefix_mut.bin and prefix_opp.bin -> (epochs [E], mutation [E][96], opportunity [E][96])"""
    ep = np.zeros(64, np.float64)
    m, o = np.zeros((64, MUTCTX_CATEGORIES)), np.zeros((64, MUTCTX_CATEGORIES))
    E = C.c_int(64)
    _check(lib().rl_mutctx_read(os.fsencode(prefix), _p(ep), C.byref(E), _p(m), _p(o)))
    return ep[:E.value].copy(), m[:E.value].copy(), o[:E.value].copy()


def mutctx_sum(prefix, chromosomes, out_prefix):
    """rl_mutctx_sum: prefix_chr<c>_{mut,opp}.bin of every chromosome name, added in order -> out_prefix_{mut,opp}.bin"""
    _check(lib().rl_mutctx_sum(os.fsencode(prefix), "".join(str(c) + "\n" for c in chromosomes).encode(), os.fsencode(out_prefix)))


def mutctx_finalize(in_prefix, rate_path):
    """rl_mutctx_finalize: in_prefix_{mut,opp}.bin -> the .rate text of `RelateMutationRate --mode Finalize`"""
    _check(lib().rl_mutctx_finalize(os.fsencode(in_prefix), os.fsencode(rate_path)))


COALTREE_BLOCK_SIZE = 1000  # trees per block in the reference's CoalRateForTree


def coaltree_batch_trees(N):
    """trees per batch of the device path of coaltree_trees / coaltree_anc at N leaves"""
    return lib().rl_coaltree_batch_trees(int(N))


def coaltree_num_blocks(ntrees, block_size=COALTREE_BLOCK_SIZE):
    """rl_coaltree_num_blocks: (int)(ntrees / block_size + 1), the blocks of a sequence of ntrees trees"""
    return lib().rl_coaltree_num_blocks(int(ntrees), int(block_size))


def coaltree_trees(parents, branch_length, factors, epochs, block_size=COALTREE_BLOCK_SIZE, device=None):
    """rl_coaltree_trees: the coalescence counts and the pair opportunity of `RelateCoalescentRate --mode
    CoalRateForTree` per block of block_size trees and epoch.  parents, branch_length: [trees][2N-1] (or one tree);
    factors: [trees] float32, the bases every tree persists for; epochs: [E] float64, epochs[0] = 0, rising; device:
    None = the reference's walk on the host, an int = that GPU.  -> (num, denom), each [blocks][E] float64"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    f = np.ascontiguousarray(np.atleast_1d(factors), dtype=np.float32)
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or f.shape != (len(pa),) or ep.ndim != 1 or int(block_size) < 1:
        raise RelateError("coaltree_trees: parents %s, branch lengths %s, factors %s, epochs %s, block size %s"
                          % (pa.shape, bl.shape, f.shape, ep.shape, block_size))
    blocks = C.c_int(coaltree_num_blocks(len(pa), block_size))
    num, denom = np.zeros((blocks.value, len(ep)), np.float64), np.zeros((blocks.value, len(ep)), np.float64)
    _check(lib().rl_coaltree_trees(_p(pa), _p(bl), _p(f), (pa.shape[1] + 1) // 2, len(pa), _p(ep), len(ep),
                                   int(block_size), -1 if device is None else int(device), _p(num), _p(denom),
                                   C.byref(blocks)))
    return num, denom


def coaltree_anc(anc_path, mut_path, epochs, device=None):
    """rl_coaltree_anc: the trees of a text .anc with the factors of its .mut, in the reference's blocks of 1000,
    the blocks added in order -> (num [E] float64, denom [E] float64, trees taken)"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    num, denom, ntrees = np.zeros(len(ep)), np.zeros(len(ep)), C.c_int(0)
    _check(lib().rl_coaltree_anc(os.fsencode(anc_path), os.fsencode(mut_path), _p(ep), len(ep),
                                 -1 if device is None else int(device), _p(num), _p(denom), C.byref(ntrees)))
    return num, denom, ntrees.value


def coaltree_rates(num, denom):
    """rl_coaltree_rates: num / denom where denom != 0, otherwise the rate before it (0 at the start) -> [E] float64"""
    n = np.ascontiguousarray(num, dtype=np.float64)
    d = np.ascontiguousarray(denom, dtype=np.float64)
    if n.shape != d.shape or n.ndim != 1:
        raise RelateError("coaltree_rates: num %s, denom %s" % (n.shape, d.shape))
    rates = np.zeros(len(n), np.float64)
    _check(lib().rl_coaltree_rates(_p(n), _p(d), len(n), _p(rates)))
    return rates


def coaltree_write(path, epochs, rates):
    """rl_coaltree_write: the .coal file of CoalRateForTree: `0 `, the boundaries, `0 0 ` and the rates"""
    ep = np.ascontiguousarray(epochs, dtype=np.float64)
    r = np.ascontiguousarray(rates, dtype=np.float64)
    if ep.shape != r.shape or ep.ndim != 1:
        raise RelateError("coaltree_write: epochs %s, rates %s" % (ep.shape, r.shape))
    _check(lib().rl_coaltree_write(os.fsencode(path), _p(ep), len(ep), _p(r)))


def subtrees_batch_trees(N):
    """trees per batch of the device path of subtrees_trees / subtrees_files at N leaves"""
    return lib().rl_subtrees_batch_trees(int(N))


def subtrees_trees(parents, branch_length, subset, device=None):
    """rl_subtrees_trees: the subtrees of `RelateExtract --mode SubTreesForSubpopulation` for the leaves in `subset`
    (labels, rising).  parents, branch_length: [trees][2N-1] (or one tree); device: None = the reference's loop on the
    host, an int = that GPU.  -> dict(sub_parent [trees][2M-1] int32, sub_bl float64, sub_time float32, convert_index
    [trees][2N-1] int32, number_in_subpop int32)"""
    pa = np.ascontiguousarray(np.atleast_2d(parents), dtype=np.int32)
    bl = np.ascontiguousarray(np.atleast_2d(branch_length), dtype=np.float64)
    su = np.ascontiguousarray(subset, dtype=np.int32)
    if pa.shape[1] % 2 == 0 or bl.shape != pa.shape or su.ndim != 1:
        raise RelateError("subtrees_trees: parents %s, branch lengths %s, subset %s" % (pa.shape, bl.shape, su.shape))
    T, nodes, M = len(pa), pa.shape[1], len(su)
    sub = max(2 * M - 1, 1)
    out = {"sub_parent": np.zeros((T, sub), np.int32), "sub_bl": np.zeros((T, sub), np.float64),
           "sub_time": np.zeros((T, sub), np.float32), "convert_index": np.zeros((T, nodes), np.int32),
           "number_in_subpop": np.zeros((T, nodes), np.int32)}
    _check(lib().rl_subtrees_trees(_p(pa), _p(bl), (nodes + 1) // 2, T, _p(su), M, -1 if device is None else int(device),
                                   _p(out["sub_parent"]), _p(out["sub_bl"]), _p(out["sub_time"]), _p(out["convert_index"]),
                                   _p(out["number_in_subpop"])))
    return out


def read_poplabels(path, pop_of_interest=None):
    """rl_subtrees_poplabels: a .poplabels file as Sample::Read takes it -> (groups: the names sorted,
    group_of_haplotype [haplotypes] int32, of_interest: the sorted indices of the groups named in pop_of_interest
    ("A,B", duplicates ignored, "All"), or None without one)"""
    pops = None if pop_of_interest is None else pop_of_interest.encode()
    nh, ng, nb = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().rl_subtrees_poplabels(os.fsencode(path), pops, None, C.byref(nh), None, C.byref(ng), None, C.byref(nb)))
    goh, flags, names = np.zeros(nh.value, np.int32), np.zeros(ng.value, np.int32), C.create_string_buffer(nb.value + 1)
    _check(lib().rl_subtrees_poplabels(os.fsencode(path), pops, _p(goh), C.byref(nh), _p(flags), C.byref(ng), names, C.byref(nb)))
    groups = names.raw[:nb.value].decode().split("\n")[:-1]
    return groups, goh, (None if pops is None else [g for g in range(ng.value) if flags[g]])


class _SubtreesSummary(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("trees_read", "trees_kept", "snps_read", "snps_kept", "M", "N", "has_freq")]


def subtrees_files(anc_path, mut_path, poplabels_path, pop_of_interest, out_prefix, device=None):
    """rl_subtrees_files: `RelateExtract --mode SubTreesForSubpopulation`: out_prefix.anc (text), .mut and .poplabels
    for the haplotypes of the groups in pop_of_interest ("A,B" or "All") -> dict(trees_read, trees_kept, snps_read,
    snps_kept, M, N, has_freq)"""
    s = _SubtreesSummary()
    _check(lib().rl_subtrees_files(os.fsencode(anc_path), os.fsencode(mut_path), os.fsencode(poplabels_path),
                                   pop_of_interest.encode(), os.fsencode(out_prefix), -1 if device is None else int(device),
                                   C.byref(s)))
    return {n: getattr(s, n) for n, _ in s._fields_}


def subtrees_rewrite(anc_in, mut_in, anc_out, mut_out):
    """rl_subtrees_rewrite: a text .anc and .mut read with every column and written again with the mode's writers"""
    _check(lib().rl_subtrees_rewrite(os.fsencode(anc_in), os.fsencode(mut_in), os.fsencode(anc_out), os.fsencode(mut_out)))


def stage_find_equivalent_branches(out_dir, chunk_index=0):
    _check(lib().rl_stage_find_equivalent_branches(out_dir.encode(), chunk_index))


def num_sections(out_dir, chunk_index=0):
    """number of windows (= BuildTopology sections) of a chunk, from parameters_c<chunk>.bin"""
    p = np.fromfile(os.path.join(out_dir, "parameters_c%d.bin" % chunk_index), dtype=np.int32, count=3)
    return int(p[2]) - 1
