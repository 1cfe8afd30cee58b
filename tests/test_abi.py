"""The C-ABI shared library loads and exports every symbol include/relate_amd.h
declares; the GPU entry points fail loudly (never fall back) without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rlutil
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "relate_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(rl_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_symbol_is_exported():
    lib = api.lib()
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), "librelate_amd.so does not export %s" % s


def test_version_and_device_count():
    lib = api.lib()
    assert b"relate_amd" in lib.rl_version()
    assert api.device_count() >= 0


def test_no_cpu_fallback_without_gpu():
    if api.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(api.RelateError) as e:
        api.Context()
    assert "no usable HIP device" in str(e.value)
    rc = api.lib().rl_stage_paint(b"/nonexistent", 0, 0, 0.001, 1.0, 0, 0)
    assert rc != 0


def test_synth_panel_deterministic_and_chunk_files_roundtrip(tmp_path):
    a = rlutil.synth_chunk(40, 500, seed=9, budget=20000)
    b = rlutil.synth_chunk(40, 500, seed=9, budget=20000)
    assert np.array_equal(a.seq, b.seq) and np.array_equal(a.wb, b.wb) and a.W > 1
    f = (a.seq == ord("1")).mean()
    assert 0.05 < f < 0.4
    # the product's chunk-file writer and the test-side writer agree byte for byte
    lib = api.lib()
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir()
    a.write(str(d2))
    rc = lib.rl_write_chunk_files(str(d1).encode(), 0, a.N, a.L, a.seq.ctypes.data_as(C.c_void_p),
                                  a.bp.ctypes.data_as(C.c_void_p), a.r.ctypes.data_as(C.c_void_p),
                                  a.rpos.ctypes.data_as(C.c_void_p), a.wb.ctypes.data_as(C.c_void_p), a.W)
    assert rc == 0
    for fn in ["chunk_0.hap", "chunk_0.r", "chunk_0.rpos", "chunk_0.bp", "chunk_0.state", "parameters_c0.bin"]:
        assert open(d1 / fn, "rb").read() == open(d2 / fn, "rb").read(), fn
    c = rlutil.read_chunk(str(d1))
    assert np.array_equal(c.seq, a.seq) and np.array_equal(c.wb, a.wb)


def test_debug_wave_sum_refuses_bad_arguments():
    """rl_debug_wave_sum_ex: RL_EINVAL with a message before any device work (so also without a GPU)"""
    lib = api.lib()
    f = lib.rl_debug_wave_sum_ex
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                  C.c_void_p]
    x = np.ones(4 * 10241)
    out = np.zeros(4)
    px, po = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    bad = [((None, 8, 1, 1, 0, po), "null"), ((px, 8, 1, 1, 0, None), "null"),
           ((px, 0, 1, 1, 0, po), "n=0"), ((px, -5, 1, 1, 0, po), "n=-5"), ((px, 10241, 1, 1, 0, po), "n=10241"),
           ((px, 8, 4, 0, 0, po), "rows_per_group=0"), ((px, 8, 4, 3, 0, po), "rows_per_group=3"),
           ((px, 8, 0, 1, 0, po), "batch=0")]
    for (xp, n, batch, rpg, mode, op), msg in bad:
        rc = f(xp, n, batch, rpg, mode, None, 0.001, 0.999, op, None)
        assert rc == -1, (n, batch, rpg)  # RL_EINVAL
        err = lib.rl_last_error().decode()
        assert err.startswith("rl_debug_wave_sum_ex:") and msg in err, err
    # the old entry is the special case: the same checks
    assert lib.rl_debug_wave_sum(px, 10241, 1, 0, po) == -1
    assert b"n=10241" in lib.rl_last_error()
    assert not out.any()


def test_debug_alloc_peek_refuses_bad_arguments():
    """rl_debug_alloc_peek: RL_EINVAL with a message before any device work; without a GPU a good call says so"""
    lib = api.lib()
    f = lib.rl_debug_alloc_peek
    f.argtypes = [C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    out = np.zeros(16 + 4096, np.uint8)
    got = C.c_size_t(7)
    for args in ((16, -1, None, C.byref(got)), (16, -1, out.ctypes.data_as(C.c_void_p), None),
                 (16, 256, out.ctypes.data_as(C.c_void_p), C.byref(got))):
        assert f(*args) == -1, args[:2]  # RL_EINVAL
        assert lib.rl_last_error().decode().startswith("rl_debug_alloc_peek:")
    if api.device_count() == 0:
        with pytest.raises(api.RelateError, match="no usable HIP device"):
            api.debug_alloc_peek(16)
    assert not out.any()


def test_debug_window_place_refuses_bad_arguments():
    """rl_debug_window_place: RL_EINVAL with a message for a null window or output, nothing written (a target outside
    the window's range: test_repaint_geometry_gpu.py, it needs a window)"""
    lib = api.lib()
    f = lib.rl_debug_window_place
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = np.full(8, 7, np.int32)
    assert f(None, 0, out.ctypes.data_as(C.c_void_p)) == -1  # RL_EINVAL
    assert lib.rl_last_error().decode().startswith("rl_debug_window_place:")
    assert f(None, 0, None) == -1
    assert (out == 7).all()


def test_stage_opts_that_never_saw_init_are_refused():
    """a zeroed rl_stage_opts (size 0) must not silently run with the defaults: RL_EINVAL before any
    device work, from all three *_ex stages"""
    lib = api.lib()
    raw = (C.c_ubyte * 256)()  # larger than the struct, all zero: size field 0
    for fn, args in ((lib.rl_stage_paint_ex, (b"/nonexistent", 0)),
                     (lib.rl_stage_build_topology_ex, (b"/nonexistent", 0, 0, 0)),
                     (lib.rl_stage_paint_build_topology_ex, (b"/nonexistent", 0, 0, 0))):
        fn.argtypes = [C.c_char_p] + [C.c_int] * (len(args) - 1) + [C.c_void_p]
        assert fn(*args, C.cast(raw, C.c_void_p)) == -1, fn  # RL_EINVAL
        assert b"rl_stage_opts_init" in lib.rl_last_error()
