"""The window range of a Paint (rl_set_window_range, rl_stage_opts.paint_windows, --paint_all_windows) as far as it
goes without a GPU: what the header declares, the Python mirror of rl_stage_opts, a struct of the size the header had
before the field, and the command line."""
import ctypes as C
import os
import re
import subprocess

from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
RL_EINVAL = -1


def header():
    hdr = open(os.path.join(ROOT, "include", "relate_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def header_stage_opts_fields():
    body = re.search(r"typedef struct rl_stage_opts \{(.*?)\} rl_stage_opts;", header(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:  # `double theta, rho` declares two
            first, *rest = decl.split(",")
            names.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", first)[-1])
            names += [x.strip() for x in rest]
    return names


def test_header_declares_the_range_entry_points_and_the_field():
    hdr = header()
    assert re.search(r"int rl_set_window_range\(rl_ctx \*ctx, int w_first, int w_last\);", hdr)
    assert re.search(r"int rl_window_range\(const rl_ctx \*ctx, int \*w_first, int \*w_last\);", hdr)
    assert re.search(r"int rl_paint_account\(const rl_ctx \*ctx, long long \*fwd_steps, long long \*bwd_steps,\s*"
                     r"long long \*stone_bytes\);", hdr)
    assert header_stage_opts_fields()[-1] == "paint_windows", "new fields are appended: older callers keep working"
    lib = api.lib()
    for s in ("rl_set_window_range", "rl_window_range", "rl_paint_account"):
        assert hasattr(lib, s), s


def test_python_stage_opts_mirror_the_struct():
    assert [f[0] for f in api.StageOpts._fields_] == header_stage_opts_fields()
    o = api.stage_opts()
    assert o.size == C.sizeof(api.StageOpts)
    assert api.StageOpts.paint_windows.offset + C.sizeof(C.c_int) <= o.size
    assert o.paint_windows == -1  # the default: the fused stage paints the windows of its sections
    assert api.stage_opts(paint_windows=0).paint_windows == 0
    for name in ("set_window_range", "window_range", "paint_account"):
        assert callable(getattr(api.Context, name))


def test_a_struct_of_the_size_before_the_field_is_still_accepted():
    """a caller built against the header before paint_windows passes a struct that ends where the field begins: the
    stage takes it (and fails later, on the chunk that is not there or the device that is not there), it does not
    refuse the struct"""
    lib = api.lib()
    o = api.stage_opts()
    o.size = api.StageOpts.paint_windows.offset
    assert o.size % C.sizeof(C.c_int) == 0 and o.size < C.sizeof(api.StageOpts)
    fn = lib.rl_stage_paint_build_topology_ex
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    rc = fn(b"/nonexistent", 0, 0, 0, C.byref(o))
    assert rc not in (0, RL_EINVAL), rc
    assert b"rl_stage_opts_init" not in lib.rl_last_error()


def run_cli(tmp_path, *args):
    return subprocess.run([CLI] + list(args), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_cli_accepts_paint_all_windows(tmp_path):
    p = run_cli(tmp_path, "--mode", "PaintBuildTopology", "--paint_all_windows", "--chunk_index", "0",
                "--first_section", "0", "--last_section", "0", "-o", "absent")
    err = p.stderr.decode()
    assert "does not exist" not in err and "Unexpected argument" not in err, err
    # (no chunk files here, or no device: the stage fails, after the options were taken)
    assert p.returncode == 1 and "Error: " in err, err


def test_cli_still_refuses_an_unknown_option(tmp_path):
    p = run_cli(tmp_path, "--mode", "PaintBuildTopology", "--paint_all_window", "--chunk_index", "0", "-o", "absent")
    assert p.returncode == 1
    assert p.stderr.decode().strip() == "Option 'paint_all_window' does not exist"  # cxxopts' message, as before
