"""`Relate --mode OptimizeParameters` on the GPU against the unmodified reference binary: tests/golden/optimize.npz
(tools/make_golden_opt.py) holds the .opt file the reference wrote -- default grid and an --input grid, for a job of
3 chunks with 3, 6 and 4 sections (N = 6) and for N = 136 -- and what it left behind.  Every comparison is exact."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from relate_amd import api
from test_makechunks import write_synth_haps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")
Z = os.path.join(ROOT, "tests", "golden", "optimize.npz")
INPUT = ["--haps", "s.haps", "--sample", "s.sample", "--map", "s.map"]


def text(a):
    return a.tobytes().decode()


def inputs(work, z, tag):
    N, L = [int(x) for x in z[tag + "/args"]]
    write_synth_haps(work, N, L, seed=N)
    for fn in ("s.haps", "s.sample", "s.map"):
        assert hashlib.md5(open(os.path.join(work, fn), "rb").read()).digest() == z["%s/in_md5/%s" % (tag, fn)].tobytes(), fn
    open(os.path.join(work, "grid.txt"), "w").write(text(z["input_grid"]))
    return "%g" % float(z[tag + "/memory"][0])


def listing(work):
    out = []
    for base, dirs, files in os.walk(work):
        out += [os.path.relpath(os.path.join(base, f), work) for f in files + dirs]
    return sorted(f for f in out if f != "grid.txt")


def run_mode(work, memory, extra=(), env=None, name="job", log=None):
    p = subprocess.run([CLI, "--mode", "OptimizeParameters"] + INPUT + ["--memory", memory, "-o", name] + list(extra),
                       cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    if log is not None:
        log.append(p.stderr.decode())
    return open(os.path.join(work, name + ".opt"), "rb").read()


def counts_of(opt_bytes):
    return [int(line.split()[2]) for line in opt_bytes.decode().splitlines()]


@pytest.mark.parametrize("tag", ["wide", "chunks"])
@pytest.mark.parametrize("grid", ["input", "default"])
def test_cli_writes_the_reference_opt_file(tmp_path, tag, grid):
    z = np.load(Z)
    work = str(tmp_path)
    memory = inputs(work, z, tag)
    opt = run_mode(work, memory, ["--input", "grid.txt"] if grid == "input" else [])
    want = z["%s/%s/opt" % (tag, grid)].tobytes()
    assert opt == want, "\n" + opt.decode() + "\nreference:\n" + want.decode()
    assert listing(work) == text(z["%s/%s/left" % (tag, grid)]).split("\n")


def test_api_chunk_by_chunk_sums_to_the_opt_file(tmp_path):
    """api.optimize_parameters per chunk of a MakeChunks directory, summed over the chunks = the reference's counts
    (two of the six grid points of the --input fixture; the whole grids are the CLI test's)"""
    z = np.load(Z)
    work = str(tmp_path)
    memory = inputs(work, z, "chunks")
    p = subprocess.run([CLI, "--mode", "MakeChunks"] + INPUT + ["--memory", memory, "-o", "job"], cwd=work,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    lines = [ln.split() for ln in text(z["chunks/input/opt"]).splitlines()]  # 2 thetas x 3 factors
    thetas, factors = [float(lines[3][0])], [float(lines[4][1]), float(lines[5][1])]
    want = np.array([[int(lines[4][2]), int(lines[5][2])]])
    sections = [int(x) for x in z["chunks/sections"]]
    total = np.zeros((1, 2), np.int64)
    for c in range(len(sections)):
        assert api.num_sections(os.path.join(work, "job"), c) == sections[c]
        got = api.optimize_parameters(os.path.join(work, "job"), c, thetas, factors)
        assert got.shape == (1, 2) and got.dtype == np.int32
        total += got
    assert np.array_equal(total, want), (total, want)


def test_sections_one_by_one_sum_to_the_chunk(tmp_path):
    """rl_optimize_section over the sections of a painted context = the stage's count for the chunk (N = 136: one
    chunk, so also the reference's count of that grid point)"""
    z = np.load(Z)
    work = str(tmp_path)
    memory = inputs(work, z, "wide")
    p = subprocess.run([CLI, "--mode", "MakeChunks"] + INPUT + ["--memory", memory, "-o", "job"], cwd=work,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    lines = [ln.split() for ln in text(z["wide/input/opt"]).splitlines()]
    theta, factor, want = float(lines[4][0]), float(lines[4][1]), int(lines[4][2])
    ctx = api.Context(0)
    ctx.load_chunk(os.path.join(work, "job"), 0)
    ctx.paint(api.RL_SUM_EXACT)
    got = sum(ctx.optimize_section(s, theta, factor) for s in range(ctx.W))
    ctx.close()
    assert ctx.W == int(z["wide/sections"][0]) and got == want, (got, want)


def test_trees_on_the_host_and_on_the_device_count_the_same(tmp_path):
    z = np.load(Z)
    work = str(tmp_path)
    memory = inputs(work, z, "wide")
    want = z["wide/input/opt"].tobytes()
    N, L = [int(x) for x in z["wide/args"]]
    for build in ("0", "1"):
        log = []
        opt = run_mode(work, memory, ["--input", "grid.txt"], env={"RELATE_AMD_GPU_BUILD": build, "RELATE_AMD_TIMING": "1"},
                       name="build" + build, log=log)
        assert opt == want, "RELATE_AMD_GPU_BUILD=%s\n%s\nreference:\n%s" % (build, opt.decode(), want.decode())
        # ... and the trees were built where the switch says (the stage's own account, one line per chunk)
        m = re.findall(r"\[optimize\] chunk \d+: (\d+) grid points, (\d+) trees \((\d+) on the GPU, (\d+) on the host\)", log[0])
        assert len(m) == 1, log[0][-2000:]
        points, trees, on_gpu, on_host = [int(x) for x in m[0]]
        assert points == 6 and trees == 6 * L and on_gpu + on_host == trees
        if build == "0":
            assert on_gpu == 0
        else:  # (a tree may need the host's symmetric fallback, tree_builder.cpp:255-293: most do not)
            assert on_gpu > trees // 2, (on_gpu, on_host)


def numpy_cancel(d, carriers, log_ratio):
    """the loop of src/anc_builder.cpp:869-882 in float32, then the row minima off the diagonal"""
    d = d.copy()
    lr = np.float32(log_ratio)
    for i in np.flatnonzero(carriers):
        d[i, carriers == 0] += lr
        d[i] -= d[i].min()
    off = d.copy()
    np.fill_diagonal(off, np.inf)
    return d, off.min(axis=1)


@pytest.mark.parametrize("N", [5, 64, 65, 1000, 5120, 5121, 10240])
@pytest.mark.parametrize("who", ["none", "all", "one", "random"])
def test_cancel_rowmin_kernel_bitwise(N, who):
    rng = np.random.default_rng(1000 * N + ["none", "all", "one", "random"].index(who))
    d = (rng.random((N, N), dtype=np.float32) * np.float32(40.0)).astype(np.float32)
    np.fill_diagonal(d, 0.0)
    carriers = {"none": np.zeros(N, np.uint8), "all": np.ones(N, np.uint8),
                "one": (np.arange(N) == N // 2).astype(np.uint8),
                "random": (rng.random(N) < 0.3).astype(np.uint8)}[who]
    log_ratio = np.float32(np.log(0.001 / (1.0 - 0.001)))
    want_d, want_min = numpy_cancel(d, carriers, log_ratio)
    got_d, got_min = api.debug_cancel_rowmin(d, carriers, log_ratio)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(got_min.view(np.uint32), want_min.view(np.uint32))
    if who == "none":
        assert np.array_equal(got_d.view(np.uint32), d.view(np.uint32))


def test_fast_sum_mode_is_accepted(tmp_path):
    """--sum_mode lanes is not held to the reference: the counts come out, nothing more is claimed"""
    z = np.load(Z)
    work = str(tmp_path)
    memory = inputs(work, z, "wide")
    got = counts_of(run_mode(work, memory, ["--input", "grid.txt", "--sum_mode", "lanes"]))
    N, L = [int(x) for x in z["wide/args"]]
    assert len(got) == 6 and all(0 <= c <= L for c in got)
