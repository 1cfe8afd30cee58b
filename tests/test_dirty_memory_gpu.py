"""Every device entry point on dirty device memory.

The library takes device and pinned memory from its own block cache (relate_amd/csrc/context.cpp): a released block
comes back unchanged, with the previous owner's bytes in it, and nothing may rely on what a block holds.  The rest of
the GPU suite runs its steps in fresh processes, or on blocks that hold an earlier job's VALID data; here

  a. the premise is shown (a block comes back with what the last owner left in it) and so is the test hook
     RELATE_AMD_TEST_POISON=<byte>, which fills every block the caches hand out;
  b. every device entry point runs under the patterns 0xFF (NaN as a float or double, -1 as an int32, all-ones for an
     atomicMax table: sums, counters, flags, ranks) and 0x7F (3.4e38 / 1.4e306 / a large positive integer: running
     maxima, anything compared with `>`; fmax(NaN, x) = x hides a maximum from 0xFF);
  c. two modes follow each other in one process with the hook unset, as a caller that keeps the process dirties memory.

No expected value comes from a device run: the modes are held to their host twins (device=None), computed in this
process; files to the reference's bytes in tests/golden; the core to the golden fixtures and the oracle through the
helpers of the tests that hold it to them today.  Everything is compared bit for bit, RL_SUM_LANES32 too: with
test_lanes32_gpu.compare against RO_SUM_LANES32, the oracle's restatement of that order (and its floor over all targets).

Every step that uses the GPU is a child process under a time limit of its own (rlutil.gpu_step), and the hook reaches it
through the child's environment alone.  A child is this file, run as a script with the name of a step:
`python tests/test_dirty_memory_gpu.py <step> <folder>`."""
import os
import pathlib
import pickle
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
for _p in (TESTS, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest  # noqa: E402

import rlutil  # noqa: E402
from relate_amd import api  # noqa: E402
from rlutil import gpu_step  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "relate_amd", "Relate")
HOOK = "RELATE_AMD_TEST_POISON"
PATTERNS = {"ff": "0xFF", "7f": "0x7F"}
BOTH = pytest.mark.parametrize("pattern", sorted(PATTERNS))
PEEK_SIZES = (16, 4097, (1 << 20) + 3)
DIRT = 0xA5


def environment(pattern):
    """the child's environment: the hook set to the pattern, or (None) not set whatever this process has"""
    env = {k: v for k, v in os.environ.items() if k != HOOK}
    if pattern is not None:
        env[HOOK] = PATTERNS[pattern]
    return env


def step(name, tmp_path, pattern, seconds=120, extra=()):
    """one child of this file -> its output lines"""
    p = gpu_step([sys.executable, os.path.abspath(__file__), name, str(tmp_path)] + list(extra), seconds,
                 env=environment(pattern))
    assert p.returncode == 0, (p.stdout.decode()[-2000:], p.stderr.decode()[-3000:])
    return p.stdout.decode().splitlines()


def hook_is_live():
    """in a child: with the hook set, the block the cache hands out now holds the pattern and nothing else"""
    want = os.environ.get(HOOK)
    if want is not None:
        got = api.debug_alloc_peek(1000)
        assert len(got) >= 1000 and (got == int(want, 0)).all(), (want, np.unique(got))
    print("hook", want)


# --------------------------------------------------------------------------------------- a. the premise and the hook
def child_peek(tmp):
    fill = DIRT if os.environ.get(HOOK) is None else 0
    for n in PEEK_SIZES:
        first = api.debug_alloc_peek(n, fill=fill)
        second = api.debug_alloc_peek(n)
        print("peek", n, len(first), int(first.min()), int(first.max()), len(second), int(second.min()), int(second.max()))


def peeks(tmp_path, pattern):
    lines = [[int(x) for x in ln.split()[1:]] for ln in step("peek", tmp_path, pattern) if ln.startswith("peek")]
    assert [ln[0] for ln in lines] == list(PEEK_SIZES)
    for n, got1, _, _, got2, _, _ in lines:
        assert n <= got1 <= n + n // 8 + 4096 and got2 == got1  # the same block both times, all of it seen
    return lines


def test_the_cache_hands_back_a_dirty_block(tmp_path):
    """hook unset: what one owner wrote over a block is what the next owner of that block reads, over all its bytes"""
    for n, _, _, _, _, lo, hi in peeks(tmp_path, None):
        assert (lo, hi) == (DIRT, DIRT), (n, lo, hi)


@BOTH
def test_the_hook_poisons_fresh_and_reused_blocks(tmp_path, pattern):
    """hook set: a fresh block is all pattern over all the bytes the cache gave, and so is the same block after its
    owner zeroed it and gave it back"""
    byte = int(PATTERNS[pattern], 0)
    for n, _, lo1, hi1, _, lo2, hi2 in peeks(tmp_path, pattern):
        assert (lo1, hi1) == (byte, byte), ("fresh", n, lo1, hi1)
        assert (lo2, hi2) == (byte, byte), ("reused", n, lo2, hi2)


# ------------------------------------------------------------------------------------ b. the core, against its oracles
def sub(tmp, name):
    d = pathlib.Path(tmp) / name
    d.mkdir()
    return d


def child_wave_sum(tmp):
    """rl_debug_wave_sum_ex: one and two waves per array, 16 arrays back to back in one workgroup (the WaveLink slots
    are reused), three families of test_exact_sum_gpu, the terms plain and masked; all three orders against numpy"""
    import test_exact_sum_gpu as xs
    hook_is_live()
    for n in (999, 5121):
        rng = np.random.RandomState(3000 + n)
        families = [(name, x) for name, x in xs.cases(n, 16, rng) if name in ("ties", "leading zeros")]
        families += [(name, x) for name, x, _ in xs.seam_cases(n, 16, rng) if name == "tiny and subnormal"]
        assert len(families) == 3
        for masked in (False, True):
            for name, x in families:
                mis = rng.rand(*x.shape) < 0.3 if masked else None
                st = xs.check(x, rows_per_group=16, mismatch=mis, what=(n, name, masked))
                assert st["sums"] == 16 * (2 if n > 5120 else 1), st
                print("ok", n, name.replace(" ", "_"), masked)


def oracle_paint_files(ch, folder):
    import test_copying_gpu as tcg
    tcg.oracle_paint(ch, str(folder))
    return [open(os.path.join(str(folder), "relate_%d.bin" % w), "rb").read() for w in range(ch.W)]


def child_paint(tmp):
    """Context.paint in the exact, lanes and lanes32 orders, Context.stones, write_paint_files / write_paint_file /
    paint_record: example8 against the reference's paint files, every chunk's stones against the oracle's"""
    import test_edge_gpu as te
    import test_golden_gpu as tg
    import test_lanes32_gpu as tl
    from golden_util import Fixture
    hook_is_live()
    tg.test_paint_files_byte_identical_to_reference(sub(tmp, "golden"), "example8", None)
    print("ok example8 files")
    chunks = [("example8", Fixture("example8", sub(tmp, "fx")).chunk), ("synth65", rlutil.synth_chunk(65, 1200)),
              ("random5121", te.random_chunk(5121, 90, 0.15, seed=5121, wb=[0, 40, 90], special="flat_targets"))]
    for name, ch in chunks:
        te.check(ch, modes=("exact", "lanes"))
        print("ok", name, "stones")
        tl.compare(ch)
        print("ok", name, "lanes32")
    ch = chunks[1][1]
    want = oracle_paint_files(ch, sub(tmp, "oracle"))
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    ctx.paint(api.RL_SUM_EXACT)
    for w in range(ch.W):
        one = str(pathlib.Path(tmp) / ("one_%d.bin" % w))
        ctx.write_paint_file(w, one)
        assert open(one, "rb").read() == want[w], w
    ctx.close()
    print("ok synth65 files")


def bounded_window_against_oracle(ch, paint_file, ctx, w, share):
    """a window that keeps `share` of its posterior rows resident and repaints on demand: its matrices, SNP by SNP,
    against the oracle's -> RePaint launches"""
    import ctypes as C
    o = rlutil.oracle()
    d = ch.ro()
    s0, s1 = int(ch.wb[w]), int(ch.wb[w + 1]) - 1
    full = ctx.open_window(w, paint_file, s0, api.RL_SUM_EXACT)
    rows = sum(full.rows(n) for n in range(ch.N))
    full.close()
    part = ctx.open_window(w, paint_file, s0, api.RL_SUM_EXACT, max_rows=max(1, int(share * rows)))
    ow = o.ro_window_open(C.byref(d), paint_file.encode(), s0, 4)
    assert ow
    M = np.zeros((ch.N, ch.N), np.float32)
    every = max(1, (s1 - s0) // 12)
    for s in range(s0, s1 + 1):
        if s > s0:
            part.advance(s)
            o.ro_window_advance(C.c_void_p(ow), s)
        if (s - s0) % every == 0 or s == s1:
            o.ro_window_matrix(C.c_void_p(ow), s, M.ctypes.data_as(C.c_void_p))
            G = part.matrix(s)
            assert np.array_equal(G.view(np.uint32), M.view(np.uint32)), (w, s)
    repaints = part.repaints
    part.close()
    o.ro_window_free(C.c_void_p(ow))
    return repaints


def copying_against_the_restatement(ch, folder, ctx):
    """Window.copying window after window, and Context.copying_matrix over the chunk, against copying_cases"""
    import copying_cases as cc
    import test_copying_gpu as tcg
    got = tcg.check_all_windows(ch, str(folder), ctx)
    want = np.zeros((ch.N, ch.N), np.float64)
    for w in range(ch.W):
        ow = cc.OracleWindow(ch, os.path.join(str(folder), "relate_%d.bin" % w), w)
        cc.add_window(ow, want)
        ow.close()
    assert np.array_equal(cc.bits(got), cc.bits(want))
    ctx.paint(api.RL_SUM_EXACT)
    Cm, snps = ctx.copying_matrix()
    assert snps == ch.L and np.array_equal(cc.bits(Cm), cc.bits(want))


def child_window(tmp):
    """Window.matrix and Window.topology of whole windows, a bounded window, Window.copying and
    Context.copying_matrix: example8 against the reference's rows and matrices, example8 and N = 257 against the
    oracle and the restatement of copying_cases"""
    import test_copying_gpu as tcg
    import test_golden_gpu as tg
    import test_window_gpu as tw
    from golden_util import Fixture
    hook_is_live()
    tg.test_repaint_and_matrices_bit_identical_to_reference(sub(tmp, "golden"), "example8", None)
    print("ok example8 whole")
    fx = Fixture("example8", sub(tmp, "fx"))
    pdir = sub(tmp, "fxpaint")
    fx.write_paint_files(str(pdir))
    ctx = tg.open_ctx(fx)
    repaints = bounded_window_against_oracle(fx.chunk, os.path.join(str(pdir), "relate_1.bin"), ctx, 1, 0.1)
    assert repaints >= 2, repaints
    print("ok example8 bounded", repaints)
    copying_against_the_restatement(fx.chunk, pdir, ctx)
    ctx.close()
    print("ok example8 copying")
    ch = tcg.edge_chunk(257)
    tw.run_case(sub(tmp, "n257"), 257, ch.L, None, 5, chunk=ch, windows=[0])
    print("ok n257 whole")
    pdir = sub(tmp, "n257paint")
    oracle_paint_files(ch, pdir)
    ctx = api.Context()
    ctx.set_chunk(ch.seq, ch.r, ch.rpos, ch.wb)
    repaints = bounded_window_against_oracle(ch, os.path.join(str(pdir), "relate_1.bin"), ctx, 1, 0.1)
    assert repaints >= 2, repaints
    print("ok n257 bounded", repaints)
    copying_against_the_restatement(ch, pdir, ctx)
    ctx.close()
    print("ok n257 copying")


def child_builder(tmp):
    """Builder.build on the device: the adversarial sequences against the reference's trees on file, the same
    sequences and N = 65 with sample ages against the host builder, N = 65 without"""
    import builder_cases
    import test_builder_ages_gpu as ta
    import test_builder_golden as bg
    import test_builder_gpu as tb
    hook_is_live()
    for name in sorted(builder_cases.CASES):
        bg.test_device_builder_gives_the_reference_trees(name)
        print("ok", name, "reference")
        N, mats = builder_cases.CASES[name]()
        on_gpu = ta.run_sequence(N, ta.sample_ages(np.random.RandomState(N), N, 3), mats, all_on_gpu=False)
        assert on_gpu >= 1
        print("ok", name, "ages", on_gpu)
    N, mats = builder_cases.case_tied(65, seed=65)
    assert tb.run_sequence(65, mats) == len(mats)
    print("ok n65 plain")
    assert ta.run_sequence(65, ta.sample_ages(np.random.RandomState(65), 65, 3), mats) == len(mats)
    print("ok n65 ages")


def child_optimize_section(tmp):
    """Context.optimize_section over the sections of the chunk in sys.argv[3] for one grid point -> the count"""
    hook_is_live()
    ctx = api.Context(0)
    ctx.load_chunk(sys.argv[3], 0)
    ctx.paint(api.RL_SUM_EXACT)
    print("count", ctx.W, sum(ctx.optimize_section(s, float(sys.argv[4]), float(sys.argv[5])) for s in range(ctx.W)))
    ctx.close()


@BOTH
def test_wave_sum(tmp_path, pattern):
    """child_wave_sum: 2 sizes x 3 families x (plain, masked)"""
    lines = step("wave_sum", tmp_path, pattern)
    assert lines[0] == "hook " + PATTERNS[pattern] and len([ln for ln in lines if ln.startswith("ok ")]) == 12, lines


@BOTH
def test_paint_stones_and_paint_files(tmp_path, pattern):
    """child_paint: the files of example8 and of synth65, and (stones, lanes32) of three chunks"""
    lines = step("paint", tmp_path, pattern, 300)
    assert lines[0] == "hook " + PATTERNS[pattern] and len([ln for ln in lines if ln.startswith("ok ")]) == 8, lines


@BOTH
def test_windows_and_copying(tmp_path, pattern):
    """child_window: a whole window, a bounded one and the copying matrices, on example8 and at N = 257"""
    lines = step("window", tmp_path, pattern, 300)
    assert lines[0] == "hook " + PATTERNS[pattern] and len([ln for ln in lines if ln.startswith("ok ")]) == 6, lines


@BOTH
def test_builder_on_the_device(tmp_path, pattern):
    """child_builder: the four adversarial sequences without and with sample ages, N = 65 without and with"""
    lines = step("builder", tmp_path, pattern, 300)
    assert lines[0] == "hook " + PATTERNS[pattern] and len([ln for ln in lines if ln.startswith("ok ")]) == 10, lines


@BOTH
@pytest.mark.parametrize("name", ["example8", "synth70"])
def test_fused_stage_through_the_cli(tmp_path, pattern, name):
    """`Relate --mode PaintBuildTopology` with the trees built on the device: the bundled example data (two sections)
    and synth70 (sixteen, several of them open at a time): the reference's .anc and .mut"""
    from golden_util import Fixture
    work = tmp_path / "work"
    (work / "out").mkdir(parents=True)
    fx = Fixture(name, work / "out")
    p = gpu_step([CLI, "--mode", "PaintBuildTopology", "--chunk_index", "0", "-o", "out"], 300, cwd=str(work),
                 env=dict(environment(pattern), RELATE_AMD_GPU_BUILD="1", RELATE_AMD_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert sum(int(x) for x in re.findall(r"(\d+) trees on the GPU", p.stderr.decode())) > 0
    for w in range(fx.W):
        assert open(work / "out" / "chunk_0" / ("out_%d.mut" % w), "rb").read() == fx.z["mut/%d" % w].tobytes(), w
        assert open(work / "out" / "chunk_0" / ("out_%d.anc" % w), "rb").read() == fx.z["anc/%d" % w].tobytes(), w


@BOTH
def test_optimize_parameters(tmp_path, pattern):
    """the smaller case of optimize.npz (N = 136, one chunk of four sections): `Relate --mode OptimizeParameters` on
    the six grid points writes the reference's .opt; Context.optimize_section over the sections counts what the
    reference counted for one of them"""
    import test_optimize_gpu as og
    z = np.load(og.Z)
    work = str(tmp_path)
    memory = og.inputs(work, z, "wide")
    want = z["wide/input/opt"].tobytes()
    p = gpu_step([CLI, "--mode", "OptimizeParameters"] + og.INPUT + ["--memory", memory, "-o", "job", "--input", "grid.txt"],
                 600, cwd=work, env=dict(environment(pattern), RELATE_AMD_GPU_BUILD="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert open(os.path.join(work, "job.opt"), "rb").read() == want
    q = subprocess.run([CLI, "--mode", "MakeChunks"] + og.INPUT + ["--memory", memory, "-o", "chunks"], cwd=work,
                       stderr=subprocess.PIPE)  # (no GPU in this mode)
    assert q.returncode == 0, q.stderr.decode()
    theta, factor, count = want.decode().splitlines()[4].split()
    lines = step("optimize_section", tmp_path, pattern, 300, [os.path.join(work, "chunks"), theta, factor])
    assert lines == ["hook " + PATTERNS[pattern], "count %d %s" % (int(z["wide/sections"][0]), count)], lines


# -------------------------------------------------------------------------------- b. the modes, against their host twins
class Job:
    """one call of a mode: api.<fn>(*args, **kw, device=...); `take` picks what is compared of the result; refused:
    the tree the device must name in its refusal"""

    def __init__(self, label, fn, args, kw=None, take=None, refused=None):
        self.label, self.fn, self.args, self.kw, self.take, self.refused = label, fn, args, kw or {}, take, refused

    def run(self, device):
        out = getattr(api, self.fn)(*self.args, device=device, **self.kw)
        out = self.take(out, device) if self.take else out
        if isinstance(out, dict):
            out = [out[k] for k in sorted(out)]
        return [np.asarray(a) for a in (out if isinstance(out, (tuple, list)) else [out])]


def stacked(shapes, lengths):
    parents = np.stack(shapes)
    return parents, np.stack([lengths(p) for p in parents])


def jobs_compare():
    """CompareTopology at N = 2, 65 (one wavefront and a lane) and 130: every shape against every shape and an
    interchange, pairs that name a tree twice and a pair given twice"""
    import tree_cases as tc
    jobs = []
    for N in (2, 65, 130):
        rng = np.random.default_rng(N)
        A = np.stack(tc.shapes(N, rng))
        B = np.stack(tc.shapes(N, rng)[::-1] + ([tc.nni(A[3], rng)] if N >= 3 else []))
        pairs = [(i, j) for i in range(len(A)) for j in range(len(B))] + [(0, 0), (0, 0), (len(A) - 1, 0)]
        jobs.append(Job("N%d" % N, "compare_trees", (A, B, np.array(pairs, np.int32))))
    return jobs


def jobs_pairwise(sizes=(2, 65, 130), seed=100):
    import pairwise_cases as pc
    import tree_cases as tc
    jobs = []
    for N in sizes:
        rng = np.random.default_rng(seed + N)
        parents, bl = stacked(tc.shapes(N, rng), lambda p: pc.branch_lengths(N, rng))
        weights = [7, 1, 0, 1000003, 12, 5]
        jobs.append(Job("N%d size" % N, "pairwise_trees", (parents, weights, None, "size")))
        jobs.append(Job("N%d time" % N, "pairwise_trees", (parents, weights, bl, "time")))
    return jobs


def many_trees(N, ntrees, seed, random_tree, lengths):
    rng = np.random.default_rng(seed)
    base = [random_tree(N, rng) for _ in range(min(ntrees, 4))]
    parents = np.stack([base[k % len(base)] for k in range(ntrees)])
    return parents, np.stack([lengths(N, rng) for _ in range(ntrees)]), rng


def jobs_coalrate(cases=((2, 6), (65, 6), (1025, 6), (130, 2), (130, 64)), batches=True, seed=0):
    """N = 2, 65 and 1025 (the larger workgroups, three rows each) with six epochs, the fewest and the most epochs at
    N = 130, and one tree more than a batch at N = 4000: D waits on the device between the batches"""
    import coalrate_cases as cc
    import test_coalrate_cpu as hc
    jobs = []
    for N, E in cases:
        parents, bl, factors = hc.case(N, 1000 * N + E + seed)
        jobs.append(Job("N%d E%d" % (N, E), "coalrate_trees", (parents, bl, factors, hc.epochs_of(E))))
    if batches:
        N = 4000
        batch = api.coalrate_batch_trees(N)
        parents, bl, rng = many_trees(N, batch + 1, N, cc.random_tree, cc.dated_lengths)
        factors = rng.uniform(0.0, 9000.0, batch + 1).astype(np.float32)
        jobs.append(Job("N4000 batches", "coalrate_trees", (parents, bl, factors, hc.epochs_of(3))))
    return jobs


# the mixed job of jobs_frequency: tie-free trees and the fixture's tie trees, by their index there
MIXED_ORDER = [("free", 0), ("tie", 0), ("tie", 1), ("free", 1), ("free", 2), ("tie", 2), ("free", 3), ("tie", 3), ("tie", 4),
               ("free", 4)]
MIXED_TIE_TREES = [t for t, (kind, _) in enumerate(MIXED_ORDER) if kind == "tie"]


def frequency_take(host_trees):
    """(freq, lin, marks, root_time) over ALL rows, the unmarked ones and those the device left to the host walk
    included; and the trees the device handed to the host, which must be the tied ones and no other (a tree whose flag
    was not cleared would get the right rows from the host walk too)"""
    return lambda out, device: out[:4] + (out[4] if device is not None else host_trees,)


def jobs_frequency(first=True, mixed=True, batches=True, seed=0):
    """N = 66 with every branch of every tree; tie-free trees mixed with the fixture's tie trees (N = 16), whose rows
    the device leaves unwritten for the host walk; one tree more than a batch at the larger workgroup size"""
    import frequency_cases as fc
    import test_frequency_cpu as hf
    jobs = []
    if first:
        N = 66 if not seed else 130
        parents, bl, ep = hf.generated(N, 7 * N + seed, 31)
        st, sb = hf.all_branches(parents, 140, np.random.default_rng(N + seed))
        jobs.append(Job("N%d" % N, "frequency_trees", (parents, bl, st, sb, ep), take=frequency_take(0)))
    if mixed:
        fx = fc.fixture()
        free_p, free_b, ep = hf.generated(16, 5, 31)
        tie_p, tie_b = fx["tie/parents"].astype(np.int32), fx["tie/bl"].astype(np.float64)
        assert not any(fc.tie_free(p, b) for p, b in zip(tie_p, tie_b))
        order = MIXED_ORDER
        parents = np.stack([(free_p if kind == "free" else tie_p)[k] for kind, k in order])
        bl = np.stack([(free_b if kind == "free" else tie_b)[k] for kind, k in order])
        rows = fx["tie/rows"]  # (pos, dist, tree, branch, second branch or -2, flipped): what the reference walked
        st, sb = [], []
        for t, (kind, k) in enumerate(order):
            if kind == "free":
                br = list(range(-1, 2 * 16 - 1))
            else:
                br = [-1] + sorted(int(r[3]) for r in rows if r[2] == k and r[4] == -2 and not r[5] and 0 <= r[3] < 30) + [30]
            st += [t] * len(br)
            sb += br
        jobs.append(Job("mixed ties", "frequency_trees", (parents, bl, np.array(st, np.int32), np.array(sb, np.int32), ep),
                        take=frequency_take(len(MIXED_TIE_TREES))))
    if batches:
        N = 2049
        batch = api.frequency_batch_trees(N)
        rng = np.random.default_rng(N)
        base = np.stack(fc.shapes(N, rng, randoms=1))
        parents = base[np.arange(batch + 1) % len(base)]
        bl = np.stack([fc.clock_lengths(p, rng) for p in parents])
        st = np.repeat(np.arange(batch + 1), 2)[1:].astype(np.int32)
        sb = rng.integers(0, 2 * N - 2, len(st)).astype(np.int32)
        sb[-1], sb[-2] = 2 * N - 3, N - 1
        ep = np.concatenate(([0.0], np.exp(np.linspace(2.0, 5.0, 30)))).astype(np.float32)
        jobs.append(Job("N2049 batches", "frequency_trees", (parents, bl, st, sb, ep), take=frequency_take(0)))
    return jobs


TIE_EPOCHS = np.array([0, 100, 200, 300, 400, 800, 1000, 1200, 5000, 1e6], np.float64)


def tie_heavy(shapes, seed=300):
    """N = 300 with lengths from a small set, many of them 0 (test_mutrate_gpu.test_tie_heavy_trees)"""
    rng = np.random.default_rng(seed)
    parents = np.stack(shapes(300, rng, randoms=3))
    return parents, rng.choice(np.array([0.0, 0.0, 0.0, 100.0, 200.0, 400.0]), parents.shape), rng


def jobs_mutrate(sizes=(2, 130, 2049), rest=True, seed=0):
    import mutrate_cases as mc
    import test_mutrate_gpu as tm
    jobs = []
    for N in sizes:
        parents, bl = tm.dated(N, 7 * N + seed)
        jobs.append(Job("N%d" % N, "mutrate_trees", (parents, bl, mc.default_epochs())))
    if rest:
        parents, bl, _ = tie_heavy(mc.shapes)
        jobs.append(Job("N300 ties", "mutrate_trees", (parents, bl, TIE_EPOCHS)))
        N = 8
        batch = api.mutrate_batch_trees(N)
        rng = np.random.default_rng(N)
        base = np.stack(mc.shapes(N, rng, randoms=5))
        parents = base[np.arange(batch + 1) % len(base)]
        bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
        jobs.append(Job("N8 batches", "mutrate_trees", (parents, bl, mc.default_epochs())))
    return jobs


def jobs_coaltree(sizes=(2, 130, 2049), rest=True, seed=0):
    import coaltree_cases as ct
    import test_coaltree_gpu as tg
    jobs = []
    for N in sizes:
        parents, bl, f = tg.dated(N, 7 * N + seed)
        jobs.append(Job("N%d" % N, "coaltree_trees", (parents, bl, f, ct.default_epochs(), 4)))  # (two blocks)
    if rest:
        parents, bl, rng = tie_heavy(ct.shapes)
        jobs.append(Job("N300 ties", "coaltree_trees", (parents, bl, tg.factors_for(len(parents), rng), TIE_EPOCHS, 4)))
        N = 24
        batch = api.coaltree_batch_trees(N)
        rng = np.random.default_rng(N)
        base = np.stack(ct.shapes(N, rng, randoms=5))
        parents = base[np.arange(batch + 1) % len(base)]
        bl = np.exp(rng.uniform(0.0, 14.0, parents.shape)).astype(np.float32).astype(np.float64)
        # (blocks of 5000: the second block takes its trees from both launches, through the accumulators on the device)
        jobs.append(Job("N24 batches", "coaltree_trees", (parents, bl, tg.factors_for(batch + 1, rng), ct.default_epochs(), 5000)))
    return jobs


def jobs_subtrees(big=True, seed=0):
    import test_subtrees_gpu as ts
    N = 130
    parents, bl, rng = ts.trees_at(N, 11 * N + seed)
    subsets = [np.array([0, 1], np.int32), np.arange(N, dtype=np.int32), np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)]
    jobs = [Job("N130 M%d" % len(s), "subtrees_trees", (parents, bl, s)) for s in subsets]
    if big:
        N = 2049
        parents, bl, rng = ts.trees_at(N, 11 * N, randoms=1)
        jobs.append(Job("N2049", "subtrees_trees", (parents, bl, np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32))))
    return jobs


def mutctx_take(out, device):
    return out[:2]  # (opportunity, root times); the third entry is seconds


def jobs_mutctx(first=True, batches=True, seed=0):
    """the jobs of test_mutctx_gpu.test_device_equals_host_twin with trees of their own in every job, and its
    two-batch job at N = 4000, whose accumulators persist from the first batch to the second"""
    import mutrate_cases as mc
    import test_mutctx_cpu as hx
    import test_mutctx_gpu as tx
    D = api.MUTCTX_DEPTH
    jobs = []
    if first:
        for E in ((2, 31, 64) if not seed else (31,)):
            rng = np.random.default_rng(E + seed)
            ep = mc.default_epochs() if E == 31 else np.concatenate(([0.0], np.exp(np.linspace(2.0, 15.0, E - 1))))
            for S in (0, 1, D - 1, D, D + 1, 2 * D + 1):
                N = 12 if not seed else 130
                parents, bl = hx.small_trees(N, 5, 1000 * E + S + seed)
                jobs.append(Job("E%d S%d" % (E, S), "mutctx_trees", (parents, bl) + tx.snps_on(5, S, rng) + (ep,),
                                {"details": True}, mutctx_take))
    if batches:
        N = 4000
        batch = api.mutrate_batch_trees(N)
        parents, bl = tx.big_trees(N, batch + 2, N)
        _, counts = tx.snps_on(1, 3 * D + 5, np.random.default_rng(1))
        tree = np.array([batch - 1] * (2 * D + 2) + [batch] * 2 + [batch + 1] * (D + 1), np.int32)
        jobs.append(Job("N4000 batches", "mutctx_trees", (parents, bl, tree, counts, mc.default_epochs()), {"details": True},
                        mutctx_take))
    return jobs


def jobs_refusal(mode):
    """a negative branch length in the second tree of the SECOND batch, then a correct small call"""
    import coalrate_cases as cc
    import test_coalrate_cpu as hc
    import test_mutctx_gpu as tx
    N = 4000 if mode != "frequency" else 2049
    batch = getattr(api, ("mutrate" if mode == "mutctx" else mode) + "_batch_trees")(N)
    parents, bl, rng = many_trees(N, batch + 2, 7 + N, cc.random_tree, cc.dated_lengths)
    if mode == "frequency":  # (tie-free at any N: no tree before the bad one goes to the host walk)
        import frequency_cases as fc
        bl = np.stack([fc.clock_lengths(p, rng) for p in parents])
    bl[batch + 1, 4] = -0.5
    T = batch + 2
    if mode == "coalrate":
        bad = (parents, bl, np.ones(T, np.float32), hc.epochs_of(3))
        good = jobs_coalrate(((65, 6),), batches=False, seed=1)
    elif mode == "frequency":
        bad = (parents, bl, np.arange(T, dtype=np.int32), np.full(T, 5, np.int32), hc.epochs_of(31))
        good = jobs_frequency(mixed=False, batches=False, seed=1)
    elif mode == "mutrate":
        bad = (parents, bl, TIE_EPOCHS)
        good = jobs_mutrate((130,), rest=False, seed=1)
    elif mode == "coaltree":
        bad = (parents, bl, np.ones(T, np.float32), TIE_EPOCHS, 50)
        good = jobs_coaltree((130,), rest=False, seed=1)
    elif mode == "subtrees":
        bad = (parents, bl, np.arange(0, N, 2, dtype=np.int32))
        good = jobs_subtrees(big=False, seed=1)[2:]
    else:
        tree, counts = tx.snps_on(T, api.MUTCTX_DEPTH + 1, rng)
        bad = (parents, bl, tree, counts, TIE_EPOCHS)
        good = jobs_mutctx(batches=False, seed=1)[3:4]
    return [Job("refused", mode + "_trees", bad, refused=batch + 1)] + good


def jobs_two_modes():
    """c. what a caller that keeps the process does: one mode after another, each on trees of its own, and the same
    modes backwards on other trees again"""
    def round_of(seed):
        return [jobs_coalrate(((1025, 6),), batches=False, seed=seed)[0], jobs_mutctx(batches=False, seed=seed + 1)[3],
                jobs_frequency(mixed=False, batches=False, seed=seed + 1)[0], jobs_subtrees(big=False, seed=seed)[2],
                jobs_coaltree((130,), rest=False, seed=seed)[0], jobs_mutrate((130,), rest=False, seed=seed)[0],
                jobs_pairwise((130,), seed=seed)[1]]
    return round_of(10) + round_of(20)[::-1]


MODES = {"compare": jobs_compare, "pairwise": jobs_pairwise, "coalrate": jobs_coalrate, "frequency": jobs_frequency,
         "mutrate": jobs_mutrate, "coaltree": jobs_coaltree, "subtrees": jobs_subtrees, "mutctx": jobs_mutctx}
REFUSALS = ("coalrate", "frequency", "mutrate", "coaltree", "subtrees", "mutctx")


def jobs_of(name):
    if name == "two_modes":
        return jobs_two_modes()
    if name.startswith("refusal_"):
        return jobs_refusal(name[len("refusal_"):])
    return MODES[name]()


def child_jobs(tmp):
    """the jobs of sys.argv[3] on the device, in order, in this one process -> results.pickle"""
    hook_is_live()
    results = []
    for job in jobs_of(sys.argv[3]):
        try:
            results.append(job.run(0))
            print("done", job.label)
        except api.RelateError as e:
            results.append(str(e))
            print("refused", job.label)
    with open(os.path.join(str(tmp), "results.pickle"), "wb") as f:
        pickle.dump(results, f, protocol=4)


def check_jobs(name, tmp_path, pattern, seconds=300):
    """every job of `name`: what the device gave in the child, bit for bit what the host twin gives here"""
    jobs = jobs_of(name)
    lines = step("jobs", tmp_path, pattern, seconds, [name])
    assert lines[0] == "hook " + (PATTERNS[pattern] if pattern else "None"), lines[:1]
    with open(str(tmp_path / "results.pickle"), "rb") as f:
        results = pickle.load(f)
    assert len(results) == len(jobs)
    for job, got in zip(jobs, results):
        if job.refused is not None:
            assert isinstance(got, str) and "tree %d" % job.refused in got and "negative" in got, (name, job.label, got)
            continue
        assert not isinstance(got, str), (name, job.label, got)
        want = job.run(None)
        assert len(got) == len(want), (name, job.label)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, job.label, k, g.dtype, w.dtype, g.shape, w.shape)
            gb, wb = np.frombuffer(g.tobytes(), np.uint8), np.frombuffer(w.tobytes(), np.uint8)
            assert np.array_equal(gb, wb), (name, job.label, "output %d" % k, "%d bytes differ" % int((gb != wb).sum()))
    return jobs, results


@BOTH
@pytest.mark.parametrize("mode", sorted(MODES))
def test_mode_equals_its_host_twin(tmp_path, pattern, mode):
    jobs, results = check_jobs(mode, tmp_path, pattern)
    if mode == "frequency":  # the rows of the tie trees are in the comparison, and none of them is all zero
        mixed = [j for j in jobs if j.label == "mixed ties"][0]
        _, lin, marks, _, _ = mixed.run(None)
        rows = marks & np.isin(mixed.args[2], MIXED_TIE_TREES)
        assert rows.sum() >= len(MIXED_TIE_TREES) and lin[rows].any(axis=1).all()


@BOTH
@pytest.mark.parametrize("mode", REFUSALS)
def test_a_refusal_in_the_second_batch_and_then_a_correct_call(tmp_path, pattern, mode):
    check_jobs("refusal_" + mode, tmp_path, pattern)


def test_two_modes_in_one_process_with_the_hook_unset(tmp_path):
    check_jobs("two_modes", tmp_path, None)


# ------------------------------------------------------------------- b. the file-writing modes through the command line
def cli_case(mode, tmp_path, run):
    if mode == "coalrate":
        import coalrate_cases as cases
        import test_coalrate_cpu as host
        return host.run_cli(cases.fixture(), tmp_path, 0, run=run)
    cases = __import__(mode + "_cases")
    host = __import__("test_%s_cpu" % mode)
    return host.run_cli(cases.fixture(), tmp_path, "a", 0, run=run)


@BOTH
@pytest.mark.parametrize("mode", REFUSALS)
def test_fixture_case_through_the_cli_on_the_device(tmp_path, pattern, mode):
    """case `a` of every file-writing mode with `--device 0`: the reference's bytes"""
    ran = []

    def run(cmd, cwd):
        ran.append(cmd)
        return gpu_step(cmd, 120, cwd=cwd, env=environment(pattern))
    cli_case(mode, tmp_path, run)
    assert ran and "--device" in ran[0]


CHILDREN = {"peek": child_peek, "wave_sum": child_wave_sum, "paint": child_paint, "window": child_window,
            "builder": child_builder, "optimize_section": child_optimize_section, "jobs": child_jobs}

if __name__ == "__main__":
    CHILDREN[sys.argv[1]](sys.argv[2])
