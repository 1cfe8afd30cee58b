#!/usr/bin/env python3
"""tests/golden/optimize.npz: what the unmodified reference's `Relate --mode OptimizeParameters` writes for synthetic
inputs (tests/test_optimize_gpu.py compares the drop-in CLI against it, byte for byte).

Needs oracle/_ref/Relate (`make -C oracle ref`, build container only).  The inputs are the synthetic .haps / .sample /
.map of tests/test_makechunks.py write_synth_haps, regenerated from the seed by the test and md5-checked.  Per case:
  (a) the default grid (4 thetas x 5 recombination factors), (b) an --input file of 2 x 3 values;
each run TWICE, a few seconds apart, and the two .opt files must be identical: the mode seeds a generator from
time + pid that its code path never draws from (pipeline/OptimizeParameters.cpp:169, src/anc_builder.cpp:831), so the
counts must not depend on when the run happens -- if they ever do, this tool stops and the parity target of the test
has to change.
Stored: the .opt bytes, the listing of everything under the working directory after the run (the mode ends with the
reference's Clean), the chunk / section counts MakeChunks chose, the reference's wall-clock (one run each, labelled as
such).

Cases: N = 6 x L = 50,000 cut into 3 overlapping chunks of 3, 6 and 4 sections, and N = 136 with a short L (more than two
wavefronts of leaves and more than two 64-column panels for the device tree builder).
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_makechunks import write_synth_haps  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "Relate")
# name -> N, L, --memory
CASES = {"chunks": (6, 50000, "0.0005"), "wide": (136, 400, "0.002")}
INPUT_GRID = "0.0005 0.02\n0.5 2 20\n"


def listing(work):
    out = []
    for base, dirs, files in os.walk(work):
        for f in files + dirs:
            out.append(os.path.relpath(os.path.join(base, f), work))
    return sorted(out)


def run_ref(work, memory, name, extra):
    args = [REF, "--mode", "OptimizeParameters", "--haps", "s.haps", "--sample", "s.sample", "--map", "s.map",
            "--memory", memory, "-o", name] + extra
    t0 = time.time()
    subprocess.run(args, cwd=work, check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
    return time.time() - t0


def shape(work, memory):
    """chunks and sections per chunk, from the reference's own MakeChunks"""
    subprocess.run([REF, "--mode", "MakeChunks", "--haps", "s.haps", "--sample", "s.sample", "--map", "s.map",
                    "--memory", memory, "-o", "shape"], cwd=work, check=True, stderr=subprocess.DEVNULL)
    d = os.path.join(work, "shape")
    C = struct.unpack("<3i", open(os.path.join(d, "parameters.bin"), "rb").read(12))[2]
    W = [struct.unpack("<3i", open(os.path.join(d, "parameters_c%d.bin" % c), "rb").read(12))[2] - 1 for c in range(C)]
    subprocess.run([REF, "--mode", "Clean", "-o", "shape"], cwd=work, check=True, stderr=subprocess.DEVNULL)
    return C, W


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/Relate is not built: make -C oracle ref")
    out = {"input_grid": np.frombuffer(INPUT_GRID.encode(), dtype=np.uint8)}
    for tag, (N, L, memory) in CASES.items():
        with tempfile.TemporaryDirectory() as work:
            write_synth_haps(work, N, L, seed=N)
            out[tag + "/args"] = np.array([N, L], np.int64)
            out[tag + "/memory"] = np.array([float(memory)])
            for fn in ("s.haps", "s.sample", "s.map"):
                out["%s/in_md5/%s" % (tag, fn)] = np.frombuffer(
                    hashlib.md5(open(os.path.join(work, fn), "rb").read()).digest(), dtype=np.uint8)
            C, W = shape(work, memory)
            out[tag + "/sections"] = np.array(W, np.int64)
            open(os.path.join(work, "grid.txt"), "w").write(INPUT_GRID)
            for grid, extra in (("default", []), ("input", ["--input", "grid.txt"])):
                t1 = run_ref(work, memory, "job", extra)
                time.sleep(3)  # (another time(0), another pid: another seed)
                run_ref(work, memory, "again", extra)
                a = open(os.path.join(work, "job.opt"), "rb").read()
                b = open(os.path.join(work, "again.opt"), "rb").read()
                if a != b:
                    sys.exit("%s/%s: two runs of the reference wrote different .opt files -- the counts depend on the "
                             "seed; the fixture cannot be a parity target" % (tag, grid))
                os.remove(os.path.join(work, "again.opt"))
                left = [f for f in listing(work) if f != "grid.txt"]
                os.remove(os.path.join(work, "job.opt"))
                out["%s/%s/opt" % (tag, grid)] = np.frombuffer(a, dtype=np.uint8)
                out["%s/%s/left" % (tag, grid)] = np.frombuffer("\n".join(left).encode(), dtype=np.uint8)
                out["%s/%s/ref_seconds_one_run" % (tag, grid)] = np.array([t1])
                counts = [int(x.split()[2]) for x in a.decode().splitlines()]
                print("%s/%s: N=%d L=%d, %d chunks, sections %s: %d grid points, counts %d..%d, reference %.1f s, "
                      "two runs identical; left behind: %s" % (tag, grid, N, L, C, W, len(counts), min(counts),
                                                              max(counts), t1, left))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "optimize.npz"), **out)


if __name__ == "__main__":
    main()
