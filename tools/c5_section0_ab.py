#!/usr/bin/env python3
"""BASELINE.json config #5 (synthetic N = 10,000 x L = 200,000, seed 1, 327 windows), `Relate --mode PaintBuildTopology`
of section 0 alone with the trees on the device, once per executable given, on the same chunk files -- builds A/B:

    python tools/c5_section0_ab.py [name=path/to/Relate ...] [out.json]      (default: this=relate_amd/Relate)

-> per executable: wall-clock, the stage's own timing lines, whether out_0.anc is the reference's
(tests/golden/c5_first.npz).  profiles/window_range.json."""
import ctypes as C, hashlib, json, os, subprocess, sys, tempfile, time, shutil
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from relate_amd import api
z = np.load(os.path.join(ROOT, "tests", "golden", "c5_first.npz"))
N, L, W, seed = [int(x) for x in z["meta"]]
lib = api.lib()
seq = np.zeros((L, N), dtype=np.uint8); bp = np.zeros(L, dtype=np.int32); r = np.zeros(L); rpos = np.zeros(L + 1)
assert lib.rl_synth_panel(N, L, C.c_uint64(seed), 100, 1, seq.ctypes.data_as(C.c_void_p), None, 0, bp.ctypes.data_as(C.c_void_p),
                          r.ctypes.data_as(C.c_void_p), rpos.ctypes.data_as(C.c_void_p)) == 0
wb = np.zeros(L + 2, dtype=np.int32); wb[:W + 1] = z["wb"]
work = tempfile.mkdtemp(); d = os.path.join(work, "out"); os.makedirs(d)
lib.rl_write_chunk_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
assert lib.rl_write_chunk_files(d.encode(), 0, N, L, seq.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                rpos.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p), W) == 0
del seq
out = {"N": N, "L": L, "W": W, "command": "Relate --mode PaintBuildTopology --chunk_index 0 --first_section 0 --last_section 0 -o out (RELATE_AMD_TIMING=1 RELATE_AMD_GPU_BUILD=1)"}
builds = [a.split("=", 1) for a in sys.argv[1:] if "=" in a] or [["this", os.path.join(ROOT, "relate_amd", "Relate")]]
dest = [a for a in sys.argv[1:] if "=" not in a]
for name, exe in builds:
    exe = os.path.abspath(exe)
    shutil.rmtree(os.path.join(d, "chunk_0"), ignore_errors=True)
    t0 = time.time()
    p = subprocess.run([exe, "--mode", "PaintBuildTopology", "--chunk_index", "0", "--first_section", "0", "--last_section", "0", "-o", "out"],
                       cwd=work, stderr=subprocess.PIPE, timeout=500, env=dict(os.environ, RELATE_AMD_TIMING="1", RELATE_AMD_GPU_BUILD="1"))
    wall = time.time() - t0
    err = p.stderr.decode().replace("\r", "\n")
    res = {"rc": p.returncode, "wall_s": round(wall, 2),
           "lines": [l.strip() for l in err.split("\n") if l.startswith("[fused stage]") or l.startswith("[stage]") or l.startswith("[tree sequence]")]}
    anc = os.path.join(d, "chunk_0", "out_0.anc")
    if os.path.exists(anc):
        res["anc_md5_is_the_references"] = hashlib.md5(open(anc, "rb").read()).digest() == z["s0/anc_md5"].tobytes()
    if p.returncode != 0:
        res["stderr_tail"] = err[-600:]
    out[name] = res
    print(json.dumps({name: res}), flush=True)
    if p.returncode != 0:
        break
shutil.rmtree(work, ignore_errors=True)
if dest:
    json.dump(out, open(dest[0], "w"), indent=1)
