"""The stage's sizing against HBM (relate_amd/csrc/stage_plan.h plan_sections, through rl_debug_stage_plan) holds the
decisions of the code it was cut from.

tests/golden/stage_plan_parent.json is NOT made by the code under test: the sizing block of build_sections as it stood
before the split (treeseq.cpp:949-1049 and :1140-1146 of commit 02698c3) was copied verbatim into a stand-alone C++
program -- its knobs, `room` and `known` plain parameters, the device calls stubs -- and run over a grid; the file is
that program's output.  Every output field of every row has to come back exactly: the same integer and double
operations in the same order.

The grid: the shapes of C3 (N = 5000, S = 80, 267 sections, 1,004,402 rows at most), of a C4 chunk (N = 2000, 235
sections, 126,716 rows), of C5 on one GPU (N = nloc = 10,000, two waves, 327 sections, 634,777 rows), of C5 sharded
by target (nloc = 2500 < N) and of the fixture synth70; free HBM from 0.02 GB ("one section barely fits") to 280 GB
(everything fits whole at synth70; C4 whole in two waves; C3 and C5 never fit whole) and unknown; rows per window by
hand (positive, negative, zero from the environment); window_parts 1, 4, 32; section threads set (8, 500, 0 from the environment) and unset; a single section and a range;
one and two RePaint lanes; device and host builder (16, 96, 256 host threads); stones per window (from paint files,
or parked in host memory) and not.

Rows that reproduce recorded runs:
  * C3, fused stage, defaults, 240 - 280 GB free (room = 0.9 x that): 134 section threads, 134 open at once -- the two
    waves of 134 of DESIGN.md 6 (the run had ~235 GB free after 53 GB of stones: room 211 GB gives 134 as well, 220 GB
    free (room 198 GB) falls to three waves of 89).
  * C5 on one GPU (profiles/r06_c5_job_one_gpu.json: 43 threads, 30,064 = 3 * 10,000 + 64 rows kept): every C5 row
    with bounded windows keeps 30,064 rows from 22 parts on; 43 threads is NOT a row of the grid -- with the stones
    parked in host memory (8 N nloc B more per window) it needs room in [235.7, 238.9] GB, without in [199.2, 203.7] GB
    (221 - 226 GB free), and the grid's neighbours give 41 (220 GB free; 260 GB free with the stones parked) and 46
    (240 GB free); see test_c5_recorded_run.
"""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "stage_plan_parent.json")))
OUTPUTS = GOLDEN["columns"][15:]  # (a row of the file: shape, the 14 inputs, the 12 outputs)
GOLDEN["rows"] = [dict(zip(GOLDEN["columns"][:15], row[:15]), out=dict(zip(OUTPUTS, row[15:]))) for row in GOLDEN["rows"]]
INPUTS = ("first_section", "last_section", "stones_per_window", "gpu_build", "room_known", "room", "host_threads",
          "window_rows_set", "window_rows", "window_parts", "section_threads_set", "section_threads", "repaint_lanes", "probe")


def plan(row):
    from relate_amd import api
    sh = GOLDEN["shapes"][row["shape"]]
    return api.debug_stage_plan(sh["N"], sh["nloc"], sh["S"], sh["waves"], sh["rows_of"], *[row[k] for k in INPUTS])


@pytest.mark.parametrize("shape", sorted(GOLDEN["shapes"]))
def test_plan_reproduces_the_parents_decisions(shape):
    rows = [r for r in GOLDEN["rows"] if r["shape"] == shape]
    assert len(rows) > 50
    for i, row in enumerate(rows):
        got = plan(row)
        assert set(got) == set(row["out"])
        for k, want in row["out"].items():
            # (the file's doubles are written with 17 significant digits: they read back as the same double)
            assert got[k] == want, (shape, i, k, got[k], want, row)


def test_grid_reaches_every_branch():
    rows = GOLDEN["rows"]
    outs = [r["out"] for r in rows]
    assert any(not r["room_known"] for r in rows)
    assert any(o["cap_rows"] == 0 for o in outs) and any(o["cap_rows"] > 0 for o in outs)  # whole and bounded windows
    assert any(r["window_rows_set"] and r["window_rows"] < 0 for r in rows)
    assert any(r["window_rows_set"] and r["window_rows"] > 0 for r in rows)
    assert {1, 4, 32} <= {r["window_parts"] for r in rows}
    assert any(o["wants_second_lane"] for o in outs)
    assert any(r["repaint_lanes"] == 2 and not r["out"]["wants_second_lane"] for r in rows)  # asked for, windows whole
    assert any(r["first_section"] == r["last_section"] for r in rows)
    assert {0, 1} == {r["gpu_build"] for r in rows} == {r["stones_per_window"] for r in rows}
    assert any(o["nthreads"] == 1 and o["cap_rows"] > 0 for o in outs)  # one section barely fits
    # one, two, three and more waves of sections: C4's 235 sections at once and in halves; C3's 267 in halves and
    # thirds (one wave of 267 is past the 256 section threads of a device build)
    threads = {s: {r["out"]["nthreads"] for r in rows if r["shape"] == s and not r["section_threads_set"]} for s in ("C3", "C4")}
    assert {235, 118} <= threads["C4"] and {134, 89} <= threads["C3"] and min(threads["C3"]) == 1
    # everything fits whole: all 16 sections of synth70, C4's 235 in two waves of whole windows
    assert any(r["shape"] == "synth70" and r["out"]["nthreads"] == 16 and r["out"]["cap_rows"] == 0 and r["room_known"]
               for r in rows)
    assert any(r["shape"] == "C4" and r["out"]["nthreads"] == 118 and r["out"]["cap_rows"] == 0 and r["room_known"]
               and not r["window_rows_set"] for r in rows)
    # the floor of 3 nloc + 64 rows and a cap above it
    c5 = {r["out"]["cap_rows"] for r in rows if r["shape"] == "C5" and not r["window_rows_set"]}
    assert 30064 in c5 and max(c5) > 30064


def test_c3_recorded_run():
    """C3's 267 sections go in two waves of 134, all of them open at once"""
    rows = [r for r in GOLDEN["rows"] if r["shape"] == "C3" and r["room_known"] and r["room"] in (0.9 * 240e9, 0.9 * 260e9)
            and not r["window_rows_set"] and not r["section_threads_set"] and r["window_parts"] == 32 and r["gpu_build"]
            and r["last_section"] - r["first_section"] == 266]
    assert len(rows) >= 4
    for r in rows:
        assert (r["out"]["nthreads"], r["out"]["concurrent"]) == (134, 134)
        assert r["out"]["cap_rows"] >= 3 * 5000 + 64
    sh = GOLDEN["shapes"]["C3"]
    from relate_amd import api
    got = api.debug_stage_plan(5000, 5000, 80, 1, sh["rows_of"], 0, 266, 0, 1, 1, 0.9 * 235e9, 256, 0, 0, 32, 0, 0, 1, 0)
    assert (got["nthreads"], got["concurrent"]) == (134, 134)


def test_c5_recorded_run():
    """profiles/r06_c5_job_one_gpu.json: 43 threads, 30,064 rows kept -- eight waves of 327 sections"""
    sh = GOLDEN["shapes"]["C5"]
    from relate_amd import api
    for stones, room in ((1, 237e9), (0, 201e9)):
        got = api.debug_stage_plan(10000, 10000, 80, 2, sh["rows_of"], 0, 326, stones, 1, 1, room, 256, 0, 0, 32, 0, 0, 1, 0)
        assert (got["nthreads"], got["concurrent"], got["cap_rows"]) == (43, 43, 30064)
