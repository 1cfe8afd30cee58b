"""The families of tests/builder_cases.py on the HOST builder alone: every census figure a family is there for
(rl_builder_census), where stays_on_device puts every tree, and -- for the golden families -- the reference's parent
arrays (tests/golden/builder_lists.npz, the unmodified reference's MinMatch through oracle/ref_harness
quickbuild_seq; `python tools/make_golden.py builder`).  A case that stops crossing the edge it is there for fails
here, on any machine, not silently on the GPU.  With up to 513 rebuilt clusters in a merge the golden families also
hold the host builder's own overflow path (more than MAX_GATHER = 32 rebuilt: phase 2 visits every later cluster,
minmatch.cpp) to the reference."""
import os

import numpy as np
import pytest

import builder_cases as bc
from relate_amd import api

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builder_lists.npz"))
# (N = 10,240 -- 7 s of matrices and 9 s of host build, no figure of its own -- is built once, in
#  test_builder_lists_gpu.py, where the same census is taken and the same prediction made; a family under a switch has
#  its twin's matrices and figures, the one without a pool of symmetric matrices another prediction)
HERE = [f for f in bc.FAMILIES if (f.N <= 5120 and f.name not in bc.TWINS) or f.sym_slots == 0]
# where the device builder is predicted to build the trees of a family (0: the host's), family by family
PLACES = {"S_G515_N700": [0, 0, 1], "P_G113_N736": [0, 0, 1], "P_flat_N1300": [1, 0, 1], "L_N700_H350_no_pool": [0, 1],
          "T_tied_N2048": [0, 0, 1]}


def host_census(f):
    b = api.Builder(f.N)
    ages = f.sample_ages()
    if ages is not None:
        b.set_sample_ages(ages)
    out = []
    for d, prior in f.make():
        parent = b.build(d, prior)[0]
        out.append((parent, b.census()))
    b.close()
    return out


@pytest.mark.parametrize("name", [f.name for f in HERE])
def test_family_census_and_place(name):
    f = next(x for x in bc.FAMILIES if x.name == name)
    built = host_census(f)
    assert len(built) == len(f.want)
    for t, (parent, census) in enumerate(built):
        assert not bc.check_census(census, f.want[t]), (name, t, census)
        if f.golden:
            assert np.array_equal(parent, GOLD[name][t]), (name, t, int(np.argmax(parent != GOLD[name][t])))
    places = [int(bc.stays_on_device(c, f.N, f.ages is not None, f.sym_slots)) for _, c in built]
    assert places == PLACES.get(name, [1] * len(built)), (name, places)


def test_golden_families_are_all_on_file():
    assert sorted(GOLD.files) == sorted(f.name for f in bc.FAMILIES if f.golden)
    assert max(f.N for f in bc.FAMILIES if f.golden) <= 900


def test_pair_list_edge_is_one_leaf_wide():
    """C(112, 2) - MM_PAIRS_LDS = 8 x 737: the star of 113 with a feasible interior fills the global pair list of a tree
    of 737 leaves to its last entry and has one pair too many for a tree of 736"""
    draws = 112 * 111 // 2
    assert draws - bc.MM_PAIRS_LDS == bc.pair_cap(737, False) and draws - bc.MM_PAIRS_LDS > bc.pair_cap(736, False)
    assert 26 * 25 // 2 == bc.MM_PAIRS_LDS + 5


def test_stays_on_device_is_the_three_conditions():
    c = dict(max_rebuilt=512, max_draws=8 * 700 + 320, first_sym_merge=-1)
    assert bc.stays_on_device(c, 700)
    assert not bc.stays_on_device(dict(c, max_rebuilt=513), 700)
    assert bc.stays_on_device(dict(c, max_rebuilt=513), 700, ages=True)
    assert not bc.stays_on_device(dict(c, max_draws=8 * 700 + 321), 700)
    assert bc.stays_on_device(dict(c, max_draws=32 * 700 + 320), 700, ages=True)
    assert not bc.stays_on_device(dict(c, max_draws=32 * 700 + 321), 700, ages=True)
    assert bc.stays_on_device(dict(c, first_sym_merge=5), 700)
    assert not bc.stays_on_device(dict(c, first_sym_merge=5), 700, sym_slots=0)


def test_census_of_the_older_inputs():
    """what the inputs of test_builder_gpu.py ask of the lists: the tied matrices fit them at every N that file builds
    (a row has more partners than MM_HITS from N = 260 on: the kernel scans such rows itself), the circulant ones start
    the symmetric fallback at merge 0"""
    for N, seed in ((130, 3), (260, 4), (1100, 5)):
        rng = np.random.RandomState(seed)
        b = api.Builder(N)
        b.build(bc.tied_matrix(rng, N))
        c = b.census()
        b.close()
        assert bc.stays_on_device(c, N) and c["max_rebuilt"] <= bc.MM_UPD_LDS and c["first_sym_merge"] == -1, (N, c)
        assert (c["max_partners"] > bc.MM_HITS) == (N >= 260), (N, c)
    N = 700
    idx = np.arange(N)
    circ = (((idx[None, :] - idx[:, None]) % N) * 10.0).astype(np.float32)
    b = api.Builder(N)
    b.build(circ)
    c = b.census()
    b.close()
    assert c["first_sym_merge"] == 0 and c["sym_merges"] >= 1 and c["max_rebuilt"] == 1, c


def test_census_refuses_bad_arguments_and_is_reset_per_build():
    import ctypes as C
    lib = api.lib()
    lib.rl_builder_census.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    out = np.full(9, 7, np.int64)
    assert lib.rl_builder_census(None, out.ctypes.data_as(C.c_void_p), 9) == -1  # RL_EINVAL
    assert lib.rl_last_error().decode().startswith("rl_builder_census:") and (out == 7).all()
    b = api.Builder(8)
    assert b.census() == dict(zip(api.Builder.CENSUS, (0, 0, 0, 0, 0, 0, 0, -1, 0)))  # (no tree yet)
    rng = np.random.RandomState(1)
    b.build(bc.tied_matrix(rng, 8))
    first = b.census()
    assert first["init_draws"] >= 1
    idx = np.arange(8)
    b.build((((idx[None, :] - idx[:, None]) % 8) * 10.0).astype(np.float32))
    assert b.census()["first_sym_merge"] == 0
    b.build(bc.tied_matrix(np.random.RandomState(1), 8))
    assert b.census()["first_sym_merge"] == -1  # (not carried over; the draws of a tree depend on carried state)
    b.close()
