"""The device tree builder (minmatch_build.h, minmatch_worker.hip, minmatch_builder.hip) against the host builder at
every kernel and list edge -- the families of tests/builder_cases.py: the rebuilt list's tail in global memory and
its hand-off at MM_UPD_MAX (S), the pair list in global memory and its hand-off at the pair cap (P), a symmetric
fallback that starts after erasures have moved the live list (L), sizes at which every register slot of every thread
is taken (T), the AGES build on both sides of its layouts' edge, with a rebuilt list beyond 512 and with bucketed
merges (A).  Tree by tree: the host builder's parent and child arrays, the reference's parents for the golden families
(tests/golden/builder_lists.npz), the place of construction predicted from the host builder's census
(builder_cases.stays_on_device: an equality, not a bound), and the worker kernel rl_debug_builder_kind reports for
the size.  RELATE_AMD_BUILD_OCC and RELATE_AMD_TEST_SYM_SLOTS are read once per process: the families with such a
switch are built in a fresh child process."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import builder_cases as bc
from relate_amd import api

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(TESTS, "golden", "builder_lists.npz"))
# (a child's family is the twin of one without a switch: the reference's parents of that one, where on file)
CHILD = ("import sys, json; sys.path[:0] = [%r, %r]; import numpy as np; import builder_cases as bc; "
         "import test_builder_lists_gpu as tl; gold = np.load(%r); twin = bc.TWINS.get(sys.argv[1]); "
         "print('FAMILY ' + json.dumps(tl.check_family(sys.argv[1], gold[twin] if twin in gold.files else None)))"
         % (os.path.dirname(TESTS), TESTS, os.path.join(TESTS, "golden", "builder_lists.npz")))


def check_family(name, gold=None, device=0):
    """One family on the device builder, tree by tree (needs a GPU; in the process whose switches are f.env's): the host
    builder's parent and child arrays, the reference's parents where they are on file, the place of construction
    stays_on_device predicts from the host's census -- an equality --, a tree of the device's behind the last hand-off,
    and the worker kernel the family names.  -> per tree (built on the device, seconds of the device build)"""
    f = bc.family(name)
    ages = f.sample_ages()
    assert api.builder_kind(f.N, ages is not None) == f.kind, (name, api.builder_kind(f.N, ages is not None), f.kind)
    host, dev = api.Builder(f.N), api.Builder(f.N, device=device)
    if ages is not None:
        host.set_sample_ages(ages)
        dev.set_sample_ages(ages)
    out = []
    for t, (d, prior) in enumerate(f.make()):
        ref = host.build(d, prior)
        census = host.census()
        assert not bc.check_census(census, f.want[t]), (name, t, census)
        t0 = time.time()
        got = dev.build(d, prior)
        out.append((int(dev.last_on_gpu), round(time.time() - t0, 3)))
        for what, a, b in zip(("parent", "child_left", "child_right"), ref, got):
            assert np.array_equal(a, b), (name, t, what, int(np.argmax(a != b)))
        if gold is not None:
            assert np.array_equal(got[0], gold[t]), (name, t, "reference", int(np.argmax(got[0] != gold[t])))
        predicted = bc.stays_on_device(census, f.N, ages is not None, f.sym_slots)
        assert dev.last_on_gpu == predicted, (name, t, "on the device: %s, predicted: %s" % (dev.last_on_gpu, predicted),
                                              census)
    host.close()
    dev.close()
    # (every family ends with a tree the lists hold: behind a hand-off the device builder has taken the state back)
    assert out[-1][0], (name, "the family ends with a tree of the device's")
    return out


@pytest.mark.parametrize("name", [f.name for f in bc.FAMILIES if not f.env])
def test_family(name):
    f = bc.family(name)
    built = check_family(name, GOLD[name] if f.golden else None)
    print("%s: (on the device, seconds) per tree %s" % (name, built))


@pytest.mark.parametrize("name", [f.name for f in bc.FAMILIES if f.env])
def test_family_under_a_switch(name):
    """the 10-slot kernel with two workgroups per CU (RELATE_AMD_BUILD_OCC=2, 2048 < N <= 5120), the 10-slot kernel at
    N = 2048 (=1), a device without a pool of symmetric matrices: the host's tree"""
    f = bc.family(name)
    # (a limit per child, by its size: the largest family builds in 5 s, a start of the runtime included)
    p = subprocess.run([sys.executable, "-c", CHILD, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **f.env), timeout=60 if f.N <= 2049 else 120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [x for x in p.stdout.decode().splitlines() if x.startswith("FAMILY ")]
    assert len(line) == 1, p.stdout.decode()[-1000:]
    built = json.loads(line[0][7:])
    assert len(built) == len(f.want)
    if f.sym_slots == 0:
        assert [b[0] for b in built] == [0, 1]  # (the tree that needs the symmetric matrix is the host's, the next one not)
    print("%s: (on the device, seconds) per tree %s" % (name, built))


def test_every_kernel_kind_at_its_largest_size():
    """worker_kind through rl_debug_builder_kind, without RELATE_AMD_BUILD_OCC (the two-per-CU 10-slot kernel: the
    families under the switch): the sizes at which a kernel's last register slot is taken and the first size of the
    next one (this process runs without the switch); the AGES build's edge between LDS and global memory where
    builder_cases puts it"""
    for N, kind in ((2, bc.HOT4), (2048, bc.HOT4), (2049, bc.WARM10), (5120, bc.WARM10), (5121, bc.HOT20),
                    (10240, bc.HOT20)):
        assert api.builder_kind(N) == kind, N
    E = bc.AGES_LDS_LAST_N
    for N, kind in ((2, bc.AGES_LDS10), (E, bc.AGES_LDS10), (E + 1, bc.AGES_GLOBAL10), (5120, bc.AGES_GLOBAL10),
                    (5121, bc.AGES_GLOBAL20), (10240, bc.AGES_GLOBAL20)):
        assert api.builder_kind(N, ages=True) == kind, N
    with pytest.raises(api.RelateError, match="rl_debug_builder_kind"):
        api.builder_kind(10241)
    largest = {}
    for f in bc.FAMILIES:
        largest[f.kind] = max(largest.get(f.kind, 0), f.N)
    # (the 20-slot AGES kernel: tests/test_builder_ages_gpu.py builds N = 5200 with it)
    assert largest == {bc.HOT4: 2048, bc.HOT10_2: 5120, bc.WARM10: 5120, bc.HOT20: 10240, bc.AGES_LDS10: E,
                       bc.AGES_GLOBAL10: 5120}
