"""Selection (rl_selection_logp, rl_selection_files, `Relate --mode Selection`; relate_amd/csrc/selection.cpp) against
what the reference's RelateSelection wrote (tests/golden/selection_ref.npz): the .sele bytes from the reference's
.freq / .lin and from this library's, single cells, any thread count."""
import os
import subprocess

import numpy as np
import pytest

import frequency_cases as fc
import test_frequency_cpu as freq_tests
from relate_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "relate_amd", "Relate")


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def write_reference_files(tmp_path, fx, key):
    prefix = str(tmp_path / ("ref_" + key))
    open(prefix + ".freq", "wb").write(fx[key + "/freq"].tobytes())
    open(prefix + ".lin", "wb").write(fx[key + "/lin"].tobytes())
    return prefix


@pytest.mark.parametrize("key", fc.CASES)
def test_sele_from_the_references_files(fx, tmp_path, key):
    prefix = write_reference_files(tmp_path, fx, key)
    api.selection_files(prefix, prefix + ".sele")
    assert open(prefix + ".sele", "rb").read() == fx[key + "/sele"].tobytes()


@pytest.mark.parametrize("key", fc.CASES)
def test_sele_from_this_librarys_files(fx, tmp_path, key):
    freq_tests.check_fixture_case(fx, tmp_path, key, None)
    out = str(tmp_path / (key + "_out"))
    api.selection_files(out, out + ".sele")
    assert open(out + ".sele", "rb").read() == fx[key + "/sele"].tobytes()


def cells(fx, key):
    """every cell of a case: (k, fk, N, fN, the reference's text), rows with fN <= 2 left out (they are all `1`)"""
    freq, lin, sele = (fx[key + ext].tobytes().decode().split("\n")[1:-1] for ext in ("/freq", "/lin", "/sele"))
    N = int(lin[0].split()[-3])
    for f, l, s in zip(freq, lin, sele):
        f, l, s = f.split()[2:], l.split()[2:], s.split()[2:]
        E, fN = len(l) - 2, float(f[len(l) - 3])
        if fN <= 2:
            assert s == ["1"] * (E + 2)
            continue
        for i in range(E):
            yield int(l[i]), float(f[i]), N, fN, s[i]
        yield int(l[E]), float(int((fN + 1.0) / 2.0)), N, fN, s[E]
        yield int(l[E + 1]), 2.0, N, fN, s[E + 1]


def test_logp_equals_the_fixtures_cells(fx):
    """every 7th cell of case a, every cell of case s and of the tie case, with the kinds the issue names among them:
    fk < 2 and a sum without a term (fN - fk == N - k); k = -1 with fk >= 2 is in no row of a file (a row whose
    when_DAF_is_half is -1 has fN <= 2 and is all `1`): it is asked for directly"""
    seen = {"fk<2": 0, "no term": 0, "terms": 0}
    for key, step in (("a", 7), ("s", 1), ("tie", 1)):
        for n, (k, fk, N, fN, text) in enumerate(cells(fx, key)):
            if n % step:
                continue
            assert "%g" % api.selection_logp(k, fk, N, fN) == text, (key, k, fk, N, fN)
            kind = "fk<2" if fk < 2 else "no term" if fN - fk == N - k else "terms"
            seen[kind] += 1
    assert all(seen.values()), seen
    assert api.selection_logp(-1, 5, 100, 40) == 1.0 and api.selection_logp(50, 1, 100, 40) == 1.0
    for k, fk, N, fN, word in ((50, 10, 100, 100, "fN < N"), (10, 10, 100, 40, "fk < k"), (50, 45, 100, 40, "index")):
        with pytest.raises(api.RelateError, match=word):
            api.selection_logp(k, fk, N, fN)


def test_thread_count_does_not_change_a_byte(fx, tmp_path, monkeypatch):
    prefix = write_reference_files(tmp_path, fx, "a")
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("RELATE_AMD_THREADS", threads)
        api.selection_files(prefix, prefix + "_%s.sele" % threads)
        assert open(prefix + "_%s.sele" % threads, "rb").read() == fx["a/sele"].tobytes(), threads


def test_cli(fx, tmp_path):
    write_reference_files(tmp_path, fx, "s")
    p = subprocess.run([CLI, "--mode", "Selection", "-i", "ref_s", "-o", "out"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert b"Calculating evidence of selection for ref_s.\n" in p.stderr and b"CPU Time spent" in p.stderr
    assert open(str(tmp_path / "out.sele"), "rb").read() == fx["s/sele"].tobytes()


def test_refusals(fx, tmp_path):
    prefix = write_reference_files(tmp_path, fx, "b")
    lin = fx["b/lin"].tobytes().split(b"\n")
    open(prefix + "_short.freq", "wb").write(fx["b/freq"].tobytes())
    open(prefix + "_short.lin", "wb").write(b"\n".join(lin[:-2]) + b"\n")
    with pytest.raises(api.RelateError, match="rows"):
        api.selection_files(prefix + "_short", prefix + ".sele")
    with pytest.raises(api.RelateError, match="failed to open"):
        api.selection_files(prefix + "_none", prefix + ".sele")
    # a row whose carriers exceed its lineages: the reference's assert, named with the row
    freq = fx["s/freq"].tobytes().split(b"\n")
    r = next(r for r in range(1, len(freq) - 1) if float(freq[r].split(b" ")[2 + 30]) > 2)
    row = freq[r].split(b" ")
    row[2 + 28] = b"299"
    freq[r] = b" ".join(row)
    open(prefix + "_bad.freq", "wb").write(b"\n".join(freq))
    open(prefix + "_bad.lin", "wb").write(fx["s/lin"].tobytes())
    with pytest.raises(api.RelateError, match="row %d: .*fk < k" % (r - 1)):
        api.selection_files(prefix + "_bad", prefix + ".sele")
    # and the process goes on to a correct answer
    api.selection_files(prefix, prefix + ".sele")
    assert open(prefix + ".sele", "rb").read() == fx["b/sele"].tobytes()
