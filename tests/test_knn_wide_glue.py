"""The reference's own knntest.o linked with host/glue/somhip_glue.c (oracle/_ref/knntest_hip) for more than 8
neighbours, against what the reference's knntest printed for the same inputs (tests/golden/knn_wide/expected.json, made
by tests/golden/make_golden_knn_wide.py): -knn 9 and -knn 21 on ex2.dat and on the masked ex2.

knntest.c:205-206 calls set_teach_params and then puts find_winner_knn into the winner slot itself, as setlabel.c:150,
balance.c:273 and lvqtrain.c:224-228 do: the "hip" row's table-serving winner is never asked for knn > 1 by these
programs, and its stderr line "winner: ... on the GPU (knn N)" cannot come out of knntest_hip whatever the glue does.
What is checked here is therefore the output: the same bytes with the "hip" row selected (on the GPU machine) and
without it.  The glue's own limit (hip_winner: the engine up to somhip_knn_max(), the reference's loop beyond) serves a
host program that leaves the row's winner in place; the engine behind it is tested in test_knn_wide.py."""
import importlib.util
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

REF = os.path.join(ROOT, "oracle", "_ref")
EXPECTED = json.load(open(os.path.join(GOLDEN, "knn_wide", "expected.json")))
KNNS = (9, 21)


def _glued(tool):
    exe = os.path.join(REF, tool)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs the reference sources at build time)" % tool)
    return exe


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (data file, codebook), the masked data made again by the fixture script's seeded masking"""
    spec = importlib.util.spec_from_file_location("make_golden_masked", os.path.join(GOLDEN, "make_golden_masked.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path_factory.mktemp("masked_data")
    mod.write_masked_data(str(out))
    return {"ex2": (os.path.join(GOLDEN, "data", "ex2.dat"), os.path.join(GOLDEN, "cli", "lvq_olvq1.cod")),
            "ex2_masked": (os.path.join(str(out), "ex2_masked.dat"), os.path.join(GOLDEN, "masked", "olvq1.cod"))}


def _knntest(din, cin, knn, *extra):
    p = subprocess.run([_glued("knntest_hip"), "-din", din, "-cin", cin, "-knn", str(knn)] + [str(a) for a in extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr
    return p


def test_fixtures_are_whole():
    assert sorted(EXPECTED) == ["ex2", "ex2_masked"]
    for name, runs in EXPECTED.items():
        assert sorted(runs) == ["21", "9"]
        for out in runs.values():
            assert "Total accuracy" in out
        assert runs["9"] != runs["21"], name


@pytest.mark.parametrize("knn", KNNS)
@pytest.mark.parametrize("name", ("ex2", "ex2_masked"))
def test_glued_knntest_keeps_its_cpu_path(cases, name, knn):
    din, cin = cases[name]
    assert _knntest(din, cin, knn, "-v", 0).stdout == EXPECTED[name][str(knn)]


@pytest.mark.gpu
@pytest.mark.parametrize("knn", KNNS)
@pytest.mark.parametrize("name", ("ex2", "ex2_masked"))
def test_glued_knntest_with_the_hip_row(cases, name, knn):
    din, cin = cases[name]
    p = _knntest(din, cin, knn, "-selfuncs", "hip", "-v", 2)
    assert p.stdout == EXPECTED[name][str(knn)]
