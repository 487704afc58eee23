"""vfind's trial loop as a map set (som_lvq_pak_amd/host/vfind.c): the default route (all trials trained together),
-together 1 (one trial at a time, the earlier route), -together 3 (several sets) and -gpus 2 (each rank its share) print
the same bytes and save the same map -- and two of the cases are the REAL reference's own vfind, nine trials each
(tests/golden/vfind_together, made by tests/golden/make_golden_vfind_together.py)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
DATA = os.path.join(GOLDEN, "data")
GOLD = os.path.join(GOLDEN, "vfind_together")
EXPECTED = json.load(open(os.path.join(GOLD, "expected.json")))

# trials, data, test, out, topology, neighbourhood, xdim, ydim, length / alpha / radius of the two parts
HEXA_BUBBLE = ["{n}", "{data}", "{data}", "{out}", "hexa", "bubble", "6", "5", "300", "0.05", "5", "700", "0.02", "2"]
RECT_GAUSSIAN = ["{n}", "{data}", "{data}", "{out}", "rect", "gaussian", "7", "4", "300", "0.05", "4", "500", "0.02", "1.5"]
CASES = {
    "hexa_bubble": ("ex.dat", HEXA_BUBBLE, []),
    "rect_gaussian": ("ex.dat", RECT_GAUSSIAN, []),
    "fixed_weights": ("ex_fts.dat", HEXA_BUBBLE, ["-fixed", "1", "-weights", "1"]),
    "qetype1": ("ex.dat", HEXA_BUBBLE, ["-qetype", "1"]),
    "masked": ("ex_masked.dat", HEXA_BUBBLE, []),
    "inverse_t": ("ex.dat", RECT_GAUSSIAN, ["-alpha_type", "inverse_t"]),
}
ROUTES = {"default": [], "together1": ["-together", "1"], "together3": ["-together", "3"], "gpus2": ["-gpus", "2"]}


@pytest.fixture(scope="module")
def tools():
    if not os.path.exists(os.path.join(BIN, "vfind")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def vfind(tmp, data, answers, trials, args, tag):
    """one run with -v 1 in tmp (short, relative file names: an answer is at most 99 characters): (stdout, stderr, map bytes)"""
    if not os.path.exists(os.path.join(tmp, data)):
        shutil.copy(os.path.join(DATA, data), os.path.join(tmp, data))
    out = "out.cod"
    if os.path.exists(os.path.join(tmp, out)):
        os.remove(os.path.join(tmp, out))
    ans = "\n".join(a.format(n=trials, data=data, out=out) for a in answers) + "\n"
    p = subprocess.run([os.path.join(BIN, "vfind"), "-v", "1"] + args, input=ans, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, cwd=tmp, timeout=120)
    assert p.returncode == 0, (tag, p.stderr)
    return p.stdout, p.stderr, open(os.path.join(tmp, out), "rb").read()


@pytest.mark.parametrize("case", sorted(CASES))
def test_vfind_routes_agree_byte_for_byte(tools, tmp_path, case):
    data, answers, args = CASES[case]
    runs = {route: vfind(str(tmp_path), data, answers, 7, args + extra, (case, route)) for route, extra in ROUTES.items()}
    base = runs["together1"]                              # the route that was there before map sets
    assert len([ln for ln in base[1].splitlines() if ": " in ln and ln.strip()[:1].isdigit()]) == 7, base[1]
    assert base[0].strip().splitlines()[-1].startswith("Smallest error with random seed")
    for route, got in runs.items():
        assert got[0] == base[0], (case, route, "stdout")
        assert got[1] == base[1], (case, route, "stderr")
        assert got[2] == base[2], (case, route, "map")


@pytest.mark.parametrize("case", sorted(EXPECTED))
@pytest.mark.parametrize("route", ["default", "together3"])
def test_vfind_sets_equal_the_reference(tools, tmp_path, case, route):
    ex = EXPECTED[case]
    answers = [a.replace("9", "{n}") if i == 0 else a for i, a in enumerate(ex["answers"])]
    out, err, cod = vfind(str(tmp_path), ex["data"], answers, 9, ex["args"] + ROUTES[route], (case, route))
    assert [ln for ln in err.splitlines() if ": " in ln and ln.strip()[:1].isdigit()] == ex["trials_stderr"]
    assert out.strip().splitlines()[-1] == ex["last_stdout_line"]
    assert cod == open(os.path.join(GOLD, case + ".cod"), "rb").read()
