"""somqual -conn: the pairs of best and second-best unit of a map with their sample counts, from somhip_map_connectivity in
the same search as the tool's other figures, on the package's example data and a committed map, against the CPU replay
(map_conn_replay.py)."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, read_cod
from map_conn_replay import ConnReplay, apart, pair_lines

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
DATA = os.path.join(GOLDEN, "data", "ex.dat")
MAP = os.path.join(GOLDEN, "cli", "som_hexa_bubble.cod")


@pytest.fixture(scope="module")
def tools():
    if not os.path.exists(os.path.join(BIN, "somqual")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(*args):
    p = subprocess.run([os.path.join(BIN, "somqual")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (args, p.stderr)
    return p.stdout


@pytest.mark.gpu
def test_somqual_conn_on_the_example_data(tools, tmp_path, oracle, exdata):
    cod = read_cod("som_hexa_bubble.cod")
    table = ConnReplay(oracle, cod.points, exdata["ex"].points).table()
    far = apart(cod.topol, cod.xdim, table[0], table[1])
    plain = run("-din", DATA, "-cin", MAP)
    assert plain.count("\n") == 3
    out, uout = tmp_path / "pairs.txt", tmp_path / "units.txt"
    got = run("-din", DATA, "-cin", MAP, "-conn", out, "-uout", uout)
    lines = got.split("\n")
    assert len(lines) == 5 and lines[4] == ""
    assert "\n".join(lines[:3]) + "\n" == plain
    assert 0 < int(far.sum()) < len(far)
    assert lines[3] == ("Connected pairs (best unit, second-best unit): %d, of which %d are not neighbours on the lattice"
                        % (len(far), int(far.sum())))
    assert out.read_text() == pair_lines(cod.topol, cod.xdim, table)
    # -uout is what it is without -conn
    u0 = tmp_path / "units0.txt"
    run("-din", DATA, "-cin", MAP, "-uout", u0)
    assert uout.read_bytes() == u0.read_bytes()
    # the data taken buffer by buffer, one table through all of them: the same bytes
    for n in (7, 4096):
        ob = tmp_path / ("pairs_%d.txt" % n)
        assert run("-din", DATA, "-cin", MAP, "-conn", ob, "-buffer", n) == got
        assert ob.read_bytes() == out.read_bytes()


@pytest.mark.gpu
def test_somqual_conn_on_a_generated_source(tools, tmp_path):
    gen = "gen:k=4,dim=5,n=3000,seed=9"
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    whole = run("-din", gen, "-cin", MAP, "-conn", a)
    assert whole == run("-din", gen, "-cin", MAP, "-conn", b, "-buffer", 1000)
    assert a.read_bytes() == b.read_bytes() and len(a.read_text().split("\n")) > 2
    assert whole.split("\n")[:3] == run("-din", gen, "-cin", MAP).split("\n")[:3]
    assert sum(int(line.split()[4]) for line in a.read_text().splitlines()) == 3000
