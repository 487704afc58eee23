"""somqual: the qerror tool's line, the topographic error and the per-unit file of a map, from somhip_map_quality, on the
package's example data and a committed map, against the qerror tool and the CPU replay (map_quality_replay.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_cod
from map_quality_replay import Replay, unit_lines

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
DATA = os.path.join(GOLDEN, "data", "ex.dat")
MAP = os.path.join(GOLDEN, "cli", "som_hexa_bubble.cod")


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("somqual", "qerror")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args, check=True):
    p = subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    if check:
        assert p.returncode == 0, (tool, args, p.stderr)
    return p


@pytest.fixture(scope="module")
def replayed(oracle, exdata):
    cod = read_cod("som_hexa_bubble.cod")
    rep = Replay(oracle, cod.points, cod.xdim, cod.ydim, cod.topol, exdata["ex"].points)
    return cod, rep.run()


@pytest.mark.gpu
def test_somqual_on_the_example_data(tools, tmp_path, replayed):
    cod, (tot, hits, qsum) = replayed
    uout = tmp_path / "units.txt"
    p = run("somqual", "-din", DATA, "-cin", MAP, "-uout", uout)
    lines = p.stdout.split("\n")
    assert len(lines) == 4 and lines[3] == ""
    assert lines[0] + "\n" == run("qerror", "-din", DATA, "-cin", MAP).stdout
    m = re.fullmatch(r"Topographic error is (\d+\.\d{6}) \((\d+) of (\d+) samples\)", lines[1])
    assert m and (int(m.group(2)), int(m.group(3))) == (tot["topo_errors"], tot["topo_defined"])
    assert m.group(1) == "%f" % (tot["topo_errors"] / tot["topo_defined"])
    assert 0 < tot["topo_errors"] < tot["topo_defined"] == tot["searched"] == int(hits.sum())
    assert lines[2] == "%d of %d units were hit by no sample" % (int((hits == 0).sum()), len(hits))
    assert uout.read_text() == unit_lines(cod.xdim, hits, qsum)
    # -v 0: the bare number, as qerror prints it
    q0 = run("somqual", "-din", DATA, "-cin", MAP, "-v", 0).stdout.split("\n")
    assert q0[0] + "\n" == run("qerror", "-din", DATA, "-cin", MAP, "-v", 0).stdout and q0[1:] == lines[1:]
    # the data taken buffer by buffer: the same bytes
    for n in (7, 4096):
        ub = tmp_path / ("units_%d.txt" % n)
        pb = run("somqual", "-din", DATA, "-cin", MAP, "-uout", ub, "-buffer", n)
        assert pb.stdout == p.stdout and ub.read_bytes() == uout.read_bytes()


@pytest.mark.gpu
def test_somqual_reads_raw_fp32_and_generated_sources(tools, tmp_path):
    """the other two sources the tools read: the first line is the qerror tool's on the same source"""
    raw = tmp_path / "ex.f32"
    run("datconv", "-din", DATA, "-dout", raw)
    text = run("somqual", "-din", DATA, "-cin", MAP).stdout.split("\n")
    got = run("somqual", "-din", raw, "-cin", MAP).stdout.split("\n")
    assert got[0] + "\n" == run("qerror", "-din", raw, "-cin", MAP).stdout and got[1:] == text[1:]
    gen = "gen:k=4,dim=5,n=3000,seed=9"
    got = run("somqual", "-din", gen, "-cin", MAP).stdout.split("\n")
    assert got[0] + "\n" == run("qerror", "-din", gen, "-cin", MAP).stdout
    assert re.fullmatch(r"Topographic error is \d+\.\d{6} \(\d+ of 3000 samples\)", got[1])
    assert got == run("somqual", "-din", gen, "-cin", MAP, "-buffer", 1000).stdout.split("\n")


@pytest.mark.gpu
def test_somqual_refusals(tools, tmp_path):
    other = tmp_path / "dim3.dat"
    other.write_text("3\n1 2 3\n4 5 6\n")
    p = run("somqual", "-din", other, "-cin", MAP, check=False)
    assert p.returncode != 0 and "different dimensions" in p.stderr
    masked = tmp_path / "masked.cod"
    rows = open(MAP).read().split("\n")
    rows[1] = " ".join(["x"] + rows[1].split()[1:])
    masked.write_text("\n".join(rows))
    p = run("somqual", "-din", DATA, "-cin", masked, check=False)
    assert p.returncode != 0 and "masked components" in p.stderr
    lvq = os.path.join(GOLDEN, "cli", "lvq_init.cod")
    p = run("somqual", "-din", DATA, "-cin", lvq, check=False)
    assert p.returncode != 0 and "not a map file" in p.stderr
