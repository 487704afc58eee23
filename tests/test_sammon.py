"""sammon: SOM_PAK's Sammon mapping on the GPU, bit for bit.

The real reference enters through tests/golden/sammon (written by tests/golden/make_golden_sammon.py from the reference's
own sammon.c).  tests/sammon_replay.py restates the reference's arithmetic in numpy; the CPU tests pin that replay against
the recorded reference outputs, the GPU tests compare the engine with the replay bit for bit and the tool with the
recorded files byte for byte."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sammon_replay as R
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
CLI = os.path.join(GOLDEN, "cli")
SAM = os.path.join(GOLDEN, "sammon")
EXPECTED = json.load(open(os.path.join(SAM, "expected.json")))
RUNS = sorted(EXPECTED["runs"])


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def tools():
    if not os.path.exists(os.path.join(BIN, "sammon")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a directory with every input of the recorded runs: the stored fixtures and the generated ones, md5 checked"""
    d = str(tmp_path_factory.mktemp("sammon_inputs"))
    R.write_generated(d, CLI)
    for name, want in EXPECTED["inputs"].items():
        if name not in R.GENERATED:
            shutil.copy(os.path.join(CLI, name), os.path.join(d, name))
        assert md5(os.path.join(d, name)) == want, name
    return d


def run_tool(args, cwd=None):
    return subprocess.run([os.path.join(BIN, "sammon")] + [str(a) for a in args], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, cwd=cwd)


def cod_rows(path):
    lines = [ln.split() for ln in open(path).read().split("\n")[1:] if ln.strip()]
    return lines


# ------------------------------------------------------------------ CPU side
@pytest.mark.parametrize("tag", RUNS)
def test_replay_reproduces_the_reference(tag, inputs):
    """the numpy replay (the promotion table of kernels/sammon.hpp) against what the real reference wrote: survivors,
    stderr lines of the removal, every token of the .cod under %g, and the -v 2 error lines"""
    from som_lvq_pak_amd import textio
    run = EXPECTED["runs"][tag]
    assert md5(os.path.join(SAM, tag + ".cod")) == run["md5"]
    ent, _ = textio.read_entries(os.path.join(inputs, run["cin"]))
    verbose = "-v 2" in " ".join(run["args"])
    out = R.sammon(ent.points, run["seed"], run["rlen"], errors=verbose)
    alive, msgs, x, y = out[:4]
    want = cod_rows(os.path.join(SAM, tag + ".cod"))
    assert len(want) == len(alive)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    for r, tok in enumerate(want):
        assert tok[0] == "%g" % float(x[r]) and tok[1] == "%g" % float(y[r]), (tag, r)
    removal = "".join(ln + "\n" for ln in run["stderr"].split("\n") if ln.startswith("Identical"))
    assert msgs == removal
    if verbose:
        assert ["Mapping error: %7.3f" % float(v) for v in out[4]] == [ln for ln in run["stdout"].split("\n") if ln]
    else:
        assert run["stdout"] == ""


def test_tool_usage_and_refusals(tools, tmp_path):
    p = run_tool(["-help"])
    assert p.returncode == 0 and "MI355X" in p.stdout and "-rlen" in p.stdout and "-eps" in p.stdout
    p = run_tool(["-cin", "a", "-cout", "b"])
    assert p.returncode == 255 and "Can't find asked option -rlen" in p.stderr
    out = tmp_path / "o.cod"
    # a masked codebook is refused before anything else happens, with or without a GPU
    p = run_tool(["-cin", os.path.join(GOLDEN, "masked", "olvq1.cod"), "-cout", out, "-rlen", 3, "-eps"])
    assert p.returncode == 1 and "masked components" in p.stderr
    assert not out.exists() and not (tmp_path / "o_sa.eps").exists()
    import torch
    if not torch.cuda.is_available():
        p = run_tool(["-cin", os.path.join(CLI, "som_hexa_gaussian.cod"), "-cout", out, "-rlen", 3, "-eps"])
        assert p.returncode == 1 and "no CPU path" in p.stderr
        assert not out.exists() and not (tmp_path / "o_sa.eps").exists()


def test_signatures_carry_sammon():
    import ctypes as C
    from som_lvq_pak_amd import _lib
    assert _lib.SIGNATURES["somhip_sammon_zero_pairs"] == (C.c_int, [C.c_void_p, _lib.c_u32_p, C.c_int64, _lib.c_i64_p])
    assert _lib.SIGNATURES["somhip_sammon"] == (C.c_int, [C.c_void_p, C.c_int64, _lib.c_float_p, _lib.c_float_p,
                                                          _lib.c_double_p])
    lib = _lib.load()
    names = [lib.somhip_kernel_name(i).decode() for i in range(lib.somhip_kernel_count())]
    assert names[0] == "k_scan_exact" and names[21] == "k_l2_select"          # the earlier ids keep their numbers
    for k in ("k_sammon_dist", "k_sammon_sweep", "k_sammon_centre", "k_sammon_error"):
        assert names.index(k) >= 22
    assert len(names) <= 64                                                     # somhip_timing_select's mask


def test_replay_walk_counts_like_the_reference():
    """remove_identicals' counters on a hand-made table: distance 0 is not transitive, and ij jumps by two after a
    removal (sammon.c:115)"""
    D = np.ones((5, 5), dtype=np.float32)
    np.fill_diagonal(D, 0)
    for a, b in ((0, 1), (1, 2), (0, 3)):        # 1 goes with 0; 2 stays although dd(1, 2) == 0; 3 goes
        D[a, b] = D[b, a] = 0
    alive, msgs = R.remove_identicals(D)
    assert list(alive) == [0, 2, 4]
    assert msgs == ("Identical entries in codebook (entries 1, 2), removing one.\n"
                    "Identical entries in codebook (entries 1, 5), removing one.\n")


# ------------------------------------------------------------------ GPU side
MAPPING_ERROR_BOUND = 0.002


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RUNS)
def test_tool_equals_the_reference_byte_for_byte(tag, tools, inputs, tmp_path):
    """.cod, _sa.eps / _sa.ps and stderr of every recorded run.  The -v 2 runs also print the mapping error: each value
    within 0.002 of the reference's line.  Derivation of that bound: the reference adds n = noc (noc - 1) / 2 positive
    terms in fp32 in sequence, off by at most (n - 1) 2^-24 relative; the recorded -v 2 runs keep (n - 1) 2^-24 e below
    0.0014 (asserted below from the reference's own lines: noc = 96, e <= 2.6 and e <= 4.6; the reference's step of 0.2
    overshoots in its first iterations, so e <= 0.5 holds on no recorded run from its start), plus
    0.0005 of print rounding.  The engine's value is a double-precision tree sum of the same float terms."""
    run = EXPECTED["runs"][tag]
    work = str(tmp_path)
    shutil.copy(os.path.join(inputs, run["cin"]), os.path.join(work, run["cin"]))
    p = run_tool(run["args"], cwd=work)
    assert p.returncode == 0, p.stderr
    assert p.stderr == run["stderr"]
    assert open(os.path.join(work, tag + ".cod"), "rb").read() == open(os.path.join(SAM, tag + ".cod"), "rb").read()
    for kind in ("eps", "ps"):
        pic = os.path.join(work, "%s_sa.%s" % (tag, kind))
        assert os.path.exists(pic) == (kind + "_md5" in run)
        if os.path.exists(pic):
            assert md5(pic) == run[kind + "_md5"], kind
    if "-v 2" not in " ".join(run["args"]):
        assert p.stdout == ""
        return
    want = [float(ln.split(":")[1]) for ln in run["stdout"].split("\n") if ln]
    got = [float(ln.split(":")[1]) for ln in p.stdout.split("\n") if ln]
    assert len(got) == len(want) == run["rlen"]
    noc = len(cod_rows(os.path.join(SAM, tag + ".cod")))
    pairs = noc * (noc - 1) // 2
    worst = max(abs(a - b) for a, b in zip(got, want))
    print("mapping error %s: noc %d, largest difference to the reference's line %.4f" % (tag, noc, worst))
    assert noc <= 300 and (pairs - 1) * 2.0 ** -24 * max(want) < 0.0014        # the case is inside the derivation
    assert worst <= MAPPING_ERROR_BOUND


def _case_rows(noc, dim):
    rs = np.random.RandomState(1000 * dim + noc)
    return (3.0 * rs.standard_normal((noc, dim))).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 5, 33])
@pytest.mark.parametrize("noc", [2, 3, 63, 64, 65, 257, 1085])
def test_engine_equals_the_replay_bit_for_bit(noc, dim, eng):
    """(the plan has one form of the sweep kernel to choose: the lane-per-row form lost at every measured size and
    was deleted, profiles/sammon_sweep.txt)"""
    from som_lvq_pak_amd import engine as E
    rows = _case_rows(noc, dim)
    D = R.distances(rows)
    assert len(R.zero_pairs(D)) == 0
    x0, y0 = R.initial_table(noc, 11 + noc)
    rlens = (0, 1, 7, 50)
    _, _, snap = R.iterate(x0, y0, D, max(rlens), snapshots=rlens)
    cb = E.Codebook(eng, rows)
    assert len(E.sammon_zero_pairs(cb)) == 0
    for rlen in rlens:
        x, y = E.sammon(cb, x0, y0, rlen)
        wx, wy = snap[rlen]
        assert np.array_equal(x.view(np.uint32), wx.view(np.uint32)), (rlen, "x")
        assert np.array_equal(y.view(np.uint32), wy.view(np.uint32)), (rlen, "y")
    cb.close()


@pytest.mark.gpu
def test_engine_maps_a_map_in_patch_order(eng):
    """a 16 x 8 map is stored in 8 x 8 patches on the device; the mapping works on the rows in unit order all the same"""
    from som_lvq_pak_amd import engine as E
    rows = _case_rows(128, 6)
    D = R.distances(rows)
    x0, y0 = R.initial_table(128, 5)
    wx, wy = R.iterate(x0, y0, D, 5)
    cb = E.Codebook(eng, rows, E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 8)
    x, y = E.sammon(cb, x0, y0, 5)
    assert np.array_equal(x.view(np.uint32), wx.view(np.uint32)) and np.array_equal(y.view(np.uint32), wy.view(np.uint32))
    cb.close()


def _zero_pair_cases():
    rs = np.random.RandomState(77)
    base = rs.standard_normal((200, 7)).astype(np.float32)
    dup = base.copy()
    for a, b in ((5, 0), (6, 0), (150, 149), (199, 3), (64, 63), (128, 3)):
        dup[a] = dup[b]
    same = np.repeat(base[:1], 100, axis=0)                  # one repeated row: 4950 pairs, more than 16 * noc
    # distance 0 without equality: the squares of these differences underflow (2e-23 ^ 2 = 4e-46 rounds to 0, while
    # 4e-23 ^ 2 = 1.6e-45 rounds to the smallest subnormal), so 0 ~ 1 and 1 ~ 2 but not 0 ~ 2
    tiny = np.zeros((70, 3), dtype=np.float32)
    tiny[:, 0] = np.arange(70, dtype=np.float32) * np.float32(5.0)
    tiny[1] = tiny[0]; tiny[2] = tiny[0]
    tiny[1, 1] = np.float32(2e-23); tiny[2, 1] = np.float32(4e-23)
    tiny[40, 2] = np.float32(1e-30); tiny[41] = tiny[40]; tiny[41, 2] = np.float32(-1e-30)
    return {"duplicates": dup, "one_row_repeated": same, "underflow": tiny, "none": base}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["duplicates", "one_row_repeated", "underflow", "none"])
def test_zero_pairs_equal_the_reference_distance(name, eng):
    from som_lvq_pak_amd import engine as E
    rows = _zero_pair_cases()[name]
    want = R.zero_pairs(R.distances(rows))
    if name == "underflow":
        assert [0, 1] in want.tolist() and [1, 2] in want.tolist() and [0, 2] not in want.tolist()
        assert [40, 41] in want.tolist() and not np.array_equal(rows[40], rows[41])
    assert (len(want) == 0) == (name == "none")
    cb = E.Codebook(eng, rows)
    got = E.sammon_zero_pairs(cb)
    assert got.shape == want.shape and np.array_equal(got, want)
    cb.close()


@pytest.mark.gpu
def test_refusals(eng, tools, tmp_path):
    from som_lvq_pak_amd import engine as E
    from som_lvq_pak_amd._lib import SomhipError
    one = E.Codebook(eng, np.ones((1, 4), dtype=np.float32))
    with pytest.raises(SomhipError, match="no pair"):
        E.sammon(one, np.zeros(1, np.float32), np.zeros(1, np.float32), 3)
    rows = _zero_pair_cases()["duplicates"]
    cb = E.Codebook(eng, rows)
    x0, y0 = R.initial_table(200, 3)
    with pytest.raises(SomhipError, match="distance 0"):
        E.sammon(cb, x0, y0, 3)
    with pytest.raises(ValueError):
        E.sammon(cb, x0[:10], y0[:10], 3)
    good = E.Codebook(eng, _zero_pair_cases()["none"])           # the engine is fine after the refusals
    x, y = E.sammon(good, x0, y0, 1)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    # the tool: a masked codebook, and a codebook that is one row after the removal
    out = tmp_path / "o.cod"
    p = run_tool(["-cin", os.path.join(GOLDEN, "masked", "olvq1.cod"), "-cout", out, "-rlen", 3])
    assert p.returncode == 1 and "masked components" in p.stderr and not out.exists()
    with open(tmp_path / "same.cod", "w") as f:
        f.write("3\n" + "1 2 3\n" * 40)
    p = run_tool(["-cin", tmp_path / "same.cod", "-cout", out, "-rlen", 3, "-v", 0])
    assert p.returncode == 1 and "nothing to map" in p.stderr and not out.exists()
    assert p.stderr.count("Identical entries in codebook") == 39
