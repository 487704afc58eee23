"""planes: SOM_PAK's component-plane and trajectory pictures of a map, grey levels computed on the GPU, bit for bit.

The real reference enters through tests/golden/planes (written by tests/golden/make_golden_planes.py from the reference's
own planes.c; only results are recorded, never the bodies of its two PostScript procedures).  tests/planes_replay.py
restates the reference's arithmetic, its winner search and its two writers in numpy; the CPU tests pin that replay against
the recorded runs, the GPU tests compare the engine's entry point with the replay bit for bit and the tool with the
recorded runs byte for byte outside the procedure bodies."""
import ctypes as C
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import planes_replay as R
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
HOST = os.path.join(ROOT, "som_lvq_pak_amd", "host")
EXPECTED = json.load(open(os.path.join(GOLDEN, "planes", "expected.json")))
RUNS = sorted(EXPECTED["runs"])


@pytest.fixture(scope="module")
def tools():
    if not os.path.exists(os.path.join(BIN, "planes")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", HOST])
    return BIN


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a directory with every input of the recorded runs: the stored fixtures and the generated ones, md5 checked"""
    d = str(tmp_path_factory.mktemp("planes_inputs"))
    R.write_generated(d)
    for name, want in EXPECTED["inputs"].items():
        if name not in R.generated_names():
            shutil.copy(os.path.join(GOLDEN, "data" if name.endswith(".dat") else "cli", name), os.path.join(d, name))
        assert hashlib.md5(open(os.path.join(d, name), "rb").read()).hexdigest() == want, name
    return d


def run_tool(args, cwd=None, tool="planes"):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, cwd=cwd)


def pictures(d):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.eps")) + glob.glob(os.path.join(d, "*.ps")))


def fresh_copy(inputs, tmp_path, args):
    """a directory of its own that holds the run's input files: the output lands beside -cin"""
    for flag in ("-cin", "-din"):
        if flag in args:
            name = args[args.index(flag) + 1]
            shutil.copy(os.path.join(inputs, name), os.path.join(str(tmp_path), name))
    return str(tmp_path)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ CPU side
@pytest.mark.parametrize("tag", RUNS)
def test_replay_reproduces_the_reference(tag, inputs):
    """the numpy replay writes what the real reference wrote: the file names, the md5 of every normalised file, its parsed
    content, the return code and both message streams"""
    run = EXPECTED["runs"][tag]
    got = R.replay_run(run["args"], inputs)
    assert sorted(got["files"]) == sorted(run["files"])
    for name, want in run["files"].items():
        content = json.loads(json.dumps(R.parse_text(got["files"][name])))
        for key in sorted(want["content"]):
            assert content[key] == want["content"][key], (name, key)
        assert R.md5_text(got["files"][name]) == want["md5"], name
    assert (got["returncode"], got["stdout"], got["stderr"]) == (run["returncode"], run["stdout"], run["stderr"])


def test_recorded_runs_cover_the_cases():
    runs = EXPECTED["runs"]
    assert sorted(runs["all_hexa"]["files"]) == ["som_hexa_gaussian_p%d.eps" % k for k in range(1, 6)]
    assert sorted(runs["ps_all_rect"]["files"]) == ["som_rect_gaussian_p%d.ps" % k for k in range(1, 6)]
    assert list(runs["default_plane"]["files"]) == ["som_rect_gaussian_p1.eps"]
    assert list(runs["single_plane"]["files"]) == ["som_hexa_bubble_p3.eps"]
    ps = runs["ps_plane"]["files"]["som_hexa_bubble_p2.ps"]["content"]
    assert ps["showpage"] == 1 and ps["sizes"]["page"] == ["760", "500", "510", "272"]           # 12 * 40 + 20, 8 * 34
    assert runs["all_rect"]["files"]["som_rect_bubble_p1.eps"]["content"]["sizes"]["BoundingBox"] == ["0", "0", "480", "320"]
    assert any(lab for f in runs["labels_vcal"]["files"].values() for lab in f["content"]["labels"])
    parens = runs["labels_parens"]["files"]["parens_p1.eps"]["content"]["labels"]
    assert [l[2] for l in parens] == ["f(x)", "back\\slash", "c)(", "plain", "((", "a\\(b"]
    constant = runs["constant"]["files"]
    assert {d[2] for d in constant["constant_p3.eps"]["content"]["discs"]} == {"0.500000"}
    assert len({d[2] for d in constant["constant_p2.eps"]["content"]["discs"]}) > 10
    for tag, n in (("traj_ex_hexa", 3840), ("traj_ex_rect_ps", 3840), ("traj_masked", 500)):
        tr = [f for name, f in runs[tag]["files"].items() if "_tr." in name][0]["content"]
        assert [len(p) for p in tr["paths"]] == [n] and tr["strokes"] == 1 and len(tr["circles"]) == 96
    # rows with every component masked: nothing at the start, a break for two in a row and for a single one, and two
    # stroke lines in a row at the end
    for tag in ("traj_breaks", "traj_breaks_buffer"):
        tr = runs[tag]["files"]["som_hexa_gaussian_tr.eps"]
        assert [len(p) for p in tr["content"]["paths"]] == [12, 11, 11] and tr["content"]["strokes"] == 4
    assert runs["traj_breaks"]["files"] == runs["traj_breaks_buffer"]["files"]
    assert runs["traj_masked"]["files"] == runs["traj_masked_buffer"]["files"] and "-buffer" in runs["traj_masked_buffer"]["args"]
    # x outermost among the circles, y outermost among the discs
    assert runs["traj_ex_hexa"]["files"]["som_hexa_gaussian_tr.eps"]["content"]["circles"][:2] == [[20, 17], [40, 51]]
    assert [d[:2] for d in runs["all_hexa"]["files"]["som_hexa_gaussian_p1.eps"]["content"]["discs"][:2]] == [[20, 17], [60, 17]]
    assert runs["err_not_a_map"]["stdout"] == "File lvq_olvq1.cod is not a map file\n" and runs["err_not_a_map"]["stderr"] == ""
    assert runs["err_plane_too_high"]["stderr"] == "Required plane is bigger than codebook vector dimension"
    assert runs["err_data_wider"]["stderr"] == "Dimensions in data and codebook files are different"
    assert all(runs[t]["returncode"] == 1 and not runs[t]["files"] for t in runs if t.startswith("err_"))


@pytest.mark.parametrize("mode", ["all_float", "double_difference"])
def test_rounding_map_tells_the_arithmetic_apart(mode, inputs):
    """an evaluation all in float32, and one whose differences are taken in float64, each print another grey level
    somewhere on the rounding map: the recorded md5s pin the reference's promotions"""
    run = EXPECTED["runs"]["round"]
    assert len(run["files"]) == R.ROUND_SHAPE[2]
    got = R.replay_run(run["args"], inputs, mode=mode)
    changed = [name for name, want in run["files"].items() if R.md5_text(got["files"][name]) != want["md5"]]
    assert changed, mode
    rows = R.round_rows()
    a, b = R.planes(rows)[0], R.planes(rows, mode=mode)[0]
    assert (bits(a) != bits(b)).sum() > 100                                  # hundreds of floats, a few dozen of them printed


def test_replay_edge_values():
    """the replay itself at the values the GPU tests lean on"""
    tiny = np.float32(1e-45)
    g, lo, hi = R.planes(np.array([[0.0], [tiny], [0.0]], dtype=np.float32))
    assert bits(g[0]).tolist() == bits(np.float32([0.05, 0.95, 0.05])).tolist() and (lo[0], hi[0]) == (0.0, tiny)
    g, lo, hi = R.planes(np.array([[-0.0], [0.0], [-0.0]], dtype=np.float32))
    assert g[0].tolist() == [0.5] * 3 and bits(lo)[0] == bits(hi)[0] == 0x80000000       # the first row's zero stays
    g, lo, hi = R.planes(np.array([[0.0], [-0.0]], dtype=np.float32))
    assert bits(lo)[0] == bits(hi)[0] == 0
    g, lo, hi = R.planes(np.array([[7.0, -3.0]], dtype=np.float32), 1, 1)
    assert g.tolist() == [[0.5]] and (lo[0], hi[0]) == (-3.0, -3.0)


def test_abi_names_the_entry_point():
    from som_lvq_pak_amd import _lib
    fp = _lib.c_float_p
    assert _lib.SIGNATURES["somhip_planes"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp, fp, fp])
    assert hasattr(_lib.load(), "somhip_planes")
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r"int\s+somhip_planes\(somhip_codebook \*cb, int first_plane, int n_planes,\s*float \*grey, float \*lo, "
                     r"float \*hi\);", hdr)
    from som_lvq_pak_amd import engine as E
    assert callable(E.planes)


def test_tool_usage_and_refusals_without_a_gpu(tools, inputs, tmp_path):
    p = run_tool(["-help"])
    assert p.returncode == 0 and b"MI355X" in p.stdout
    for flag in ("-cin", "-din", "-plane", "-ps", "-buffer", "-selfuncs", "-v"):
        assert flag.encode() in p.stdout, flag
    p = run_tool(["-plane", "2"])
    assert p.returncode == 255 and b"Can't find asked option -cin" in p.stderr
    d = str(tmp_path)
    for name in ("som_hexa_gaussian.cod", "lvq_olvq1.cod", "wide.dat"):
        shutil.copy(os.path.join(inputs, name), os.path.join(d, name))
    (tmp_path / "masked.cod").write_text("2 hexa 2 2 bubble\n1 2\n3 x\n5 6\n7 8\n")
    (tmp_path / "short.cod").write_text("2 rect 2 2 bubble\n1 2\n3 4\n5 6\n")
    (tmp_path / "narrow.dat").write_text("4\n1 2 3 4\n5 6 7 8\n")
    runs = EXPECTED["runs"]
    cases = [(runs[t]["args"], runs[t]["stdout"], runs[t]["stderr"]) for t in ("err_not_a_map", "err_plane_too_high",
                                                                              "err_data_wider")]
    for args, out, err in cases:                                           # the reference's three, with its messages
        p = run_tool(args, cwd=d)
        assert (p.returncode, p.stdout.decode(), p.stderr.decode()) == (1, out, err), args
    for args, word in ((["-cin", "som_hexa_gaussian.cod", "-plane", "-1"], b"-plane -1"),
                       (["-cin", "masked.cod"], b"masked"),
                       (["-cin", "short.cod"], b"3 entries"),
                       (["-cin", "som_hexa_gaussian.cod", "-din", "narrow.dat"], b"4 components")):
        p = run_tool(args, cwd=d)
        assert p.returncode == 1 and word in p.stderr and p.stdout == b"", (args, p.stderr)
        assert b"HIP" not in p.stderr and b"hip" not in p.stderr           # refused before an engine was asked for
    assert pictures(d) == []


# ------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


KINDS = ["negative", "positive", "mixed", "constant", "last_group", "denormal", "zeros"]
SHAPES = [(1, 1, 0), (63, 3, 4), (64, 4, 0), (65, 5, 2), (4485, 9, 0)]       # rows, dim, the kind of component 0


def case_rows(n, d, shift):
    """component c is of kind KINDS[(c + shift) % 7]:
    negative    every value below -1                      positive   every value from 1000 up (padding zeros would win the minimum)
    mixed       both signs, magnitudes over six decades   constant   one value (cv = 0.5)
    last_group  as mixed, but the smallest and the largest value lie in the last two rows
    denormal    0 and 1e-45, the smallest denormal: maxval - minval is not zero unless denormals are flushed
    zeros       +0.0 and -0.0 (cv = 0.5; minval and maxval keep the sign of the first row)"""
    rs = np.random.RandomState(100 * n + d)
    rows = np.empty((n, d), dtype=np.float32)
    for c in range(d):
        kind = KINDS[(c + shift) % 7]
        mixed = (rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 3, size=n)).astype(np.float32)
        if kind == "negative":
            col = -1.0 - np.abs(mixed)
        elif kind == "positive":
            col = 1000.0 + np.abs(mixed)
        elif kind == "mixed":
            col = mixed
        elif kind == "constant":
            col = np.full(n, -2.75)
        elif kind == "last_group":
            col = mixed
            if n >= 2:
                col[-2], col[-1] = 3e7, -2e7
        elif kind == "denormal":
            col = np.where(rs.randint(0, 2, size=n) > 0, np.float32(1e-45), np.float32(0.0))
            if n >= 2:
                col[0], col[-1] = 0.0, 1e-45
        else:
            col = np.where(rs.randint(0, 2, size=n) > 0, np.float32(0.0), np.float32(-0.0))
            col[0] = -0.0
            if n >= 2:
                col[1] = 0.0
        rows[:, c] = col
    return rows


def assert_same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_entry_point_equals_the_replay_bit_for_bit(shape, eng):
    """every float of grey, lo and hi: one row, a partial row group, a full one, one row more than a group, 70 full groups
    and a partial one (several workgroups combine their keys); every kind of plane; the whole range and windows inside a
    chunk, across a chunk border, and of the last plane alone"""
    from som_lvq_pak_amd import engine as E
    n, d, shift = shape
    rows = case_rows(n, d, shift)
    cb = E.Codebook(eng, rows)
    want = R.planes(rows)
    if shift == 0 and d >= 4 and n >= 2:
        assert want[1][0] < -1 and want[1][1] >= 1000 and want[1][3] == want[2][3]
    windows = [(0, None)]
    if d >= 3:
        windows.append((1, 2))
    if d >= 6:
        windows.append((3, 3))
    if d % 4:
        windows.append((d - 1, 1))
    for first, count in windows:
        got = E.planes(cb, first, count)
        cnt = d - first if count is None else count
        for name, g, w in zip(("grey", "lo", "hi"), got, want):
            assert_same_bits(g, w[first:first + cnt], (first, count, name))
    cb.close()


@pytest.mark.gpu
def test_planes_of_a_map_in_patch_order(eng):
    """a 16 x 8 map is kept as 8x8 patches on the device: the planes still come in the reference's row order, with the
    first row's zero among equals, and training is seen"""
    from som_lvq_pak_amd import engine as E
    rows = case_rows(128, 9, 0)
    cb = E.Codebook(eng, rows, E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 8)
    for g, w, name in zip(E.planes(cb), R.planes(rows), ("grey", "lo", "hi")):
        assert_same_bits(g, w, name)
    ds = E.Dataset(eng, case_rows(200, 9, 2))
    E.som_train(cb, ds, 300, 0.05, 3.0, batch=1)
    after = cb.download()
    assert not np.array_equal(bits(after), bits(rows))
    for g, w, name in zip(E.planes(cb, 2, 5), R.planes(after, 2, 5), ("grey", "lo", "hi")):
        assert_same_bits(g, w, name)
    ds.close()
    cb.close()


@pytest.mark.gpu
def test_entry_point_refusals(eng):
    from som_lvq_pak_amd import _lib
    from som_lvq_pak_amd import engine as E
    from som_lvq_pak_amd._lib import SomhipError
    rows = case_rows(256, 5, 0)
    shard = E.Codebook(eng, rows[:128], E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 16, row_offset=0, n_global=256)
    inter = E.Codebook(eng, rows[E.shard_units(16, 16, 0, 2)], E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 16, interleave=(0, 2))
    ok = E.Codebook(eng, rows[:70])
    for cb in (shard, inter):
        with pytest.raises(SomhipError, match="shard"):
            E.planes(cb)
    for first, count, word in ((5, 1, "outside"), (-1, 2, "outside"), (3, 3, "outside"), (0, 6, "outside"), (0, 0, "at least 1"),
                               (2, -1, "at least 1")):
        with pytest.raises(SomhipError, match=word):
            E.planes(ok, first, count)
    g = np.zeros((5, 70), dtype=np.float32)
    assert eng.lib.somhip_planes(ok.h, 0, 5, None, None, None) != 0 and b"null" in eng.lib.somhip_last_error()
    assert eng.lib.somhip_planes(None, 0, 5, g.ctypes.data_as(_lib.c_float_p), None, None) != 0
    assert eng.lib.somhip_planes(ok.h, 0, 5, g.ctypes.data_as(_lib.c_float_p), None, None) == 0     # lo and hi may be NULL
    assert_same_bits(g, R.planes(rows[:70])[0], "after the refusals")
    for cb in (shard, inter, ok):
        cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RUNS)
def test_tool_equals_the_reference_byte_for_byte(tag, tools, inputs, tmp_path):
    """the names of the files the tool writes, every one of them outside the procedure bodies, the status and both
    message streams"""
    run = EXPECTED["runs"][tag]
    d = fresh_copy(inputs, tmp_path, run["args"])
    p = run_tool(run["args"], cwd=d)
    assert (p.returncode, p.stdout.decode(), p.stderr.decode()) == (run["returncode"], run["stdout"], run["stderr"])
    assert pictures(d) == sorted(run["files"])
    for name, want in run["files"].items():
        text = open(os.path.join(d, name), encoding="latin-1").read()
        assert text.count("\n} def\n") == (1 if "_tr." in name else 2)      # the project's own procedure bodies are there
        norm = R.normalise(text)
        content = json.loads(json.dumps(R.parse_text(norm)))
        for key in sorted(want["content"]):
            assert content[key] == want["content"][key], (name, key)
        assert R.md5_text(norm) == want["md5"], name


@pytest.mark.gpu
def test_trajectory_of_other_data_sources(tools, inputs, tmp_path, eng):
    """a `gen:` source and the raw fp32 side format (with its masked components) go through the same readers: the
    trajectory is the replay's writer over the engine's own winners of the same rows"""
    from som_lvq_pak_amd import engine as E
    from som_lvq_pak_amd import textio
    d = fresh_copy(inputs, tmp_path, ["-cin", "som_hexa_gaussian.cod", "-din", "ex_masked.dat"])
    codes = textio.read_entries(os.path.join(d, "som_hexa_gaussian.cod"))[0]
    cb = E.Codebook(eng, codes.points, codes.topol, codes.neigh, codes.xdim, codes.ydim)
    masked = textio.read_entries(os.path.join(d, "ex_masked.dat"), skip_empty=False)[0]
    assert run_tool(["-din", "ex_masked.dat", "-dout", "m.f32"], cwd=d, tool="datconv").returncode == 0
    gen_x, _ = E.gen_rows(9, 5, 5, 0, 300)
    for source, ds in (("gen:k=5,dim=5,n=300,seed=9", E.Dataset(eng, gen_x)),
                       ("m.f32", E.Dataset(eng, masked.points, mask=masked.mask))):
        idx, _, ret = E.find_winners(cb, ds)
        win = np.where((ret == 0) | (idx[:, 0] < 0), -1, idx[:, 0])
        assert (win >= 0).all() and len(set(win.tolist())) > 1                     # a path, not a point
        p = run_tool(["-cin", "som_hexa_gaussian.cod", "-din", source, "-plane", "2"], cwd=d)
        assert p.returncode == 0, p.stderr
        assert pictures(d) == ["som_hexa_gaussian_p2.eps", "som_hexa_gaussian_tr.eps"]
        text = R.normalise(open(os.path.join(d, "som_hexa_gaussian_tr.eps"), encoding="latin-1").read())
        assert text == R.trajectory_text(win, codes.xdim, codes.ydim, codes.topol, 0), source
        ds.close()
    cb.close()
