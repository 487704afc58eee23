"""umat: SOM_PAK's U-matrix of a trained map, computed on the GPU, bit for bit.

The real reference enters through tests/golden/umat (written by tests/golden/make_golden_umat.py from the reference's own
umat.c, map.c and median.c; only results are recorded, never its PostScript prologue).  tests/umat_replay.py restates
the reference's arithmetic and its writer in numpy; the CPU tests pin that replay against the recorded runs, the GPU
tests compare the engine's entry point with the replay bit for bit and the tool with the recorded runs byte for byte
outside the prologue and the %%CreationDate: line."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import umat_replay as R
from conftest import GOLDEN, ROOT, synth

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
HOST = os.path.join(ROOT, "som_lvq_pak_amd", "host")
CLI = os.path.join(GOLDEN, "cli")
EXPECTED = json.load(open(os.path.join(GOLDEN, "umat", "expected.json")))
RUNS = sorted(EXPECTED["runs"])
OPERATORS = ["LAB", "ML", "LN", "H", "R", "XSH", "XSR", "NL", "selfont", "swapx", "swapy"]
REDEFINED = ["xstep", "ystep", "radius", "xoff", "yoff", "y", "xoffset", "yoffset", "picwidth", "picheight", "doborder",
             "fontname", "fontsize", "bt", "wt"]


@pytest.fixture(scope="module")
def tools():
    if not os.path.exists(os.path.join(BIN, "umat")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", HOST])
    return BIN


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a directory with every input of the recorded runs: the stored fixtures and the generated ones, md5 checked"""
    import hashlib
    d = str(tmp_path_factory.mktemp("umat_inputs"))
    R.write_generated(d)
    for name, want in EXPECTED["inputs"].items():
        if name not in R.generated_names():
            shutil.copy(os.path.join(CLI, name), os.path.join(d, name))
        assert hashlib.md5(open(os.path.join(d, name), "rb").read()).hexdigest() == want, name
    return d


def run_tool(args, cwd=None, env=None):
    return subprocess.run([os.path.join(BIN, "umat")] + [str(a) for a in args], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, cwd=cwd, env=env)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ CPU side
@pytest.mark.parametrize("tag", RUNS)
def test_replay_reproduces_the_reference(tag, inputs):
    """the numpy replay, walking the reference's case ladders, writes what the real reference wrote: md5 of the
    normalised text, its parsed content, and the two stderr lines of -v 2; the whole-array form writes the same"""
    run = EXPECTED["runs"][tag]
    text, err = R.replay_run(run["args"], inputs, ladder=True)
    got = json.loads(json.dumps(R.parse_text(text)))
    for key in ("numbers", "blocks", "units"):
        assert got[key] == run["content"][key], key
    assert R.md5_text(text) == run["md5"]
    assert err == run["stderr"] and run["returncode"] == 0
    assert R.replay_run(run["args"], inputs, ladder=False) == (text, err)


@pytest.mark.parametrize("topol", [R.HEXA, R.RECT])
def test_whole_array_form_equals_the_ladders(topol):
    """umatrix (entries of a fixed neighbour list that lie inside the matrix) against umatrix_ladder (the cases as the
    reference writes them) at sides 2 and 3, at every y % 4 on both borders, with ties and with the filters"""
    for mx, my, d in ((2, 2, 1), (3, 2, 2), (2, 3, 2), (3, 3, 1), (9, 7, 4), (6, 8, 3), (7, 6, 3)):
        rows = R.gen_rows(mx, my, d, 31 * mx + my)
        rows[2::3] = rows[1::3][:len(rows[2::3])]
        for avg in (False, True):
            for med in (False, True):
                a, mma = R.umatrix(rows, mx, my, topol, avg, med)
                b, mmb = R.umatrix_ladder(rows, mx, my, topol, avg, med)
                assert same_bits(a, b) and mma == mmb, (mx, my, avg, med)


def test_recorded_runs_cover_the_cases(inputs, monkeypatch):
    runs = EXPECTED["runs"]
    for t in ("hexa", "rect"):
        for n in ("gaussian", "bubble"):
            assert runs["plain_%s_%s" % (t, n)]["args"] == ["-cin", "som_%s_%s.cod" % (t, n)]
        md5s = {runs[k + "_" + t]["md5"] for k in ("average", "median", "both")} | {runs["plain_%s_gaussian" % t]["md5"]}
        assert len(md5s) == 4                                              # every filter changes the picture
        for mx, my, d in R.SHAPES:
            assert "gen_%s_%dx%dx%d" % (t, mx, my, d) in runs and "gen_%s_%dx%dx%d_both" % (t, mx, my, d) in runs
    assert runs["plain_hexa_gaussian"]["stderr"].split()[5] == "0.502032"
    assert runs["plain_hexa_gaussian"]["stderr"].split()[-1] == "6.261151"
    several = [un for row in runs["labels_several"]["content"]["units"] for un in row]
    assert [len(names) for names, _ in several] == [1, 2, 1, 0, 3, 1]
    assert several[2][0] == ["f(x)"] and several[4][0] == ["back\\slash", "A", "c)("]
    assert any(names for row in runs["labels_vcal"]["content"]["units"] for names, _ in row)
    assert len(runs["ps_default"]["content"]["numbers"]["translate"]) == 2 and "translate" not in runs["swap"]["content"]["numbers"]
    assert runs["ps_default"]["content"]["numbers"]["translate"][0][2] == "90"          # 12 x 8: landscape by shape
    assert len(runs["ps_best_tall"]["content"]["numbers"]["translate"][0]) == 2            # 4 x 5: portrait by shape
    assert runs["ps_portrait_a3"]["content"]["numbers"]["translate"] != runs["guess_ps"]["content"]["numbers"]["translate"]
    assert runs["guess_ps"]["args"][-2:] == ["-o", "x.ps"] and len(runs["guess_ps"]["content"]["numbers"]["translate"]) == 2
    assert runs["border_thresholds"]["content"]["numbers"]["wt"] == "0.900000"
    assert runs["onlylabs"]["content"]["blocks"] == [] and runs["nolabs_notitle"]["content"]["units"] == []
    assert {c for row in runs["onlylabs"]["content"]["units"] for _, c in row} == {100}
    for tag in ("title_font", "swap"):
        assert runs[tag]["md5"] != runs["plain_rect_gaussian" if tag == "title_font" else "plain_hexa_gaussian"]["md5"]
    # the round_* maps tell a float subtraction from a double one: with the difference taken in double the replay no
    # longer gives the recorded pictures.  (The order of the double sums is the reference's too, but a change of the last
    # bit of a double sum all but never survives the rounding of its root to float.)
    monkeypatch.setattr(R, "_pair", _double_pair)
    changed = [t for t in RUNS if t.startswith("round_") and R.md5_text(R.replay_run(runs[t]["args"], inputs)[0]) != runs[t]["md5"]]
    assert len(changed) == 4, changed


def _double_pair(a, b):
    t = a.astype(np.float64) - b.astype(np.float64)
    acc = np.zeros(t.shape[:-1])
    for k in range(t.shape[-1]):
        acc = acc + t[..., k] * t[..., k]
    return acc


def test_abi_and_kernel_table():
    from som_lvq_pak_amd import _lib
    assert _lib.SIGNATURES["somhip_umatrix"] == (C.c_int, [C.c_void_p, C.c_int, _lib.c_float_p, _lib.c_double_p])
    lib = _lib.load()
    assert hasattr(lib, "somhip_umatrix")
    names = [lib.somhip_kernel_name(i).decode() for i in range(lib.somhip_kernel_count())]
    assert names[0] == "k_scan_exact" and names[25] == "k_sammon_error" and names[26] == "k_class_nearest"
    assert names[27:] == ["k_umat_dist", "k_umat_units", "k_umat_minmax", "k_umat_scale", "k_umat_average", "k_umat_median"]
    assert len(names) <= 64                                                # bench.py selects kernels by bit
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r"SOMHIP_UMAT_AVERAGE = 1, SOMHIP_UMAT_MEDIAN = 2", hdr)
    from som_lvq_pak_amd import engine as E
    assert (E.UMAT_AVERAGE, E.UMAT_MEDIAN) == (1, 2)


def test_tool_usage_and_refusals_without_a_gpu(tools, tmp_path):
    p = run_tool(["-help"])
    assert p.returncode == 0 and b"MI355X" in p.stdout
    for flag in ("-cin", "-o", "-eps", "-ps", "-portrait", "-landscape", "-paper", "-border", "-onlylabs", "-nolabs", "-W",
                 "-B", "-title", "-notitle", "-font", "-fontsize", "-average", "-median", "-headerfile", "UMAT_HEADERFILE",
                 "-swapx", "-swapy", "-v"):
        assert flag.encode() in p.stdout, flag
    p = run_tool(["-o", "a.eps"])
    assert p.returncode == 255 and b"Can't find asked option -cin" in p.stderr
    masked = tmp_path / "masked.cod"
    masked.write_text("2 hexa 2 2 bubble\n1 2\n3 x\n5 6\n7 8\n")
    one = tmp_path / "one.cod"
    one.write_text("2 rect 1 3 bubble\n1 2\n3 4\n5 6\n")
    short = tmp_path / "short.cod"
    short.write_text("2 rect 2 2 bubble\n1 2\n3 4\n5 6\n")
    for path, word in ((masked, b"masked"), (os.path.join(CLI, "lvq_olvq1.cod"), b"not a map"), (one, b"1 x 3"),
                       (short, b"3 entries")):
        p = run_tool(["-cin", path])
        assert p.returncode == 1 and word in p.stderr and p.stdout == b"", (path, p.stderr)
        assert b"HIP" not in p.stderr and b"hip" not in p.stderr           # refused before an engine was asked for
    p = run_tool(["-cin", os.path.join(CLI, "som_hexa_bubble.cod"), "-paper", "B5"])
    assert p.returncode == 1 and b"Unknown paper type: B5" in p.stderr


def prologue_text():
    src = open(os.path.join(HOST, "umat_prologue.h")).read()
    body = src[src.index("umat_prologue[] = {"):]
    lines = re.findall(r'^\s*"((?:[^"\\]|\\.)*)",\s*$', body, flags=re.M)
    assert len(lines) >= 20 and body.rstrip().endswith("};")
    assert all(set(re.findall(r"\\(.)", ln)) <= {"n"} for ln in lines)
    return "".join(ln.replace("\\n", "\n") for ln in lines)


def test_prologue_is_well_formed():
    text = prologue_text()
    assert "(" not in text and ")" not in text                            # no strings, so braces count as braces
    code = "\n".join(ln for ln in text.split("\n") if not ln.startswith("%"))
    assert "%" not in code
    depth = 0
    for ch in code:
        depth += {"{": 1, "}": -1}.get(ch, 0)
        assert depth >= 0
    assert depth == 0
    tokens = code.replace("{", " { ").replace("}", " } ").split()
    assert tokens.count("begin") == 1 and tokens[tokens.index("begin") - 1] == "dict" and "end" not in tokens
    assert tokens.index("begin") < tokens.index("def")                     # everything is defined inside that dictionary
    procs = set(re.findall(r"/(\w+)\s*\{", code))
    assert set(OPERATORS) <= procs, set(OPERATORS) - procs
    values = set(re.findall(r"/(\w+)\s+[^\s{}]+\s+def\b", code))
    assert set(REDEFINED) <= values, set(REDEFINED) - values
    # every name a procedure uses is an operator of the language, a procedure or a value of the prologue
    language = set("""def dict begin moveto lineto rlineto closepath newpath fill stroke arc gsave grestore setgray setlinewidth
        show stringwidth findfont scalefont setfont currentpoint dup pop exch roll mod div mul add sub neg abs cos sin eq lt gt or
        if ifelse for true false""".split())
    for tok in tokens:
        if tok in "{}" or tok.startswith("/") or re.fullmatch(r"-?\d+(\.\d+)?", tok):
            continue
        assert tok in language or tok in procs or tok in values, tok
    # and the body emits nothing else: the operator words of a recorded-style text are all defined
    body = R.body_text(np.zeros((3, 3), np.float32), 2, 2, 1, R.HEXA, 1, [[1], [1, 1], [], []], ["", "a"], "t",
                       dict(R.OPTIONS, swapx=True, swapy=True))
    body = R.normalise(body).split("%%EndComments\n")[1]
    words = set(re.findall(r"(?<![/\w(])([A-Za-z]\w*)(?![\w)])", re.sub(r"\([^)]*\)|^%.*$", "", body, flags=re.M)))
    assert words - {"def", "true", "false", "end", "Helvetica"} <= procs | values, words


# ------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


SHAPES = [(2, 2, 1), (2, 3, 4), (3, 2, 4), (5, 4, 3), (4, 5, 5), (64, 3, 7), (65, 3, 7), (3, 65, 7), (33, 31, 130),
          (128, 128, 16)]


def case_rows(mx, my, d, duplicated):
    """seeded normal rows scaled by 10^uniform(-3, 3) per row, so that the float subtraction rounds; `duplicated`: every
    third row equals its predecessor (ties among the entries, distances of exactly 0)"""
    rs = np.random.RandomState(1000 * mx + 10 * my + d)
    rows = (rs.standard_normal((mx * my, d)) * 10.0 ** rs.uniform(-3, 3, size=(mx * my, 1))).astype(np.float32)
    if duplicated:
        rows[2::3] = rows[1::3][:len(rows[2::3])]
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("topol", [R.HEXA, R.RECT], ids=["hexa", "rect"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_entry_point_equals_the_replay_bit_for_bit(shape, topol, eng):
    """every float of the matrix and both of minmax, filters 0 to 3: the smallest map, sides 2 and 3, an even and an odd
    ydim, a dim that is no multiple of 4, a row group that ends inside and at the end of a lattice row, more lattice rows
    than a row group, 130 components, and 128 x 128 (8x8 patch order, many workgroups)"""
    from som_lvq_pak_amd import engine as E
    mx, my, d = shape
    for duplicated in (False, True):
        rows = case_rows(mx, my, d, duplicated)
        cb = E.Codebook(eng, rows, topol, E.NEIGH_BUBBLE, mx, my)
        base, mm = R.scale(R.unit_medians(R.distances(rows, mx, my, topol), topol))
        if duplicated and mx * my >= 6:
            assert mm[0] == 0.0
        for avg in (False, True):
            for med in (False, True):
                want = R.average(base, topol) if avg else base
                want = R.median(want, topol) if med else want
                got, got_mm = E.umatrix(cb, average=avg, median=med)
                assert np.array_equal(np.array(got_mm).view(np.uint64), np.array(mm).view(np.uint64)), (duplicated, got_mm, mm)
                bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                assert got.shape == want.shape and len(bad) == 0, (duplicated, avg, med, len(bad), bad[:5].tolist())
        cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("topol", [R.HEXA, R.RECT], ids=["hexa", "rect"])
def test_matrix_of_a_trained_codebook_is_the_matrix_of_its_rows(topol, eng):
    """somhip_umatrix reads the rows as they are on the device after som_train (a 16 x 8 map is kept in 8x8 patch
    order): the same matrix as that of the downloaded rows in a fresh codebook, and as the replay's"""
    from som_lvq_pak_amd import engine as E
    x, _ = synth(5, 400, 6)
    rs = np.random.RandomState(3)
    cb = E.Codebook(eng, x[rs.randint(0, 400, size=128)], topol, E.NEIGH_GAUSSIAN, 16, 8)
    ds = E.Dataset(eng, x)
    before, _ = E.umatrix(cb)
    E.som_train(cb, ds, 600, 0.05, 5.0, batch=1)
    got, mm = E.umatrix(cb, average=True, median=True)
    rows = cb.download()
    fresh = E.Codebook(eng, rows, topol, E.NEIGH_GAUSSIAN, 16, 8)
    again, mm2 = E.umatrix(fresh, average=True, median=True)
    want, mm3 = R.umatrix(rows, 16, 8, topol, True, True)
    assert same_bits(got, again) and same_bits(got, want) and mm == mm2 == mm3
    assert not same_bits(before, E.umatrix(cb)[0])                          # training moved the rows
    for h in (cb, fresh, ds):
        h.close()


@pytest.mark.gpu
def test_entry_point_refusals(eng):
    from som_lvq_pak_amd import engine as E
    from som_lvq_pak_amd._lib import SomhipError
    rows = case_rows(16, 16, 3, False)
    shard = E.Codebook(eng, rows[:128], E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 16, row_offset=0, n_global=256)
    inter = E.Codebook(eng, rows[E.shard_units(16, 16, 0, 2)], E.TOPOL_HEXA, E.NEIGH_BUBBLE, 16, 16, interleave=(0, 2))
    lvq = E.Codebook(eng, rows[:10], labels=np.ones(10, dtype=np.int32))
    line = E.Codebook(eng, rows[:7], E.TOPOL_RECT, E.NEIGH_BUBBLE, 1, 7)
    flat = E.Codebook(eng, np.ones((12, 3), dtype=np.float32), E.TOPOL_RECT, E.NEIGH_BUBBLE, 4, 3)
    ok = E.Codebook(eng, rows[:12], E.TOPOL_RECT, E.NEIGH_BUBBLE, 4, 3)
    for cb, word in ((shard, "shard"), (inter, "shard"), (lvq, "not a map"), (line, "at least 2"), (flat, "divide by zero")):
        with pytest.raises(SomhipError, match=word):
            E.umatrix(cb)
    u = np.zeros((5, 7), dtype=np.float32)
    from som_lvq_pak_amd import _lib
    for bits in (4, 7, -1):
        assert eng.lib.somhip_umatrix(ok.h, bits, u.ctypes.data_as(_lib.c_float_p), None) != 0
        assert b"filter bits" in eng.lib.somhip_last_error()
    assert eng.lib.somhip_umatrix(ok.h, 3, u.ctypes.data_as(_lib.c_float_p), None) == 0      # minmax may be NULL
    assert same_bits(u, R.umatrix(rows[:12], 4, 3, R.RECT, True, True)[0])
    for cb in (shard, inter, lvq, line, flat, ok):
        cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RUNS)
def test_tool_equals_the_reference_byte_for_byte(tag, tools, inputs):
    """everything outside the prologue and the %%CreationDate: line, and the stderr text of -v 2"""
    run = EXPECTED["runs"][tag]
    env = {k: v for k, v in os.environ.items() if k != "UMAT_HEADERFILE"}
    p = run_tool(run["args"] + ["-v", "2"], cwd=inputs, env=env)
    assert p.returncode == run["returncode"] == 0, p.stderr
    text = p.stdout.decode("latin-1")
    if "-o" in run["args"]:
        assert text == ""
        text = open(os.path.join(inputs, run["args"][run["args"].index("-o") + 1]), encoding="latin-1").read()
    assert text.count("%%CreationDate: ") == (2 if "%!PS-Adobe-2.0" in text else 1)
    norm = R.normalise(text)
    got = json.loads(json.dumps(R.parse_text(norm)))
    for key in ("numbers", "blocks", "units"):
        assert got[key] == run["content"][key], key
    assert R.md5_text(norm) == run["md5"]
    assert p.stderr.decode() == run["stderr"]
    assert text.split("%%EndComments\n")[1].split("\n/radius ")[0] + "\n" == prologue_text()


@pytest.mark.gpu
def test_headerfile_is_copied_verbatim(tools, inputs, tmp_path):
    header = tmp_path / "own_header.ps"
    header.write_bytes(b"% a header of the user's own\n/umat 10 dict def umat begin\n\n  (odd \\( bytes) pop \xe9\n")
    other = tmp_path / "other.ps"
    other.write_bytes(b"% from the environment\n")
    env = dict(os.environ, UMAT_HEADERFILE=str(other))
    for args, want in ((["-headerfile", header], header), ([], other)):
        p = run_tool(["-cin", "som_rect_bubble.cod"] + args, cwd=inputs, env=env)
        assert p.returncode == 0, p.stderr
        assert p.stdout.split(b"%%EndComments\n")[1].split(b"\n/radius ")[0] + b"\n" == want.read_bytes()
        assert R.md5_text(R.normalise(p.stdout.decode("latin-1"))) == EXPECTED["runs"]["plain_rect_bubble"]["md5"]
    p = run_tool(["-cin", "som_rect_bubble.cod", "-headerfile", tmp_path / "missing.ps"], cwd=inputs)
    assert p.returncode == 1 and b"can't read PS header file" in p.stderr
