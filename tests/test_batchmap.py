"""The batch map (K8: somhip_som_batchmap and its two stages, engine.som_batchmap / batchmap_sums / batchmap_combine, the
bsom tool) against the CPU replay in batchmap_replay.py.

The sums stage is compared exactly: hits as integers, sums by bit pattern with the replay's data-order fp64 chains.  The
combine is compared against a bound that is derived, not measured: with q = N / D formed in np.longdouble, a device row
must satisfy |m - q| <= ulp32(q) / 2 + (2 * units + 16) * 2^-52 * A / D, A = sum_j h |S_j| -- the rounding to float, and
at most two fp64 roundings per term of a sum over `units` terms in any order, 16 more for the weight's exp, the division
and slack.  Rows whose neighbourhood holds no sample keep their bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batchmap_replay as R
from conftest import ROOT

HEXA, RECT = R.TOPOL_HEXA, R.TOPOL_RECT
BUBBLE, GAUSSIAN = R.NEIGH_BUBBLE, R.NEIGH_GAUSSIAN
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("bsom", "qerror")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    for name in ("somhip_som_batchmap", "somhip_debug_batchmap_sums", "somhip_debug_batchmap_combine", "somhip_batchmap_timing"):
        assert hasattr(lib, name), name
    S = _lib.SIGNATURES
    assert S["somhip_som_batchmap"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.BatchmapParams), _lib.c_float_p])
    assert S["somhip_debug_batchmap_sums"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _lib.c_u32_p, _lib.c_double_p])
    assert S["somhip_debug_batchmap_combine"] == (C.c_int, [C.c_void_p, C.c_float, _lib.c_u32_p, _lib.c_double_p])
    assert S["somhip_batchmap_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.BatchmapParams._fields_] == ["epochs", "radius", "start_epoch", "count", "first", "n"]
    assert C.sizeof(_lib.BatchmapParams) == 48
    for name in ("som_batchmap", "batchmap_sums", "batchmap_combine"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "batchmap_timing")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int somhip_som_batchmap(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out );" in hdr
    assert ("int somhip_debug_batchmap_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, uint32_t *hits, "
            "double *sums);") in hdr
    assert "int somhip_debug_batchmap_combine(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums);" in hdr
    assert "int somhip_batchmap_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);" in hdr
    m = re.search(r"typedef struct somhip_batchmap_params \{(.*?)\} somhip_batchmap_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int64_t epochs; float radius; int64_t start_epoch, count; int64_t first, n;"


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 3)(), (C.c_double * 3)()
    assert lib.somhip_batchmap_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_batchmap_timing: null engine"


def test_bsom_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("bsom", "-help")
    assert p.returncode == 0 and p.stdout.startswith("bsom - ") and "-epochs" in p.stdout and "-radius" in p.stdout
    cod = tmp_path / "m.cod"
    cod.write_text("2 hexa 2 2 bubble\n0 0\n1 0\n0 1\n1 1\n")
    dat = tmp_path / "d.dat"
    dat.write_text("2\n0.25 0.5\n0.75 0.5\n")
    out = tmp_path / "o.cod"
    for args, word in ((("-epochs", 0, "-radius", 2), "-epochs"), (("-epochs", -3, "-radius", 2), "-epochs"),
                       (("-epochs", 2, "-radius", 0.5), "-radius"), (("-epochs", 2, "-radius", "nan"), "-radius")):
        p = run("bsom", "-cin", cod, "-din", dat, "-cout", out, *args)
        assert p.returncode == 1 and p.stderr.startswith("bsom: " + word), (args, p.stderr)
        assert not out.exists()
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3\n4 5 6\n")
    p = run("bsom", "-cin", cod, "-din", dim3, "-cout", out, "-epochs", 2, "-radius", 2)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    xcod = tmp_path / "x.cod"
    xcod.write_text("2 hexa 2 2 bubble\nx 0\n1 0\n0 1\n1 1\n")
    p = run("bsom", "-cin", xcod, "-din", dat, "-cout", out, "-epochs", 2, "-radius", 2)
    assert p.returncode == 1 and "masked components" in p.stderr
    xdat = tmp_path / "x.dat"
    xdat.write_text("2\nx 0.5\n0.75 0.5\n")
    p = run("bsom", "-cin", cod, "-din", xdat, "-cout", out, "-epochs", 2, "-radius", 2)
    assert p.returncode == 1 and "masked components" in p.stderr
    lvq = tmp_path / "l.cod"
    lvq.write_text("2\n0 0 a\n1 1 b\n")
    p = run("bsom", "-cin", lvq, "-din", dat, "-cout", out, "-epochs", 2, "-radius", 2)
    assert p.returncode == 1 and "not a map file" in p.stderr
    assert not out.exists()


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


def mixture(seed, n, d, xdim, ydim, noise=0.4):
    """test_map_quality.py's generator, restated: a map laid out as a noisy sheet in the data space and data scattered
    around the sheet"""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((2, d)).astype(np.float32)
    u = np.arange(xdim * ydim)
    pos = np.stack([u % xdim, u // xdim], axis=1).astype(np.float32)
    codes = (pos @ v + noise * rs.standard_normal((xdim * ydim, d))).astype(np.float32)
    at = (rs.uniform(size=(n, 2)) * [xdim, ydim]).astype(np.float32)
    x = (at @ v + 0.5 * rs.standard_normal((n, d))).astype(np.float32)
    return x, codes


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_sums(got, want):
    gh, gs = got
    wh, ws = want
    assert gh.dtype == np.uint32 and gs.dtype == np.float64
    assert np.array_equal(gh, wh), np.nonzero(gh != wh)[0][:8]
    assert np.array_equal(bits(gs), bits(ws)), np.argwhere(bits(gs) != bits(ws))[:8]


def check_sums(E, eng, oracle, codes, x, topol, xdim, ydim, windows):
    cb = E.Codebook(eng, codes, topol, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x)
    win, _ = R.winners(oracle, codes, x)
    out = []
    for first, n in windows:
        got = E.batchmap_sums(cb, ds, first, n)
        same_sums(got, R.sums(win, x, codes.shape[0], first, n))
        assert int(got[0].sum()) == n
        out.append(got)
    assert np.array_equal(bits(cb.download()), bits(codes))          # the stage writes no row
    cb.close(); ds.close()
    return win, out


# ---- the sums, exact
@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol", [(1, 1, HEXA), (2, 1, RECT), (63, 1, HEXA), (1, 64, RECT), (13, 5, HEXA),
                                             (257, 1, RECT), (1030, 1, HEXA)])
def test_sums_units(E, eng, oracle, xdim, ydim, topol):
    """1, 2, 63, 64, 65, 257 and 1030 units, over 700 samples and over one"""
    x, codes = mixture(100 + xdim * ydim, 700, 3, xdim, ydim)
    check_sums(E, eng, oracle, codes, x, topol, xdim, ydim, [(0, 700), (0, 1), (699, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 63, 64, 65, 129])
def test_sums_dims(E, eng, oracle, dim):
    """a sums workgroup has 64 columns and the counts are column `dim`: 63 fills one workgroup with them, 64 puts them
    alone into a second, 129 needs a third"""
    x, codes = mixture(200 + dim, 700, dim, 13, 5)
    check_sums(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 700)])


@pytest.mark.gpu
def test_sums_chunks_and_wrap(E, eng, oracle):
    """the winner search cuts a run into chunks of 4096 samples: one fewer, one more; runs that start near the end of the
    data and wrap, once and twice"""
    x, codes = mixture(7, 6000, 5, 13, 5)
    check_sums(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 4095), (0, 4096), (0, 4097), (5990, 700), (5990, 4097), (3, 12003)])


@pytest.mark.gpu
def test_sums_one_unit_takes_everything(E, eng, oracle):
    """the longest chain: every sample of a run of more than a chunk on one unit of a 13 x 5 map"""
    x, codes = mixture(8, 4500, 5, 13, 5)
    codes = codes + np.float32(1000.0)
    codes[37] = x.mean(axis=0)
    win, (got,) = check_sums(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 4500)])
    assert (win == 37).all() and got[0][37] == 4500


@pytest.mark.gpu
def test_sums_most_units_empty(E, eng, oracle):
    x, codes = mixture(9, 700, 4, 40, 30)
    codes = codes + np.float32(500.0)
    for u in (0, 611, 1199):
        codes[u] = x[u % 7]
    win, (got,) = check_sums(E, eng, oracle, codes, x, RECT, 40, 30, [(0, 700)])
    assert set(np.nonzero(got[0])[0]) <= {0, 611, 1199} and (got[1][got[0] == 0] == 0).all()


@pytest.mark.gpu
def test_sums_duplicated_rows_lowest_index_wins(E, eng, oracle):
    x, codes = mixture(10, 700, 5, 13, 5)
    codes[40] = codes[12]
    codes[64] = codes[12]
    codes[3] = codes[50]
    win, (got,) = check_sums(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 700)])
    assert got[0][12] > 0 and got[0][3] > 0
    assert got[0][40] == 0 and got[0][64] == 0 and got[0][50] == 0


@pytest.mark.gpu
def test_sums_twice_the_same_bits(E, eng):
    x, codes = mixture(11, 3000, 17, 16, 16)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 16, 16)
    ds = E.Dataset(eng, x)
    a = E.batchmap_sums(cb, ds, 5, 2999)
    b = E.batchmap_sums(cb, ds, 5, 2999)
    same_sums(a, b)
    cb.close(); ds.close()


# ---- the combine, within the derived bound
def combine_inputs(seed, units, dim, corner=False):
    rs = np.random.RandomState(seed)
    codes = rs.standard_normal((units, dim)).astype(np.float32)
    if corner:
        hits = np.zeros(units, dtype=np.uint32)
        hits[0] = 7
    else:
        hits = rs.randint(0, 6, size=units).astype(np.uint32)
        hits[rs.uniform(size=units) < 0.3] = 0
    # sums with mixed signs, doubles that are no floats
    S = rs.standard_normal((units, dim)) * np.where(hits > 0, hits, 0)[:, None] * rs.choice([-3.0, 0.25, 1.0, 40.0], size=(units, 1))
    return codes, hits, S


def check_combine(E, eng, codes, hits, S, topol, neigh, xdim, ydim, r):
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_combine(cb, r, hits, S)
    got = cb.download()
    cb.close()
    q, D, bound = R.combine(R.weights(topol, neigh, xdim, ydim, r), hits, S)
    live = D > 0
    what = (topol, neigh, xdim, ydim, codes.shape[1], float(r))
    assert np.array_equal(bits(got[~live]), bits(codes[~live])), what
    err = np.abs(got[live].astype(np.longdouble) - q[live])
    bad = err > bound[live]
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), np.argwhere(bad)[:4])
    return live


MAPS = [(1, 1), (2, 1), (1, 2), (13, 5), (16, 16), (9, 33), (40, 3), (32, 8), (8, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim", MAPS)
@pytest.mark.parametrize("dim", [17, 64])
def test_combine_maps(E, eng, xdim, ydim, dim):
    """bubble and gaussian on hexa and rect lattices at radius 1, 2.5 and one larger than the map; sides that are no whole
    8 x 8 patches or MFMA tiles, and (32 x 8, 8 x 24) maps stored in patches, three of them in a row"""
    codes, hits, S = combine_inputs(1000 * xdim + ydim + dim, xdim * ydim, dim)
    for topol in (HEXA, RECT):
        for neigh in (BUBBLE, GAUSSIAN):
            for r in (1.0, 2.5, float(xdim + ydim + 3)):
                check_combine(E, eng, codes, hits, S, topol, neigh, xdim, ydim, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [15, 16, 17, 63, 64, 65])
def test_combine_dims(E, eng, dim):
    """the counts column on either side of a 16-column tile edge, and of a workgroup's 64 columns"""
    codes, hits, S = combine_inputs(77 + dim, 9 * 33, dim)
    for topol, neigh, r in ((HEXA, BUBBLE, 2.5), (RECT, GAUSSIAN, 2.5), (HEXA, GAUSSIAN, 1.0), (RECT, BUBBLE, 50.0)):
        check_combine(E, eng, codes, hits, S, topol, neigh, 9, 33, r)


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim", [(13, 5), (9, 33), (32, 8), (8, 24)])
def test_combine_hits_in_one_corner(E, eng, xdim, ydim):
    """bubble, radius 1, every sample on unit 0: only its neighbours have a denominator, every other row keeps its bits"""
    codes, hits, S = combine_inputs(5, xdim * ydim, 16, corner=True)
    for topol, nb in ((HEXA, {0, 1, xdim}), (RECT, {0, 1, xdim})):
        live = check_combine(E, eng, codes, hits, S, topol, BUBBLE, xdim, ydim, 1.0)
        assert set(np.nonzero(live)[0]) == nb


@pytest.mark.gpu
def test_combine_twice_the_same_bits(E, eng):
    codes, hits, S = combine_inputs(6, 9 * 33, 65)
    out = []
    for _ in range(2):
        cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 33)
        E.batchmap_combine(cb, 2.5, hits, S)
        out.append(cb.download())
        cb.close()
    assert np.array_equal(bits(out[0]), bits(out[1]))


# ---- whole runs
@pytest.fixture(scope="module")
def small_run():
    return mixture(21, 1500, 6, 13, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("topol,neigh", [(HEXA, BUBBLE), (RECT, GAUSSIAN)])
def test_epochs_in_one_call_or_many_and_twice(E, eng, small_run, topol, neigh):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    runs = []
    for how in ("one", "one", "many"):
        cb = E.Codebook(eng, codes, topol, neigh, 13, 5)
        if how == "one":
            q = E.som_batchmap(cb, ds, 5, 4.0)
        else:
            q = np.concatenate([E.som_batchmap(cb, ds, 5, 4.0, start_epoch=t, count=1) for t in range(5)])
        runs.append((cb.download(), q))
        cb.close()
    ds.close()
    assert q.dtype == np.float32 and q.shape == (5,)
    for rows, q in runs[1:]:
        assert np.array_equal(bits(rows), bits(runs[0][0])) and np.array_equal(bits(q), bits(runs[0][1]))
    assert not np.array_equal(bits(runs[0][0]), bits(codes))


@pytest.mark.gpu
@pytest.mark.parametrize("topol,neigh", [(HEXA, GAUSSIAN), (RECT, BUBBLE)])
def test_an_epoch_is_its_two_stages(E, eng, oracle, small_run, topol, neigh):
    """som_batchmap == batchmap_sums then batchmap_combine at r_t, by bits; the epoch also lies where the float64 replay
    puts it, and its qerror is the replay's chain"""
    x, codes = small_run
    ds = E.Dataset(eng, x)
    a = E.Codebook(eng, codes, topol, neigh, 13, 5)
    b = E.Codebook(eng, codes, topol, neigh, 13, 5)
    for t in (0, 1, 2):
        r = E.batchmap_radius(3.5, 3, t)
        assert bits(np.float32(r)) == bits(R.radius_at(3.5, 3, t))
        before = a.download()
        q = E.som_batchmap(a, ds, 3, 3.5, start_epoch=t, count=1, first=11, n=1400)
        hits, S = E.batchmap_sums(b, ds, 11, 1400)
        E.batchmap_combine(b, r, hits, S)
        rows = a.download()
        assert np.array_equal(bits(rows), bits(b.download()))
        want, wq = R.epoch(oracle, before, x, topol, neigh, 13, 5, r, 11, 1400)
        assert bits(q[0]) == bits(wq)
        assert np.allclose(rows, want, rtol=1e-6, atol=1e-6)
    assert bits(np.float32(E.batchmap_radius(3.5, 3, 0))) == bits(np.float32(3.5))
    a.close(); b.close(); ds.close()


@pytest.mark.gpu
def test_qerror_is_the_qerror_routes_figure(E, eng, small_run):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    for t in range(3):
        want = E.map_quality(cb, ds)[0]["qerror"]
        _, diff, ret = E.find_winners(cb, ds)
        tool = np.float32(E.qerror_sum(diff, ret))
        q = E.som_batchmap(cb, ds, 3, 3.0, start_epoch=t, count=1)
        assert bits(q[0]) == bits(np.float32(want)) == bits(tool)
    assert E.som_batchmap(cb, ds, 3, 3.0, qerror=False) is None
    cb.close(); ds.close()


@pytest.mark.gpu
def test_the_map_gets_better(E, eng):
    """2000 x 8 mixture data, 12 x 8 hexa gaussian, 10 epochs from radius 6: the last epoch starts from a lower
    quantization error than the first.  The map starts untrained, as randinit leaves one: uniform in the data's bounding
    box.  (The generator's own map is no such start: it already lies along the data's sheet with less noise, 0.4, than the
    data have around it, 0.5, and a gaussian neighbourhood that ends at radius 1.5 smooths it: from that map the figures
    were 3619.2, 12097.8, 9987.4, 9388.5, 8639.6, 7865.1, 7039.5, 6170.7, 5332.4, 4582.4 -- falling from the first
    smoothing on, never below the start.)"""
    x, _ = mixture(31, 2000, 8, 12, 8)
    rs = np.random.RandomState(32)
    lo, hi = x.min(axis=0), x.max(axis=0)
    codes = (lo + (hi - lo) * rs.uniform(size=(12 * 8, 8))).astype(np.float32)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 12, 8)
    q = E.som_batchmap(cb, ds, 10, 6.0)
    assert np.isfinite(q).all() and q[-1] < q[0], q
    cb.close(); ds.close()


@pytest.mark.gpu
def test_stage_timing_counts_launches(E, eng, small_run):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 13, 5)
    eng.timing(True)
    eng.timing_reset()
    E.som_batchmap(cb, ds, 2, 3.0, qerror=False)
    t = eng.batchmap_timing()
    eng.timing(False)
    assert t["k_batchmap_sums"][0] == 2 and t["k_batchmap_combine"][0] == 4 and t["group"][0] == 6   # (table + combine; winners, scan, sort)
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng, small_run):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    lvq = E.Codebook(eng, codes, E.TOPOL_LVQ)
    shard = E.Codebook(eng, codes[:26], HEXA, BUBBLE, 13, 5, row_offset=13, n_global=65)
    other = E.Dataset(eng, x[:, :5])

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    who = "somhip_som_batchmap"
    refused(lambda: E.som_batchmap(cb, masked, 3, 2.0), who, "masked components")
    refused(lambda: E.som_batchmap(shard, ds, 3, 2.0), who, "sharded")
    refused(lambda: E.som_batchmap(lvq, ds, 3, 2.0), who, "without a lattice")
    refused(lambda: E.som_batchmap(cb, other, 3, 2.0), who, "dimension")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, n=2 ** 32), who, "32-bit")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, n=0), who, "n 0")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, n=-5), who, "n -5")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, first=-1), who, "first row")
    refused(lambda: E.som_batchmap(cb, ds, 0, 2.0, count=0), who, "epochs 0")
    refused(lambda: E.som_batchmap(cb, ds, 3, 0.5), who, "radius")
    refused(lambda: E.som_batchmap(cb, ds, 3, float("nan")), who, "radius")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, start_epoch=-1, count=1), who, "outside")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, start_epoch=2, count=2), who, "outside")
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0, start_epoch=3, count=1), who, "outside")
    who = "somhip_debug_batchmap_sums"
    refused(lambda: E.batchmap_sums(cb, masked), who, "masked components")
    refused(lambda: E.batchmap_sums(shard, ds), who, "sharded")
    refused(lambda: E.batchmap_sums(lvq, ds), who, "without a lattice")
    refused(lambda: E.batchmap_sums(cb, ds, 0, 0), who, "n 0")
    who = "somhip_debug_batchmap_combine"
    hits, S = np.ones(65, dtype=np.uint32), np.ones((65, 6))
    refused(lambda: E.batchmap_combine(lvq, 2.0, hits, S), who, "without a lattice")
    refused(lambda: E.batchmap_combine(shard, 2.0, hits[:26], S[:26]), who, "sharded")
    refused(lambda: E.batchmap_combine(cb, -1.0, hits, S), who, "radius")
    for c, rows in ((cb, codes), (lvq, codes), (shard, codes[:26])):
        assert np.array_equal(bits(c.download()), bits(rows))
    for o in (cb, lvq, shard, ds, masked, other):
        o.close()


# ---- the tool
@pytest.mark.gpu
def test_bsom_writes_the_engines_map(E, eng, tools, tmp_path):
    from som_lvq_pak_amd import textio
    rs = np.random.RandomState(41)
    x = (np.round(rs.standard_normal((300, 4)) * 16) / 16).astype(np.float32)       # values that "%g" keeps
    codes = (np.round(rs.standard_normal((6 * 5, 4)) * 16) / 16).astype(np.float32)
    dat, cod, out = tmp_path / "d.dat", tmp_path / "m.cod", tmp_path / "o.cod"
    d = textio.Entries()
    d.dim, d.points = 4, x
    textio.write_entries(str(dat), d)
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = 4, HEXA, GAUSSIAN, 6, 5, codes
    textio.write_entries(str(cod), m)
    assert np.array_equal(textio.read_entries(str(dat))[0].points, x) and np.array_equal(textio.read_entries(str(cod))[0].points, codes)

    p = run("bsom", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 4, "-radius", 3, "-v")
    assert p.returncode == 0, p.stderr
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 6, 5)
    ds = E.Dataset(eng, x)
    q = E.som_batchmap(cb, ds, 4, 3.0)
    rows = cb.download()
    cb.close(); ds.close()
    got = textio.read_entries(str(out))[0]
    assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (4, HEXA, GAUSSIAN, 6, 5)
    printed = np.array([[np.float32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=np.float32)
    assert np.array_equal(bits(got.points), bits(printed))
    lines = p.stdout.strip().split("\n")
    assert lines == ["epoch %d radius %.9g qerror %.9g" % (t, float(E.batchmap_radius(3.0, 4, t)), float(q[t])) for t in range(4)]
    # without -v: no lines, the same file; a raw fp32 copy of the data: the same file
    out2 = tmp_path / "o2.cod"
    p = run("bsom", "-cin", cod, "-din", dat, "-cout", out2, "-epochs", 4, "-radius", 3)
    assert p.returncode == 0 and p.stdout == "" and out2.read_bytes() == out.read_bytes()
    raw, out3 = tmp_path / "d.f32", tmp_path / "o3.cod"
    assert run("datconv", "-din", dat, "-dout", raw).returncode == 0
    p = run("bsom", "-cin", cod, "-din", raw, "-cout", out3, "-epochs", 4, "-radius", 3)
    assert p.returncode == 0 and out3.read_bytes() == out.read_bytes()
    out4 = tmp_path / "o4.cod"
    p = run("bsom", "-cin", cod, "-din", "gen:k=3,dim=4,n=500,seed=5", "-cout", out4, "-epochs", 2, "-radius", 2, "-v")
    assert p.returncode == 0 and len(p.stdout.strip().split("\n")) == 2 and out4.exists()
