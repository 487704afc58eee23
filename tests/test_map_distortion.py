"""Map distortion (K1d: somhip_distortion_*, engine.Distortion / map_distortion / distortion_evaluate, somqual -distortion)
against the CPU replay in map_distortion_replay.py.

The accumulate stage is compared exactly: hits as integers, the sums S and Q by bit pattern with the replay's data-order
fp64 chains, for any cut of the data.  The evaluate stage is compared against bounds that are derived, not measured
(map_distortion_replay.c_unit / c_total / chain_extra): with e_j and E formed in np.longdouble,
|e_j - ref| <= c_unit * 2^-52 * R_j and |E - ref| <= c_total * 2^-52 * sum_j R_j, R_j the sum of the absolute values of the
terms of e_j.  Units whose neighbourhood holds no sample give exactly 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_distortion_replay as R
from batchmap_replay import NEIGH_BUBBLE as BUBBLE, NEIGH_GAUSSIAN as GAUSSIAN, TOPOL_HEXA as HEXA, TOPOL_RECT as RECT
from conftest import GOLDEN, ROOT, read_cod

ld = np.longdouble
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
DATA = os.path.join(GOLDEN, "data", "ex.dat")
MAP = os.path.join(GOLDEN, "cli", "som_hexa_bubble.cod")
NAMES = ("somhip_distortion_create", "somhip_distortion_destroy", "somhip_distortion_clear", "somhip_distortion_accumulate",
         "somhip_distortion_evaluate", "somhip_distortion_read", "somhip_debug_distortion_evaluate", "somhip_distortion_timing")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("somqual", "datconv")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


# ------------------------------------------------------------------------------------------------ without a GPU
def test_header_export_and_signatures_agree(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, hdr), name
    S, vp, dp = _lib.SIGNATURES, C.c_void_p, _lib.c_double_p
    tot = C.POINTER(_lib.DistortionTotals)
    assert S["somhip_distortion_create"] == (C.c_int, [vp, C.POINTER(vp)])
    assert S["somhip_distortion_destroy"] == (None, [vp])
    assert S["somhip_distortion_clear"] == (C.c_int, [vp])
    assert S["somhip_distortion_accumulate"] == (C.c_int, [vp, vp, vp, C.c_int64, C.c_int64])
    assert S["somhip_distortion_evaluate"] == (C.c_int, [vp, vp, C.c_float, dp, tot])
    assert S["somhip_distortion_read"] == (C.c_int, [vp, _lib.c_u32_p, dp, dp])
    assert S["somhip_debug_distortion_evaluate"] == (C.c_int, [vp, C.c_float, _lib.c_u32_p, dp, dp, dp, tot])
    assert S["somhip_distortion_timing"] == (C.c_int, [vp, _lib.c_i64_p, dp])
    assert [f[0] for f in _lib.DistortionTotals._fields_] == ["energy", "scale", "samples"] and C.sizeof(_lib.DistortionTotals) == 24
    m = re.search(r"typedef struct somhip_distortion_totals \{(.*?)\} somhip_distortion_totals;", hdr)
    assert m and m.group(1).strip() == "double energy; double scale; uint64_t samples;"
    assert ("int somhip_distortion_accumulate(somhip_distortion *st, somhip_codebook *cb, somhip_dataset *ds, int64_t first, "
            "int64_t n);") in hdr
    assert "int somhip_distortion_evaluate(somhip_distortion *st, somhip_codebook *cb, float r, double *unit_out , somhip_distortion_totals *totals);" in hdr
    for name in ("Distortion", "map_distortion", "distortion_evaluate"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "distortion_timing")


def test_null_handles_are_refused_by_name(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    out, tot = C.c_void_p(), _lib.DistortionTotals()
    n, ms = (C.c_int64 * 3)(), (C.c_double * 3)()
    u32, f64 = (C.c_uint32 * 1)(), (C.c_double * 1)()
    calls = {
        "somhip_distortion_create": (None, C.byref(out)),
        "somhip_distortion_clear": (None,),
        "somhip_distortion_accumulate": (None, None, None, 0, 1),
        "somhip_distortion_evaluate": (None, None, 1.0, None, C.byref(tot)),
        "somhip_distortion_read": (None, u32, f64, f64),
        "somhip_debug_distortion_evaluate": (None, 1.0, u32, f64, f64, None, C.byref(tot)),
        "somhip_distortion_timing": (None, n, ms),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        msg = lib.somhip_last_error().decode()
        assert msg.startswith(name + ": null"), msg
    lib.somhip_distortion_destroy(None)                              # (nothing to do, nothing to report)
    assert out.value is None


def test_somqual_distortion_refusals_need_no_engine(tools, tmp_path):
    p = run("somqual", "-help")
    assert p.returncode == 0 and "-distortion R" in p.stdout
    cod = tmp_path / "m.cod"
    cod.write_text("2 hexa 2 2 bubble\n0 0\n1 0\n0 1\n1 1\n")
    dat = tmp_path / "d.dat"
    dat.write_text("2\n0.25 0.5\n0.75 0.5\n")
    for tail in (("-distortion",), ("-distortion", "-1"), ("-distortion", "-0.5"), ("-distortion", "nan"), ("-distortion", "two")):
        p = run("somqual", "-din", dat, "-cin", cod, *tail)
        assert p.returncode == 1 and p.stderr.startswith("somqual: -distortion needs a radius >= 0"), (tail, p.stderr)
        assert p.stdout == ""
    xcod = tmp_path / "x.cod"
    xcod.write_text("2 hexa 2 2 bubble\nx 0\n1 0\n0 1\n1 1\n")
    p = run("somqual", "-din", dat, "-cin", xcod, "-distortion", 1)
    assert p.returncode == 1 and "masked components" in p.stderr and p.stdout == ""


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
    """test_batchmap.py's generator, restated: a map laid out as a noisy sheet in the data space and data scattered around
    the sheet"""
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


def same_state(got, want):
    for g, w, dt in zip(got, want, (np.uint32, np.float64, np.float64)):
        assert g.dtype == dt and g.shape == w.shape
        assert np.array_equal(bits(g), bits(np.asarray(w, dtype=dt))), np.argwhere(bits(g) != bits(np.asarray(w, dtype=dt)))[:8]


def replay_state(win, x, q, units, first=0, n=None):
    hits, S = R.sums(win, x, units, first, n)
    return hits, S, R.sq_sums(win, q, units, first, n)


def check_accumulate(E, eng, oracle, codes, x, topol, xdim, ydim, windows):
    """every window (first, n) into a cleared state: hits, S and Q as the replay's chains leave them"""
    cb = E.Codebook(eng, codes, topol, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x)
    st = E.Distortion(cb)
    win, _ = R.winners(oracle, codes, x)
    q = R.sample_sq(x)
    out = []
    for first, n in windows:
        st.clear()
        st.accumulate(cb, ds, first, n)
        got = st.read()
        same_state(got, replay_state(win, x, q, codes.shape[0], first, n))
        assert int(got[0].sum()) == n
        out.append(got)
    assert np.array_equal(bits(cb.download()), bits(codes))          # the stage writes no row
    st.close(); cb.close(); ds.close()
    return win, out


# ---- accumulate, exact
@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol", [(1, 1, HEXA), (15, 1, RECT), (12, 8, HEXA), (1030, 1, RECT)])
def test_accumulate_units(E, eng, oracle, xdim, ydim, topol):
    """1, 15, 96 and 1030 units (the q sums take a wave per unit, four to a workgroup), over 700 samples and over one; on
    the one-unit map lists of 63, 64, 65 and 128 entries: the q sums take 64 at a time"""
    x, codes = mixture(300 + xdim * ydim, 700, 3, xdim, ydim)
    check_accumulate(E, eng, oracle, codes, x, topol, xdim, ydim, [(0, 700), (0, 1), (699, 1), (5, 63), (0, 64), (3, 65), (0, 128)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 129])
def test_accumulate_dims(E, eng, oracle, dim):
    """the butterfly's edges (a lane without a component, every lane with one, lane 0 with two, three steps) and the sums
    kernel's (63 fills one workgroup with the counts column, 64 puts it alone into a second, 129 needs a third)"""
    x, codes = mixture(400 + dim, 700, dim, 13, 5)
    check_accumulate(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 700)])


@pytest.mark.gpu
def test_accumulate_chunks_and_wrap(E, eng, oracle):
    """one fewer and one more sample than the search's chunk of 4096; a range that starts near the end of the data and wraps"""
    x, codes = mixture(17, 6000, 5, 13, 5)
    check_accumulate(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 4095), (0, 4097), (5990, 700)])


@pytest.mark.gpu
def test_accumulate_one_unit_takes_everything(E, eng, oracle):
    x, codes = mixture(18, 4500, 5, 13, 5)
    codes = codes + np.float32(1000.0)
    codes[37] = x.mean(axis=0)
    win, (got,) = check_accumulate(E, eng, oracle, codes, x, HEXA, 13, 5, [(0, 4500)])
    assert (win == 37).all() and got[0][37] == 4500 and (got[2][np.arange(65) != 37] == 0).all()


@pytest.mark.gpu
def test_accumulate_most_units_empty(E, eng, oracle):
    x, codes = mixture(19, 700, 4, 40, 30)
    codes = codes + np.float32(500.0)
    for u in (0, 611, 1199):
        codes[u] = x[u % 7]
    win, (got,) = check_accumulate(E, eng, oracle, codes, x, RECT, 40, 30, [(0, 700)])
    assert set(np.nonzero(got[0])[0]) <= {0, 611, 1199} and (got[1][got[0] == 0] == 0).all() and (got[2][got[0] == 0] == 0).all()


@pytest.fixture(scope="module")
def cut_case(E, eng, oracle):
    """9000 rows over a 9 x 8 map, dim 5: the one call's state, checked against the replay once, for the cuts to equal"""
    x, codes = mixture(21, 9000, 5, 9, 8)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
    ds = E.Dataset(eng, x)
    st = E.Distortion(cb)
    st.accumulate(cb, ds)
    whole = st.read()
    win, _ = R.winners(oracle, codes, x)
    same_state(whole, replay_state(win, x, R.sample_sq(x), 72))
    yield x, cb, ds, st, whole
    st.close(); cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(1,), (4095,), (4096,), (4097,), (700, 701, 5000, 5003, 8999)])
def test_any_cut_leaves_the_bits_of_one_call(cut_case, cuts):
    """the data cut at row 1, around the search's chunk edge, and into uneven pieces with single-row pieces among them"""
    x, cb, ds, st, whole = cut_case
    st.clear()
    edges = (0,) + tuple(cuts) + (9000,)
    for a, b in zip(edges[:-1], edges[1:]):
        st.accumulate(cb, ds, a, b - a)
    same_state(st.read(), whole)
    assert st.evaluate(cb, 1.5, units=False)[0]["samples"] == 9000


@pytest.mark.gpu
def test_pieces_from_two_data_sets_and_clear(E, eng, cut_case):
    """a piece from a second data set between two pieces of the first, and one that wraps inside its own: the state of one
    call over the rows in that order; clear and the same again: the same bits"""
    x, cb, ds, st, whole = cut_case
    second = E.Dataset(eng, np.roll(x[3000:5000], -1500, axis=0))        # rows 4500 .. 4999, 3000 .. 4499
    for _ in range(2):
        st.clear()
        assert int(st.read()[0].sum()) == 0 and st.evaluate(cb, 1.0)[0] == {"energy": 0.0, "scale": 0.0, "samples": 0}
        st.accumulate(cb, ds, 0, 3000)
        st.accumulate(cb, second, 500, 2000)                             # wraps: second's rows 500 .. 1999, 0 .. 499
        st.accumulate(cb, ds, 5000, 4000)
        same_state(st.read(), whole)
    second.close()


# ---- evaluate, within the derived bounds
def evaluate_inputs(seed, units, dim, corner=False):
    rs = np.random.RandomState(seed)
    codes = rs.standard_normal((units, dim)).astype(np.float32)
    if corner:
        hits = np.zeros(units, dtype=np.uint32)
        hits[0] = 7
    else:
        hits = rs.randint(0, 6, size=units).astype(np.uint32)
        hits[rs.uniform(size=units) < 0.3] = 0
    # sums with mixed signs, doubles that are no floats
    live = np.where(hits > 0, hits, 0).astype(np.float64)
    S = rs.standard_normal((units, dim)) * live[:, None] * rs.choice([-3.0, 0.25, 1.0, 40.0], size=(units, 1))
    Q = rs.uniform(0.5, 30.0, size=units) * live * dim
    return codes, hits, S, Q


def check_evaluate(E, eng, codes, hits, S, Q, topol, neigh, xdim, ydim, r):
    units, dim = codes.shape
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    tot, e = E.distortion_evaluate(cb, r, hits, S, Q)
    tot2, e2 = E.distortion_evaluate(cb, r, hits, S, Q)
    assert np.array_equal(bits(e), bits(e2)) and tot == tot2              # the same call twice: the same bits
    assert np.array_equal(bits(cb.download()), bits(codes))             # it writes no row
    cb.close()
    h = R.weights(topol, neigh, xdim, ydim, r)
    want_e, want_E, Rj, D, scale = R.evaluate(h, hits, S, Q, codes)
    err = np.abs(e.astype(ld) - want_e)
    allow = ld(R.c_unit(units, dim)) * R.EPS * Rj
    assert (err <= allow).all(), (np.argmax(err - allow), float(err.max()), float(allow.max()))
    assert (e[D == 0] == 0).all() and not np.signbit(e[D == 0]).any()
    assert abs(ld(tot["energy"]) - want_E) <= ld(R.c_total(units, dim)) * R.EPS * Rj.sum(), (tot["energy"], float(want_E))
    assert abs(ld(tot["scale"]) - scale) <= ld(R.c_total(units, dim)) * R.EPS * scale
    assert tot["samples"] == int(hits.sum())
    return tot, e, D


EVAL_CASES = [  # (xdim, ydim, topol, neigh, dim, radius)
    (1, 1, HEXA, BUBBLE, 1, 0.0), (1, 1, RECT, GAUSSIAN, 15, 1.0),
    (5, 3, HEXA, BUBBLE, 16, 0.0), (5, 3, RECT, BUBBLE, 17, 1.0), (5, 3, HEXA, GAUSSIAN, 63, 2.5), (5, 3, RECT, GAUSSIAN, 64, 100.0),
    (9, 8, HEXA, BUBBLE, 65, 2.5), (9, 8, RECT, BUBBLE, 129, 100.0), (9, 8, HEXA, GAUSSIAN, 17, 1.0), (9, 8, RECT, GAUSSIAN, 1, 2.5),
    (32, 8, HEXA, BUBBLE, 15, 1.0), (32, 8, RECT, GAUSSIAN, 16, 2.5), (32, 8, HEXA, BUBBLE, 5, 0.0),
    (8, 24, RECT, BUBBLE, 63, 2.5), (8, 24, HEXA, GAUSSIAN, 64, 100.0), (8, 24, HEXA, BUBBLE, 65, 100.0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,dim,r", EVAL_CASES)
def test_evaluate_within_the_derived_bound(E, eng, xdim, ydim, topol, neigh, dim, r):
    """bubble and gaussian on hexa and rect; radius 0, 1, 2.5 and beyond the map; maps 1 x 1, 5 x 3, 9 x 8 and, stored in
    patches, 32 x 8 and 8 x 24; dims at the 16- and 64-column edges; sums of mixed signs"""
    codes, hits, S, Q = evaluate_inputs(1000 * xdim + 10 * dim + ydim, xdim * ydim, dim)
    _, e, D = check_evaluate(E, eng, codes, hits, S, Q, topol, neigh, xdim, ydim, r)
    if neigh == BUBBLE and r == 0.0 and xdim * ydim >= 15:
        assert (D == 0).any() and (D > 0).any()                         # some units have no sample within the radius


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh", [(9, 8, HEXA, BUBBLE), (32, 8, RECT, GAUSSIAN), (8, 24, HEXA, BUBBLE)])
def test_evaluate_every_hit_in_one_corner(E, eng, xdim, ydim, topol, neigh):
    codes, hits, S, Q = evaluate_inputs(77 + xdim, xdim * ydim, 17, corner=True)
    _, e, D = check_evaluate(E, eng, codes, hits, S, Q, topol, neigh, xdim, ydim, 1.0)
    if neigh == BUBBLE:
        assert 2 <= int((D > 0).sum()) <= 5 and (e[D == 0] == 0).all()


@pytest.mark.gpu
def test_evaluate_gaussian_at_radius_zero_is_not_a_number(E, eng):
    """K8's weight exp(-dd^2 / (2 r^2)) is 0 / 0 on the diagonal at r = 0: the definition's own value, passed on, not hidden"""
    codes, hits, S, Q = evaluate_inputs(5, 15, 4)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 5, 3)
    tot, e = E.distortion_evaluate(cb, 0.0, hits, S, Q)
    assert np.isnan(tot["energy"]) and np.isnan(e[hits > 0]).all()
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,r", [(9, 8, HEXA, GAUSSIAN, 2.5), (32, 8, RECT, BUBBLE, 1.0)])
def test_evaluate_data_far_from_the_origin(E, eng, xdim, ydim, topol, neigh, r):
    """x around 1000: every term of e_j is near 10^6 per component, their sum near 1: E << scale, the bound is what holds,
    and scale says so"""
    x, codes = mixture(31, 700, 17, xdim, ydim)
    x, codes = x + np.float32(1000.0), codes + np.float32(1000.0)
    win = ((x.astype(np.float64)[:, None, :] - codes.astype(np.float64)[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
    hits, S = R.sums(win, x, xdim * ydim)
    Q = R.sq_sums(win, R.sample_sq(x), xdim * ydim)
    tot, e, _ = check_evaluate(E, eng, codes, hits, S, Q, topol, neigh, xdim, ydim, r)
    want = R.direct(R.weights(topol, neigh, xdim, ydim, r), win, x, codes)[1]
    assert 0 < want < ld(1e-5) * ld(tot["scale"])
    assert abs(ld(tot["energy"]) - want) <= ld(R.c_total(xdim * ydim, 17) + R.chain_extra(int(hits.max()), 17)) * R.EPS * ld(tot["scale"])


# ---- end to end
@pytest.fixture(scope="module")
def e2e(E, eng, oracle):
    """700 samples on 5 x 3 (hexa, bubble) and 9 x 8 (rect, gaussian), dim 6: accumulated once"""
    out = {}
    for key, (xdim, ydim, topol, neigh) in {"5x3": (5, 3, HEXA, BUBBLE), "9x8": (9, 8, RECT, GAUSSIAN)}.items():
        x, codes = mixture(41 + xdim, 700, 6, xdim, ydim)
        cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
        ds = E.Dataset(eng, x)
        st = E.Distortion(cb)
        st.accumulate(cb, ds)
        win, _ = R.winners(oracle, codes, x)
        out[key] = dict(x=x, codes=codes, cb=cb, ds=ds, st=st, win=win, shape=(xdim, ydim, topol, neigh))
    yield out
    for c in out.values():
        c["st"].close(); c["cb"].close(); c["ds"].close()


def e2e_bound(c, R_sum):
    units, dim = c["codes"].shape
    max_hits = int(np.bincount(c["win"], minlength=units).max())
    return ld(R.c_total(units, dim) + R.chain_extra(max_hits, dim)) * R.EPS * R_sum


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["5x3", "9x8"])
@pytest.mark.parametrize("r", [1.0, 2.5])
def test_accumulate_and_evaluate_against_the_direct_sum(e2e, key, r):
    """E and e_j against sum_s sum_j h |x_s - m_j|^2 in np.longdouble: the evaluate bound plus the chains' own"""
    c = e2e[key]
    xdim, ydim, topol, neigh = c["shape"]
    tot, e = c["st"].evaluate(c["cb"], r)
    want_e, want_E, Rj = R.direct(R.weights(topol, neigh, xdim, ydim, r), c["win"], c["x"], c["codes"])
    units, dim = c["codes"].shape
    extra = R.chain_extra(int(np.bincount(c["win"], minlength=units).max()), dim)
    assert (np.abs(e.astype(ld) - want_e) <= ld(R.c_unit(units, dim) + extra) * R.EPS * Rj).all()
    assert abs(ld(tot["energy"]) - want_E) <= e2e_bound(c, Rj.sum())
    assert tot["samples"] == 700 and want_E > 0 and Rj.sum() <= ld(tot["scale"]) * (1 + ld(1e-12))


@pytest.mark.gpu
def test_radius_zero_bubble_is_the_sum_of_squared_quantization_errors(E, e2e):
    c = e2e["5x3"]
    tot, e = c["st"].evaluate(c["cb"], 0.0)
    idx, d1, _ = E.find_winners(c["cb"], c["ds"])
    assert np.array_equal(idx[:, 0], c["win"])
    want = d1[:, 0].astype(ld).sum()
    Rj = R.direct(R.weights(HEXA, BUBBLE, 5, 3, 0.0), c["win"], c["x"], c["codes"])[2]
    assert abs(ld(tot["energy"]) - want) <= e2e_bound(c, Rj.sum()) + ld(6 + 1) * ld(2.0) ** -24 * want
    per = np.bincount(c["win"], weights=d1[:, 0].astype(np.float64), minlength=15)
    assert np.allclose(e, per, rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["5x3", "9x8"])
def test_a_batch_map_epoch_minimises_the_energy_for_fixed_winners(E, eng, e2e, key):
    """with hits and S held fixed, batchmap_combine's rows are the minimiser of E(r): the energy does not rise from the
    rows the winners were found with, and falls strictly from random rows"""
    c = e2e[key]
    xdim, ydim, topol, neigh = c["shape"]
    hits, S, _ = c["st"].read()
    units, dim = c["codes"].shape
    rs = np.random.RandomState(3)
    for rows, strictly in ((c["codes"], False), (rs.standard_normal((units, dim)).astype(np.float32) * 3, True)):
        cb = E.Codebook(eng, rows, topol, neigh, xdim, ydim)
        before = c["st"].evaluate(cb, 1.5, units=False)[0]
        E.batchmap_combine(cb, 1.5, hits, S)
        after = c["st"].evaluate(cb, 1.5, units=False)[0]
        bound = float(ld(R.c_total(units, dim)) * R.EPS * ld(before["scale"] + after["scale"]))
        assert after["energy"] <= before["energy"] + bound
        if strictly:
            assert after["energy"] < before["energy"] - bound
        cb.close()


@pytest.mark.gpu
def test_evaluate_leaves_the_codebook_and_an_open_batch_map_state_alone(E, eng):
    x, codes = mixture(51, 1400, 6, 9, 8)
    ds = E.Dataset(eng, x)

    def epoch(disturb):
        cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
        E.batchmap_begin(cb)
        E.batchmap_accumulate(cb, ds, 0, 700)
        if disturb:
            addr, nbytes = E.batchmap_state(cb)
            blob = eng.copy_to_host(addr, nbytes)
            st = E.Distortion(cb)
            st.accumulate(cb, ds, 100, 900)
            st.evaluate(cb, 2.0)
            tot = E.map_distortion(cb, ds, 1.0)[0]
            assert tot["samples"] == 1400
            st.close()
            assert E.batchmap_state(cb) == (addr, nbytes) and bytes(eng.copy_to_host(addr, nbytes)) == bytes(blob)
            assert np.array_equal(bits(cb.download()), bits(codes))
        E.batchmap_accumulate(cb, ds, 700, 700)
        q = E.batchmap_finish(cb, 2.0)
        rows = cb.download()
        E.batchmap_end(cb)
        cb.close()
        return q, rows

    qa, ra = epoch(False)
    qb, rb = epoch(True)
    assert qa == qb and np.array_equal(bits(ra), bits(rb))
    ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng):
    x, codes = mixture(61, 700, 6, 13, 5)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    lvq = E.Codebook(eng, codes, E.TOPOL_LVQ)
    shard = E.Codebook(eng, codes[:26], HEXA, BUBBLE, 13, 5, row_offset=13, n_global=65)
    other_dim = E.Dataset(eng, x[:, :5])
    other_map = E.Codebook(eng, codes[:60], HEXA, BUBBLE, 12, 5)
    other_cols = E.Codebook(eng, codes[:, :5], HEXA, BUBBLE, 13, 5)
    eng2 = E.Engine(0)
    cb2, ds2 = E.Codebook(eng2, codes, HEXA, BUBBLE, 13, 5), E.Dataset(eng2, x)
    st = E.Distortion(cb)
    st.accumulate(cb, ds, 0, 300)
    state = st.read()

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)
        same_state(st.read(), state)
        assert np.array_equal(bits(cb.download()), bits(codes))

    acc, ev, mk = "somhip_distortion_accumulate", "somhip_distortion_evaluate", "somhip_distortion_create"
    refused(lambda: E.Distortion(lvq), mk, "without a lattice")
    refused(lambda: E.Distortion(shard), mk, "sharded")
    refused(lambda: st.accumulate(cb, masked), acc, "masked components")
    refused(lambda: st.accumulate(cb, other_dim), acc, "dimension")
    refused(lambda: st.accumulate(other_map, ds), acc, "the state is of a 65 x 6 codebook")
    refused(lambda: st.accumulate(other_cols, other_dim), acc, "the state is of a 65 x 6 codebook")
    refused(lambda: st.accumulate(cb2, ds2), acc, "different engines")
    refused(lambda: st.accumulate(cb, ds2), acc, "different engines")
    refused(lambda: st.accumulate(cb, ds, -1, 10), acc, "first row -1 < 0")
    refused(lambda: st.accumulate(cb, ds, 0, 0), acc, "<= 0")
    refused(lambda: st.accumulate(cb, ds, 0, -5), acc, "<= 0")
    refused(lambda: st.accumulate(cb, ds, 0, 1 << 32), acc, "32-bit hit counts")
    refused(lambda: st.accumulate(cb, ds, 0, (1 << 32) - 300), acc, "300 + 4294966996 samples do not fit")
    refused(lambda: st.evaluate(cb, -0.5), ev, "radius")
    refused(lambda: st.evaluate(cb, float("nan")), ev, "radius")
    refused(lambda: st.evaluate(other_map, 1.0), ev, "the state is of a 65 x 6 codebook")
    refused(lambda: st.evaluate(cb2, 1.0), ev, "different engines")
    refused(lambda: E.distortion_evaluate(cb, -1.0, state[0], state[1], state[2]), "somhip_debug_distortion_evaluate", "radius")
    refused(lambda: E.distortion_evaluate(lvq, 1.0, state[0], state[1], state[2]), "somhip_debug_distortion_evaluate", "without a lattice")
    st.accumulate(cb, ds, 300, 400)                                     # and the state goes on where it stood
    whole = E.Distortion(cb)
    whole.accumulate(cb, ds)
    same_state(st.read(), whole.read())
    eng2.close()
    for o in (st, whole, cb, ds, masked, lvq, shard, other_dim, other_map, other_cols):
        o.close()


@pytest.mark.gpu
def test_timing_counts_the_stages_under_ids_of_their_own(E, eng):
    x, codes = mixture(71, 5000, 70, 9, 8)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
    ds = E.Dataset(eng, x)
    eng.timing(True)
    eng.timing_reset()
    tot, _ = E.map_distortion(cb, ds, 2.0)
    t, bm = eng.distortion_timing(), eng.batchmap_timing()
    eng.timing(False)
    assert t["group"][0] == 2 + 1 + 1                                   # two chunks' winners passes, the scan, the sort
    assert t["sums"][0] == 3 and t["evaluate"][0] == 4                  # sums, q, q sums; table, kernel, two fold passes
    assert all(v == (0, 0.0) for v in bm.values())                      # nothing under the batch map's ids
    assert tot["samples"] == 5000
    cb.close(); ds.close()


# ---- the tool
def distortion_line(r, neigh, tot):
    ns = float(tot["samples"])
    return "Distortion at radius %g (%s neighbourhood) is %.9g per sample (%d samples), resolved to %.3g" % (
        r, neigh, tot["energy"] / ns, tot["samples"], np.ldexp(tot["scale"], -52) / ns)


@pytest.mark.gpu
def test_somqual_distortion_on_the_example_data(E, eng, tools, tmp_path, exdata):
    cod = read_cod("som_hexa_bubble.cod")
    cb = E.Codebook(eng, cod.points, cod.topol, cod.neigh, cod.xdim, cod.ydim)
    ds = E.Dataset(eng, exdata["ex"].points)
    tot, e = E.map_distortion(cb, ds, 2.0)
    cb.close(); ds.close()
    plain = run("somqual", "-din", DATA, "-cin", MAP)
    assert plain.returncode == 0 and plain.stdout.count("\n") == 3
    u0, u1, pairs = tmp_path / "u0.txt", tmp_path / "u1.txt", tmp_path / "pairs.txt"
    assert run("somqual", "-din", DATA, "-cin", MAP, "-uout", u0).stdout == plain.stdout     # without -distortion: as before
    p = run("somqual", "-din", DATA, "-cin", MAP, "-distortion", 2, "-uout", u1)
    assert p.returncode == 0, p.stderr
    assert p.stdout == plain.stdout + distortion_line(2.0, "bubble", tot) + "\n"
    old, new = u0.read_text().splitlines(), u1.read_text().splitlines()
    assert len(old) == len(new) == cb.n
    assert new == ["%s %.9g" % (line, e[u]) for u, line in enumerate(old)]
    # behind -conn's line, and the data taken buffer by buffer: the same bytes
    pc = run("somqual", "-din", DATA, "-cin", MAP, "-conn", pairs, "-distortion", 2)
    assert pc.stdout.split("\n")[:3] == plain.stdout.split("\n")[:3] and pc.stdout.split("\n")[3].startswith("Connected pairs")
    assert pc.stdout.split("\n")[4:] == [distortion_line(2.0, "bubble", tot), ""]
    for n in (7, 4096):
        ub = tmp_path / ("u_%d.txt" % n)
        pb = run("somqual", "-din", DATA, "-cin", MAP, "-distortion", 2, "-uout", ub, "-buffer", n)
        assert pb.stdout == p.stdout and ub.read_bytes() == u1.read_bytes()


@pytest.mark.gpu
def test_somqual_distortion_reads_raw_fp32_and_generated_sources(tools, tmp_path):
    raw = tmp_path / "ex.f32"
    assert run("datconv", "-din", DATA, "-dout", raw).returncode == 0
    text = run("somqual", "-din", DATA, "-cin", MAP, "-distortion", 1.5).stdout.split("\n")
    got = run("somqual", "-din", raw, "-cin", MAP, "-distortion", 1.5).stdout.split("\n")
    assert len(text) == 5 and text[3].startswith("Distortion at radius 1.5 (bubble neighbourhood) is ") and got[1:] == text[1:]
    gen = "gen:k=4,dim=5,n=3000,seed=9"
    whole = run("somqual", "-din", gen, "-cin", MAP, "-distortion", 1.5).stdout.split("\n")
    assert re.fullmatch(r"Distortion at radius 1\.5 \(bubble neighbourhood\) is \S+ per sample \(3000 samples\), resolved to \S+", whole[3])
    assert whole == run("somqual", "-din", gen, "-cin", MAP, "-distortion", 1.5, "-buffer", 1000).stdout.split("\n")
