"""The batch map over data with missing values (K8m: somhip_som_batchmap_missing, its two stages and its five calls over
data in pieces, `bsom -missing`; include/somhip_batchmap_missing.h) against the CPU replay in batchmap_missing_replay.py.

The sums stage is compared exactly: S by bit pattern and C by value with the replay's data-order fp64 chains, which skip a
masked component.  Masked positions of the data hold 1e30 and NaN by turns: a case passes only if nothing of them leaks.
The combine is compared against a bound that is derived, not measured: with q = N / D formed in np.longdouble per
component, |m - q| <= ulp32(q) / 2 + (4 * units + 16) * 2^-52 * A / D, A = sum_j h |S_j| -- the rounding to float, at most
two fp64 roundings per term (the FMA and the weight) in each of N and D, D's relative error acting on |q| <= A / D, and 16
for the division and slack.  Every element is compared; a component with D == 0 keeps its bits.  On data without masks
the entry point leaves the bits of somhip_som_batchmap.

The ctypes mirror of the new header is _lib.BATCHMAP_MISSING_SIGNATURES, a table of its own as every header that
include/somhip.h includes has: tests/test_build.py holds _lib.SIGNATURES to the declarations of somhip.h itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batchmap_missing_replay as R
from conftest import ROOT

HEXA, RECT = 3, 4
BUBBLE, GAUSSIAN = 1, 2
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
NAMES = ("somhip_som_batchmap_missing", "somhip_debug_batchmap_missing_sums", "somhip_debug_batchmap_missing_combine",
         "somhip_batchmap_missing_begin", "somhip_batchmap_missing_accumulate", "somhip_batchmap_missing_finish",
         "somhip_batchmap_missing_end", "somhip_batchmap_missing_state")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not os.path.exists(os.path.join(BIN, "bsom")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args, env=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, env=dict(os.environ, **env) if env else None)


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_signatures_and_wrappers(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.BATCHMAP_MISSING_SIGNATURES
    assert set(S) == set(NAMES)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == S[name][1] and getattr(lib, name).restype == S[name][0], name
    vp, i64, dp, fp = C.c_void_p, C.c_int64, _lib.c_double_p, _lib.c_float_p
    assert S["somhip_som_batchmap_missing"] == (C.c_int, [vp, vp, C.POINTER(_lib.BatchmapParams), fp])
    assert S["somhip_debug_batchmap_missing_sums"] == (C.c_int, [vp, vp, i64, i64, dp, dp])
    assert S["somhip_debug_batchmap_missing_combine"] == (C.c_int, [vp, C.c_float, dp, dp])
    assert S["somhip_batchmap_missing_begin"] == (C.c_int, [vp])
    assert S["somhip_batchmap_missing_accumulate"] == (C.c_int, [vp, vp, i64, i64, C.c_int])
    assert S["somhip_batchmap_missing_finish"] == (C.c_int, [vp, C.c_float, i64, i64, fp])
    assert S["somhip_batchmap_missing_end"] == (C.c_int, [vp])
    assert S["somhip_batchmap_missing_state"] == (C.c_int, [vp, C.POINTER(vp), _lib.c_i64_p])
    others = set(_lib.SIGNATURES) | set(_lib.RSLVQ_SIGNATURES) | set(_lib.GLVQ_PIECES_SIGNATURES) | set(_lib.NG_DENSE_SIGNATURES)
    assert not (set(S) & others)
    for name in ("som_batchmap_missing", "batchmap_missing_sums", "batchmap_missing_combine", "batchmap_missing_begin",
                 "batchmap_missing_accumulate", "batchmap_missing_finish", "batchmap_missing_end", "batchmap_missing_state"):
        assert callable(getattr(engine, name, None)), name


def test_header_declares_the_entry_points():
    top = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r'^#include "somhip_batchmap_missing.h"$', top, flags=re.M)
    hdr = open(os.path.join(ROOT, "include", "somhip_batchmap_missing.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert set(re.findall(r"\b(somhip_[a-z0-9_]+)\s*\(", hdr)) == set(NAMES)
    for decl in ("int somhip_som_batchmap_missing(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out );",
                 "int somhip_debug_batchmap_missing_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, double *sums, double *counts);",
                 "int somhip_debug_batchmap_missing_combine(somhip_codebook *cb, float r, const double *sums, const double *counts);",
                 "int somhip_batchmap_missing_begin(somhip_codebook *cb);",
                 "int somhip_batchmap_missing_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror);",
                 "int somhip_batchmap_missing_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count, float *qerror_out);",
                 "int somhip_batchmap_missing_end(somhip_codebook *cb);",
                 "int somhip_batchmap_missing_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);"):
        assert decl in hdr, decl


def test_null_arguments_are_refused_by_name(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    p = _lib.BatchmapParams(3, 2.0, 0, 3, 0, 10)
    d = (C.c_double * 4)()
    dp = C.cast(d, _lib.c_double_p)
    addr, nbytes = C.c_void_p(), C.c_int64(0)
    calls = {"somhip_som_batchmap_missing": lambda: lib.somhip_som_batchmap_missing(None, None, C.byref(p), None),
             "somhip_debug_batchmap_missing_sums": lambda: lib.somhip_debug_batchmap_missing_sums(None, None, 0, 10, dp, dp),
             "somhip_debug_batchmap_missing_combine": lambda: lib.somhip_debug_batchmap_missing_combine(None, 2.0, dp, dp),
             "somhip_batchmap_missing_begin": lambda: lib.somhip_batchmap_missing_begin(None),
             "somhip_batchmap_missing_accumulate": lambda: lib.somhip_batchmap_missing_accumulate(None, None, 0, 10, 1),
             "somhip_batchmap_missing_finish": lambda: lib.somhip_batchmap_missing_finish(None, 2.0, 0, 1, None),
             "somhip_batchmap_missing_end": lambda: lib.somhip_batchmap_missing_end(None),
             "somhip_batchmap_missing_state": lambda: lib.somhip_batchmap_missing_state(None, C.byref(addr), C.byref(nbytes))}
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        assert call() != 0, name
        assert lib.somhip_last_error().decode() in (name + ": null argument", name + ": null handle"), name


def test_bsom_help_and_refusals(tools, tmp_path):
    """-help names the option; the refusals that need no engine come before one is asked for, so they hold without a GPU"""
    p = run("bsom", "-help")
    assert p.returncode == 0 and "-missing" in p.stdout
    cod = tmp_path / "m.cod"
    cod.write_text("2 hexa 2 2 bubble\n0 0\n1 0\n0 1\n1 1\n")
    xdat = tmp_path / "x.dat"
    xdat.write_text("2\nx 0.5\n0.75 0.5\n")
    out = tmp_path / "o.cod"
    nowhere = {"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}                   # an engine, were one asked for, would fail otherwise
    p = run("bsom", "-cin", cod, "-din", xdat, "-cout", out, "-epochs", 2, "-radius", 2, "-missing", "-gpus", 2, env=nowhere)
    assert p.returncode == 1 and p.stderr.startswith("bsom: ") and "-missing" in p.stderr and "-gpus" in p.stderr, p.stderr
    assert "\n" not in p.stderr.strip()                                                # that line alone: no engine spoke
    for args, word in ((("-epochs", 0, "-radius", 2), "-epochs"), (("-epochs", 2, "-radius", 0.5), "-radius")):
        p = run("bsom", "-cin", cod, "-din", xdat, "-cout", out, "-missing", *args)
        assert p.returncode == 1 and p.stderr.startswith("bsom: " + word), (args, p.stderr)
    xcod = tmp_path / "x.cod"
    xcod.write_text("2 hexa 2 2 bubble\nx 0\n1 0\n0 1\n1 1\n")
    p = run("bsom", "-cin", xcod, "-din", xdat, "-cout", out, "-epochs", 2, "-radius", 2, "-missing")
    assert p.returncode == 1 and "masked components" in p.stderr
    p = run("bsom", "-cin", cod, "-din", xdat, "-cout", out, "-epochs", 2, "-radius", 2)      # as before, and the hint
    assert p.returncode == 1 and "masked components" in p.stderr and "not supported" in p.stderr and "-missing" in p.stderr
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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mixture(seed, n, d, xdim, ydim, noise=0.4):
    """test_batchmap.py's generator, restated: a map laid out as a noisy sheet in the data space and data scattered
    around the sheet"""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((2, d)).astype(np.float32)
    u = np.arange(xdim * ydim)
    pos = np.stack([u % xdim, u // xdim], axis=1).astype(np.float32)
    codes = (pos @ v + noise * rs.standard_normal((xdim * ydim, d))).astype(np.float32)
    at = (rs.uniform(size=(n, 2)) * [xdim, ydim]).astype(np.float32)
    x = (at @ v + 0.5 * rs.standard_normal((n, d))).astype(np.float32)
    return x, codes


def poison(x, mask):
    """x with 1e30 and NaN by turns where mask is set: what is stored at a masked component must never be seen"""
    x = x.copy()
    at = np.argwhere(mask != 0)
    x[at[0::2, 0], at[0::2, 1]] = np.float32(1e30)
    x[at[1::2, 0], at[1::2, 1]] = np.float32("nan")
    return x


def masked(seed, x, share=0.3):
    """(x poisoned, mask): `share` of the components masked at random"""
    mask = (np.random.RandomState(seed).uniform(size=x.shape) < share).astype(np.uint8)
    return poison(x, mask), mask


def check_sums(E, eng, oracle, codes, x, mask, topol, xdim, ydim, windows):
    cb = E.Codebook(eng, codes, topol, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x, mask=mask)
    win, _ = R.winners(oracle, codes, x, mask)
    out = []
    for first, n in windows:
        gs, gc = E.batchmap_missing_sums(cb, ds, first, n)
        ws, wc = R.sums(win, x, mask, codes.shape[0], first, n)
        assert gs.dtype == np.float64 and gc.dtype == np.float64 and gs.shape == gc.shape == codes.shape
        assert np.array_equal(gc, wc), np.argwhere(gc != wc)[:8]
        assert np.array_equal(bits(gs), bits(ws)), np.argwhere(bits(gs) != bits(ws))[:8]
        out.append((gs, gc))
    assert same(cb.download(), codes)                                  # the stage writes no row
    cb.close(); ds.close()
    return win, out


# ---- the sums, exact
@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol", [(1, 1, HEXA), (2, 1, RECT), (63, 1, HEXA), (1, 64, RECT), (13, 5, HEXA), (257, 1, RECT)])
def test_sums_units(E, eng, oracle, xdim, ydim, topol):
    """1, 2, 63, 64, 65 and 257 units, over 700 samples and over one"""
    x, codes = mixture(100 + xdim * ydim, 700, 3, xdim, ydim)
    x, mask = masked(1, x)
    check_sums(E, eng, oracle, codes, x, mask, topol, xdim, ydim, [(0, 700), (0, 1), (699, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 63, 64, 65, 129])
def test_sums_dims(E, eng, oracle, dim):
    """a sums workgroup has 64 columns: one short of it, one workgroup full, one column in a second, a third"""
    x, codes = mixture(200 + dim, 700, dim, 13, 5)
    x, mask = masked(2, x)
    check_sums(E, eng, oracle, codes, x, mask, HEXA, 13, 5, [(0, 700)])


@pytest.mark.gpu
def test_sums_chunks_and_wrap(E, eng, oracle):
    """the search's chunk of 4096 samples on a 5 x 3 map: one fewer, one more; runs that wrap once and twice"""
    x, codes = mixture(7, 6000, 5, 5, 3)
    x, mask = masked(3, x)
    check_sums(E, eng, oracle, codes, x, mask, HEXA, 5, 3, [(0, 4095), (0, 4096), (0, 4097), (5990, 700), (5990, 4097), (3, 12003)])


@pytest.mark.gpu
def test_sums_without_a_mask_and_with_a_mask_of_zeros(E, eng, oracle):
    """no mask array, and a mask of zeros: every count is the unit's hits, the sums are the plain stage's bits"""
    x, codes = mixture(12, 700, 65, 13, 5)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    plain = E.Dataset(eng, x)
    hits, S = E.batchmap_sums(cb, plain)
    for mask in (None, np.zeros(x.shape, dtype=np.uint8)):
        _, ((gs, gc),) = check_sums(E, eng, oracle, codes, x, mask, HEXA, 13, 5, [(0, 700)])
        assert same(gs, S) and np.array_equal(gc, np.repeat(hits.astype(np.float64)[:, None], 65, axis=1))
    cb.close(); plain.close()


@pytest.mark.gpu
def test_sums_mask_patterns(E, eng, oracle):
    """one column masked in every sample; a sample with every component masked; a sample with one known component"""
    x, codes = mixture(13, 700, 5, 13, 5)
    _, mask = masked(4, x)
    mask[:, 2] = 1                                                     # nobody knows component 2
    mask[17, :] = 1                                                    # sample 17 knows nothing
    mask[18, :] = 1
    mask[18, 4] = 0                                                    # sample 18 knows component 4 only
    xp = poison(x, mask)
    win, ((S, Cn),) = check_sums(E, eng, oracle, codes, xp, mask, HEXA, 13, 5, [(0, 700)])
    assert win[17] == R.NONE and win[18] != R.NONE
    assert not Cn[:, 2].any() and not bits(S[:, 2]).any()              # +0.0 throughout
    assert np.array_equal(Cn.sum(axis=0), (mask == 0).sum(axis=0).astype(np.float64))   # the totals: sample 17 feeds nothing
    assert np.isfinite(S).all() and np.abs(S).max() < 1e6
    # the all-masked sample alone: nothing anywhere; the one-component sample alone: one count
    check = [(17, 1), (18, 1)]
    _, ((s17, c17), (s18, c18)) = check_sums(E, eng, oracle, codes, xp, mask, HEXA, 13, 5, check)
    assert not c17.any() and not bits(s17).any()
    assert c18.sum() == 1 and c18[win[18], 4] == 1 and s18[win[18], 4] == np.float64(x[18, 4])


@pytest.mark.gpu
def test_sums_one_unit_takes_everything_and_twice(E, eng, oracle):
    """the longest chain: every sample of a run of more than a chunk on one unit; the same call twice leaves the same bits"""
    x, codes = mixture(8, 4500, 5, 13, 5)
    codes = codes + np.float32(1000.0)
    codes[37] = x.mean(axis=0)
    x, mask = masked(5, x)
    win, (a, b) = check_sums(E, eng, oracle, codes, x, mask, HEXA, 13, 5, [(0, 4500), (0, 4500)])
    assert (win[win != R.NONE] == 37).all() and a[1][37].max() > 3000
    assert same(a[0], b[0]) and same(a[1], b[1])


# ---- the combine, within the derived bound
def combine_inputs(seed, units, dim):
    """sums of mixed signs (doubles that are no floats) and counts per component, about 30 % of them zero"""
    rs = np.random.RandomState(seed)
    codes = rs.standard_normal((units, dim)).astype(np.float32)
    Cn = rs.randint(0, 6, size=(units, dim)).astype(np.float64)
    Cn[rs.uniform(size=(units, dim)) < 0.3] = 0
    S = rs.standard_normal((units, dim)) * Cn * rs.choice([-3.0, 0.25, 1.0, 40.0], size=(units, 1))
    return codes, S, Cn


def check_combine(E, eng, codes, S, Cn, topol, neigh, xdim, ydim, r):
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_missing_combine(cb, r, S, Cn)
    got = cb.download()
    cb.close()
    q, D, bound = R.combine(R.weights(topol, neigh, xdim, ydim, r), S, Cn)
    live = D > 0
    what = (topol, neigh, xdim, ydim, codes.shape[1], float(r))
    assert np.array_equal(bits(got)[~live], bits(codes)[~live]), what      # per component
    err = np.abs(got.astype(np.longdouble) - q)
    bad = live & (err > bound)
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), np.argwhere(bad)[:4])
    return live


MAPS = [(5, 3), (9, 8), (13, 5), (32, 8), (8, 24)]       # one partial row group, two groups, ..., and two maps stored in patches


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim", MAPS)
@pytest.mark.parametrize("dim", [5, 33])
def test_combine_maps(E, eng, xdim, ydim, dim):
    """bubble and gaussian on hexa and rect lattices at radius 1, 2.5 and one larger than the map"""
    codes, S, Cn = combine_inputs(1000 * xdim + ydim + dim, xdim * ydim, dim)
    for topol in (HEXA, RECT):
        for neigh in (BUBBLE, GAUSSIAN):
            for r in (1.0, 2.5, float(xdim + ydim + 3)):
                check_combine(E, eng, codes, S, Cn, topol, neigh, xdim, ydim, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129])
def test_combine_dims(E, eng, dim):
    """a workgroup has 32 value columns in two 16-column tiles: either side of a tile's and of a workgroup's edge"""
    codes, S, Cn = combine_inputs(77 + dim, 9 * 8, dim)
    for topol, neigh, r in ((HEXA, BUBBLE, 2.5), (RECT, GAUSSIAN, 2.5), (HEXA, GAUSSIAN, 1.0), (RECT, BUBBLE, 50.0)):
        check_combine(E, eng, codes, S, Cn, topol, neigh, 9, 8, r)


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim", [(13, 5), (32, 8), (8, 24)])
def test_combine_components_known_in_one_corner_or_nowhere(E, eng, xdim, ydim):
    """bubble, radius 1: component 3 is known only to samples of unit 0, so D > 0 at the corner's neighbours only; component
    5 is known to no sample and keeps its bits on every unit; the other components move everywhere they have samples"""
    codes, S, Cn = combine_inputs(5, xdim * ydim, 34)
    Cn[:, 3] = 0; S[:, 3] = 0
    Cn[0, 3] = 7; S[0, 3] = -12.625
    Cn[:, 5] = 0; S[:, 5] = 0
    for topol in (HEXA, RECT):
        live = check_combine(E, eng, codes, S, Cn, topol, BUBBLE, xdim, ydim, 1.0)
        assert set(np.nonzero(live[:, 3])[0]) == {0, 1, xdim}
        assert not live[:, 5].any() and live[:, 4].any() and live[:, 33].any()
        live = check_combine(E, eng, codes, S, Cn, topol, GAUSSIAN, xdim, ydim, 2.5)
        assert not live[:, 5].any()


# ---- equal to the plain batch map on data without masks
@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,dim", [(9, 8, HEXA, 5), (32, 8, RECT, 65)])
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN])
def test_unmasked_data_leave_the_plain_bits(E, eng, xdim, ydim, topol, dim, neigh):
    x, codes = mixture(40 + dim, 1500, dim, xdim, ydim)
    plain = E.Dataset(eng, x)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    q_ref = E.som_batchmap(ref, plain, 3, 3.0)
    want = ref.download()
    assert not same(want, codes)
    for mask in (None, np.zeros(x.shape, dtype=np.uint8)):
        ds = E.Dataset(eng, x, mask=mask)
        cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
        q = E.som_batchmap_missing(cb, ds, 3, 3.0)
        assert same(cb.download(), want) and same(q, q_ref)
        cb.close(); ds.close()
    ref.close(); plain.close()


# ---- whole runs
@pytest.fixture(scope="module")
def small_run():
    x, codes = mixture(21, 1500, 6, 13, 5)
    xp, mask = masked(6, x)
    mask[33, :] = 1                                                    # a sample that knows nothing
    return poison(x, mask), mask, codes


@pytest.mark.gpu
@pytest.mark.parametrize("topol,neigh", [(HEXA, BUBBLE), (RECT, GAUSSIAN)])
def test_epochs_in_one_call_or_many_and_twice(E, eng, small_run, topol, neigh):
    x, mask, codes = small_run
    ds = E.Dataset(eng, x, mask=mask)
    runs = []
    for how in ("one", "one", "many"):
        cb = E.Codebook(eng, codes, topol, neigh, 13, 5)
        if how == "one":
            q = E.som_batchmap_missing(cb, ds, 5, 4.0)
        else:
            q = np.concatenate([E.som_batchmap_missing(cb, ds, 5, 4.0, start_epoch=t, count=1) for t in range(5)])
        runs.append((cb.download(), q))
        cb.close()
    ds.close()
    assert q.dtype == np.float32 and q.shape == (5,) and np.isfinite(q).all() and np.isfinite(runs[0][0]).all()
    for rows, q in runs[1:]:
        assert same(rows, runs[0][0]) and same(q, runs[0][1])
    assert not same(runs[0][0], codes)


@pytest.mark.gpu
@pytest.mark.parametrize("topol,neigh", [(HEXA, GAUSSIAN), (RECT, BUBBLE)])
def test_an_epoch_is_its_two_stages_and_its_qerror_the_oracles(E, eng, oracle, small_run, topol, neigh):
    """som_batchmap_missing == batchmap_missing_sums then batchmap_missing_combine at r_t, by bits; qerror_out[t] is
    find_qerror under the masks of the codebook the epoch started from, and the replay's chain"""
    x, mask, codes = small_run
    ds = E.Dataset(eng, x, mask=mask)
    clean = np.where(mask != 0, np.float32(0.0), x)
    a = E.Codebook(eng, codes, topol, neigh, 13, 5)
    b = E.Codebook(eng, codes, topol, neigh, 13, 5)
    for t in (0, 1, 2):
        r = E.batchmap_radius(3.5, 3, t)
        before = a.download()
        q = E.som_batchmap_missing(a, ds, 3, 3.5, start_epoch=t, count=1)
        S, Cn = E.batchmap_missing_sums(b, ds)
        E.batchmap_missing_combine(b, r, S, Cn)
        assert same(a.download(), b.download())
        want = oracle.find_qerror(before, clean, mask)[0]
        assert bits(q[0]) == bits(np.float32(want)), (t, q[0], want)
        win, d1 = R.winners(oracle, before, x, mask)
        assert bits(q[0]) == bits(R.qerror_chain(d1, win))
    first, n = 11, 1400                                                 # a window of the data
    q = E.som_batchmap_missing(a, ds, 3, 3.5, start_epoch=2, count=1, first=first, n=n)
    S, Cn = E.batchmap_missing_sums(b, ds, first, n)
    E.batchmap_missing_combine(b, E.batchmap_radius(3.5, 3, 2), S, Cn)
    assert same(a.download(), b.download())
    assert E.som_batchmap_missing(a, ds, 3, 3.0, qerror=False) is None
    a.close(); b.close(); ds.close()


@pytest.mark.gpu
def test_the_map_gets_better(E, eng):
    """2000 x 8 data around a noisy sheet, 30 % of the components hidden; a 12 x 8 hexa gaussian map started from random
    rows of the data (their own hidden components filled with the column's known mean), 10 epochs from radius 6: the last
    epoch starts from a lower quantization error than the first"""
    x, _ = mixture(31, 2000, 8, 12, 8)
    xp, mask = masked(7, x)
    rs = np.random.RandomState(32)
    known = np.where(mask == 0, x, np.float32(0.0))
    mean = (known.sum(axis=0) / (mask == 0).sum(axis=0)).astype(np.float32)
    pick = rs.choice(2000, 12 * 8, replace=False)
    codes = np.where(mask[pick] == 0, x[pick], mean).astype(np.float32)
    ds = E.Dataset(eng, xp, mask=mask)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 12, 8)
    q = E.som_batchmap_missing(cb, ds, 10, 6.0)
    assert np.isfinite(q).all() and np.isfinite(cb.download()).all() and q[-1] < q[0], q
    cb.close(); ds.close()


@pytest.mark.gpu
def test_stage_timing_counts_under_the_three_ids(E, eng, small_run):
    x, mask, codes = small_run
    ds = E.Dataset(eng, x, mask=mask)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 13, 5)
    eng.timing(True)
    eng.timing_reset()
    E.som_batchmap_missing(cb, ds, 2, 3.0, qerror=False)
    t = eng.batchmap_timing()
    eng.timing(False)
    assert t["k_batchmap_sums"][0] == 2 and t["k_batchmap_combine"][0] == 4 and t["group"][0] == 6
    cb.close(); ds.close()


# ---- the epoch over data in pieces
N = 9000


def read_state(E, eng, cb):
    """(S float64[n, dim], C float64[n, dim], q float32, samples) from the state blob"""
    addr, nbytes = E.batchmap_missing_state(cb)
    assert nbytes == 8 * cb.n * 2 * cb.dim + 16
    raw = eng.copy_to_host(addr, nbytes)
    body = raw[:-16].view(np.float64).reshape(cb.n, 2 * cb.dim)
    return body[:, :cb.dim].copy(), body[:, cb.dim:].copy(), raw[-16:-12].view(np.float32)[0], int(raw[-8:].view(np.uint64)[0])


@pytest.fixture(scope="module")
def pieces_run():
    x, codes = mixture(9085, N, 5, 9, 8)
    _, mask = masked(8, x)
    mask[1000, :] = 1                                                  # the single-row piece of "seven": a row that knows nothing
    mask[0, :] = 0
    return poison(x, mask), mask, codes


@pytest.mark.gpu
@pytest.mark.parametrize("topol,neigh,radius", [(HEXA, BUBBLE, 2.5), (RECT, GAUSSIAN, 100.0)])
def test_pieces_equal_one_call(E, eng, pieces_run, topol, neigh, radius):
    """9000 masked rows on 9 x 8, dim 5, cut at row 1, around the search's chunk, and into seven uneven pieces with a single
    row that is all masked among them: rows, q, S and C equal the one call's, by bit pattern"""
    x, mask, codes = pieces_run
    whole = E.Dataset(eng, x, mask=mask)
    tail = E.Dataset(eng, x[5000:], mask=mask[5000:])                   # a second data set
    ref = E.Codebook(eng, codes, topol, neigh, 9, 8)
    S, Cn = E.batchmap_missing_sums(ref, whole)
    q_ref = E.som_batchmap_missing(ref, whole, 1, radius, count=1)[0]
    want = ref.download()
    assert not same(want, codes)
    r = E.batchmap_radius(radius, 1, 0)

    def at(edges):
        edges = [0] + list(edges) + [N]
        return [(whole, a, b - a) for a, b in zip(edges[:-1], edges[1:])]

    seven = np.cumsum([1000, 1, 2500, 37, 4096, 300])
    cuts = {"row 1": at([1]), "4095": at([4095]), "4096": at([4096]), "4097": at([4097]), "seven": at(seven),
            "second data set": [(whole, 0, 5000), (tail, 0, N - 5000)]}
    assert len(cuts["seven"]) == 7 and cuts["seven"][1] == (whole, 1000, 1) and mask[1000].all()
    cb = E.Codebook(eng, codes, topol, neigh, 9, 8)
    for name, cut in cuts.items():
        cb.upload(codes)
        E.batchmap_missing_begin(cb)
        s0, c0, q0, n0 = read_state(E, eng, cb)
        assert not bits(s0).any() and not bits(c0).any() and bits(np.float32(q0)) == 0 and n0 == 0      # all +0.0
        for ds, first, n in cut:
            E.batchmap_missing_accumulate(cb, ds, first, n)
        s1, c1, q1, n1 = read_state(E, eng, cb)
        assert same(s1, S) and same(c1, Cn), name
        assert n1 == N and bits(np.float32(q1)) == bits(np.float32(q_ref)), name
        q = E.batchmap_missing_finish(cb, r)
        assert bits(np.float32(q)) == bits(np.float32(q_ref)), (name, q, q_ref)
        assert same(cb.download(), want), name
    E.batchmap_missing_end(cb)
    for o in (cb, ref, whole, tail):
        o.close()


@pytest.mark.gpu
def test_finish_by_group_ranges(E, eng, pieces_run):
    """_finish for one row group of the two leaves the other group's rows untouched; both ranges together are the one call"""
    x, mask, codes = pieces_run
    ds = E.Dataset(eng, x, mask=mask)
    ref = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
    E.som_batchmap_missing(ref, ds, 1, 2.5, count=1)
    want = ref.download()
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
    E.batchmap_missing_begin(cb)
    E.batchmap_missing_accumulate(cb, ds, 0, 4000)
    E.batchmap_missing_accumulate(cb, ds, 4000, 5000)
    E.batchmap_missing_finish(cb, 2.5, 1, 1)
    rows = cb.download()
    assert same(rows[:64], codes[:64]) and same(rows[64:], want[64:])
    E.batchmap_missing_finish(cb, 2.5, 0, 0)                            # an empty range writes nothing
    assert same(cb.download(), rows)
    E.batchmap_missing_finish(cb, 2.5, 0, 1)
    assert same(cb.download(), want)
    for o in (cb, ref, ds):
        o.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng):
    x, codes = mixture(50, 700, 6, 13, 5)
    xp, mask = masked(9, x)
    ds = E.Dataset(eng, xp, mask=mask)
    plain = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    lvq = E.Codebook(eng, codes, E.TOPOL_LVQ)
    shard = E.Codebook(eng, codes[:26], HEXA, BUBBLE, 13, 5, row_offset=13, n_global=65)
    other = E.Dataset(eng, x[:, :5])

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    who = "somhip_som_batchmap_missing"
    refused(lambda: E.som_batchmap_missing(shard, ds, 3, 2.0), who, "sharded")
    refused(lambda: E.som_batchmap_missing(lvq, ds, 3, 2.0), who, "without a lattice")
    refused(lambda: E.som_batchmap_missing(cb, other, 3, 2.0), who, "dimension")
    refused(lambda: E.som_batchmap_missing(cb, ds, 3, 2.0, n=2 ** 32), who, "32-bit")
    refused(lambda: E.som_batchmap_missing(cb, ds, 3, 2.0, n=0), who, "n 0")
    refused(lambda: E.som_batchmap_missing(cb, ds, 3, 2.0, first=-1), who, "first row")
    refused(lambda: E.som_batchmap_missing(cb, ds, 0, 2.0, count=0), who, "epochs 0")
    refused(lambda: E.som_batchmap_missing(cb, ds, 3, 0.5), who, "radius")
    refused(lambda: E.som_batchmap_missing(cb, ds, 3, 2.0, start_epoch=3, count=1), who, "outside")
    refused(lambda: E.batchmap_missing_sums(shard, ds), "somhip_debug_batchmap_missing_sums", "sharded")
    refused(lambda: E.batchmap_missing_sums(cb, ds, 0, 0), "somhip_debug_batchmap_missing_sums", "n 0")
    ones = np.ones((65, 6))
    refused(lambda: E.batchmap_missing_combine(lvq, 2.0, ones, ones), "somhip_debug_batchmap_missing_combine", "without a lattice")
    refused(lambda: E.batchmap_missing_combine(cb, -1.0, ones, ones), "somhip_debug_batchmap_missing_combine", "radius")
    # the plain entry points refuse masked data as before
    refused(lambda: E.som_batchmap(cb, ds, 3, 2.0), "somhip_som_batchmap", "masked components")
    refused(lambda: E.batchmap_sums(cb, ds), "somhip_debug_batchmap_sums", "masked components")

    # nothing is open yet
    refused(lambda: E.batchmap_missing_accumulate(cb, ds), "somhip_batchmap_missing_accumulate", "somhip_batchmap_missing_begin")
    refused(lambda: E.batchmap_missing_finish(cb, 2.0), "somhip_batchmap_missing_finish", "somhip_batchmap_missing_begin")
    refused(lambda: E.batchmap_missing_state(cb), "somhip_batchmap_missing_state", "somhip_batchmap_missing_begin")
    refused(lambda: E.batchmap_missing_begin(lvq), "somhip_batchmap_missing_begin", "without a lattice")
    refused(lambda: E.batchmap_missing_begin(shard), "somhip_batchmap_missing_begin", "sharded")
    E.batchmap_missing_end(cb)                                          # nothing to free: fine

    # a state of this form: the plain calls are refused by name, and the usual refusals; nothing moves
    E.batchmap_missing_begin(cb)
    E.batchmap_missing_accumulate(cb, ds, 0, 300)
    before = eng.copy_to_host(*E.batchmap_missing_state(cb))
    refused(lambda: E.batchmap_accumulate(cb, plain, 0, 10), "somhip_batchmap_accumulate", "other form")
    refused(lambda: E.batchmap_finish(cb, 2.0), "somhip_batchmap_finish", "other form")
    refused(lambda: E.batchmap_state(cb), "somhip_batchmap_state", "other form")
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, 10), "somhip_batchmap_accumulate", "masked components")
    who = "somhip_batchmap_missing_accumulate"
    refused(lambda: E.batchmap_missing_accumulate(cb, other), who, "dimension")
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, 0, 0), who, "n 0")
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, -1, 5), who, "first row")
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, 0, 2 ** 32 - 300), who, "32-bit")
    who = "somhip_batchmap_missing_finish"
    refused(lambda: E.batchmap_missing_finish(cb, -1.0), who, "radius")
    refused(lambda: E.batchmap_missing_finish(cb, 2.0, 0, 3), who, "row groups")
    assert np.array_equal(eng.copy_to_host(*E.batchmap_missing_state(cb)), before)
    assert same(cb.download(), codes)

    # the refused calls changed nothing: the accumulation goes on and ends as the one call
    ref = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    q_ref = E.som_batchmap_missing(ref, ds, 1, 2.0)[0]
    E.batchmap_missing_accumulate(cb, ds, 300, 400)
    q = E.batchmap_missing_finish(cb, 2.0)
    assert bits(np.float32(q)) == bits(np.float32(q_ref)) and same(cb.download(), ref.download())
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, 0, 10), "somhip_batchmap_missing_accumulate", "the codebook has moved")
    assert same(cb.download(), ref.download())

    # the reverse: a state of the plain form refuses the calls of this one; and opening one form closes the other
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, plain, 0, 10)
    before = eng.copy_to_host(*E.batchmap_state(cb))
    rows = cb.download()
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, 0, 10), "somhip_batchmap_missing_accumulate", "other form")
    refused(lambda: E.batchmap_missing_finish(cb, 2.0), "somhip_batchmap_missing_finish", "other form")
    refused(lambda: E.batchmap_missing_state(cb), "somhip_batchmap_missing_state", "other form")
    assert np.array_equal(eng.copy_to_host(*E.batchmap_state(cb)), before) and same(cb.download(), rows)
    E.batchmap_missing_begin(cb)
    refused(lambda: E.batchmap_accumulate(cb, plain, 0, 10), "somhip_batchmap_accumulate", "other form")
    E.batchmap_begin(cb)
    refused(lambda: E.batchmap_missing_accumulate(cb, ds, 0, 10), "somhip_batchmap_missing_accumulate", "other form")

    # a writer of the rows closes the state
    writers = (lambda: cb.upload(codes), lambda: E.som_batchmap_missing(cb, ds, 1, 2.0), lambda: E.som_batchmap(cb, plain, 1, 2.0),
               lambda: E.batchmap_missing_combine(cb, 2.0, np.ones((65, 6)), np.ones((65, 6))))
    for writer in writers:
        E.batchmap_missing_begin(cb)
        E.batchmap_missing_accumulate(cb, ds, 0, 10)
        writer()
        rows = cb.download()
        refused(lambda: E.batchmap_missing_accumulate(cb, ds, 10, 10), "somhip_batchmap_missing_accumulate", "somhip_batchmap_missing_begin")
        refused(lambda: E.batchmap_missing_finish(cb, 2.0), "somhip_batchmap_missing_finish", "somhip_batchmap_missing_begin")
        assert same(cb.download(), rows)
    E.batchmap_missing_begin(cb)
    E.batchmap_missing_accumulate(cb, ds)
    for o in (cb, ref, lvq, shard, ds, plain, other):                   # (destroying the codebook frees the open state)
        o.close()


# ---- the tool
def write_inputs(tmp_path, x, mask, codes, topol, neigh, xdim, ydim):
    from som_lvq_pak_amd import textio
    dat, cod = tmp_path / "d.dat", tmp_path / "m.cod"
    d = textio.Entries()
    d.dim, d.points, d.mask = x.shape[1], x, mask
    textio.write_entries(str(dat), d)
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = x.shape[1], topol, neigh, xdim, ydim, codes
    textio.write_entries(str(cod), m)
    return dat, cod


@pytest.fixture(scope="module")
def tool_run(E, eng, tools, tmp_path_factory):
    """bsom -missing -v on a masked text file of 700 rows on a 9 x 8 map, with a row of x alone in it"""
    tmp = tmp_path_factory.mktemp("bsom_missing")
    rs = np.random.RandomState(43)
    x = (np.round(rs.standard_normal((700, 5)) * 16) / 16).astype(np.float32)       # values that "%g" keeps
    codes = (np.round(rs.standard_normal((9 * 8, 5)) * 16) / 16).astype(np.float32)
    mask = (rs.uniform(size=x.shape) < 0.3).astype(np.uint8)
    mask[6, :] = 1
    dat, cod = write_inputs(tmp, x, mask, codes, HEXA, GAUSSIAN, 9, 8)
    args = ["-cin", cod, "-din", dat, "-epochs", 3, "-radius", 3, "-v", "-missing"]
    out = tmp / "plain.cod"
    p = run("bsom", *args, "-cout", out)
    assert p.returncode == 0, p.stderr
    return tmp, args, out.read_bytes(), p.stdout, (x, mask, codes)


@pytest.mark.gpu
def test_bsom_missing_writes_the_engines_map(E, eng, tool_run):
    from som_lvq_pak_amd import textio
    tmp, args, cod_bytes, lines, (x, mask, codes) = tool_run
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 9, 8)
    ds = E.Dataset(eng, poison(x, mask), mask=mask)
    q = E.som_batchmap_missing(cb, ds, 3, 3.0)
    rows = cb.download()
    cb.close(); ds.close()
    got = textio.read_entries(str(tmp / "plain.cod"))[0]
    assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (5, HEXA, GAUSSIAN, 9, 8) and got.mask is None
    printed = np.array([[np.float32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=np.float32)
    assert np.array_equal(bits(got.points), bits(printed))
    assert lines.strip().split("\n") == ["epoch %d radius %.9g qerror %.9g" % (t, float(E.batchmap_radius(3.0, 3, t)), float(q[t]))
                                         for t in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("buffer", [1, 7, 4096, 100000])
def test_bsom_missing_buffer_writes_the_same_bytes(tool_run, buffer):
    tmp, args, cod_bytes, lines, _ = tool_run
    out = tmp / ("buffer_%d.cod" % buffer)
    p = run("bsom", *args, "-cout", out, "-buffer", buffer)
    assert p.returncode == 0, p.stderr
    assert out.read_bytes() == cod_bytes and p.stdout == lines


@pytest.mark.gpu
def test_bsom_missing_on_unmasked_data_and_masked_data_without_it(tool_run):
    """an unmasked file with -missing equals bsom without it, byte for byte; masked data without -missing are refused as ever"""
    tmp, args, _, _, (x, mask, codes) = tool_run
    (tmp / "u").mkdir()
    dat, cod = write_inputs(tmp / "u", x, None, codes, RECT, BUBBLE, 9, 8)
    base = ["-cin", cod, "-din", dat, "-epochs", 3, "-radius", 3, "-v"]
    a, b, c = tmp / "u" / "a.cod", tmp / "u" / "b.cod", tmp / "u" / "c.cod"
    pa = run("bsom", *base, "-cout", a)
    pb = run("bsom", *base, "-cout", b, "-missing")
    pc = run("bsom", *base, "-cout", c, "-missing", "-buffer", 300)
    assert pa.returncode == 0 and pb.returncode == 0 and pc.returncode == 0, (pa.stderr, pb.stderr, pc.stderr)
    assert a.read_bytes() == b.read_bytes() == c.read_bytes() and pa.stdout == pb.stdout == pc.stdout
    out = tmp / "refused.cod"
    p = run("bsom", *[s for s in args if s != "-missing"], "-cout", out)
    assert p.returncode == 1 and "masked components" in p.stderr and not out.exists()
