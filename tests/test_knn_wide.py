"""Wide k-NN: somhip_find_winners for 9 <= knn <= 256 (the K1w route: every distance of a chunk of samples, then a select
per sample in a 1024-key LDS pool fed in strides of 256 rows) against the oracle's find_winner_knn, bit for bit.

The select's own boundaries are the strides (256 rows) and its flushes: the first flush comes before the stride that
starts at row 768 whatever knn is (every key passes until then), and while every key keeps passing (equal rows,
falling distances) one more every 768 rows; the row counts below sit just before, at and after those.

Oracle index -1 / diff FLT_MAX is the engine's -1 / -1.0f; -2 / -1.0f (every component masked) is the same on both."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

TIE_FIRST, TIE_KNN = 0, 1
TOPOL_HEXA = 3
KNNS = (9, 16, 17, 64, 255, 256)
ROWS = (1, 5, 9, 63, 64, 65, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 1300)
DIST_BUDGET = 256 << 20           # bytes of distances per chunk (host_scan.inc: KNN_DIST_BYTES)


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


# ------------------------------------------------------------------------------------------------ without a GPU
def test_limit_and_symbols(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    assert lib.somhip_knn_max() == 256 == engine.KNN_MAX
    assert _lib.SIGNATURES["somhip_knn_max"] == (C.c_int, [])
    assert _lib.SIGNATURES["somhip_knn_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert engine.ROUTES[4] == "wide" and hasattr(engine.Engine, "knn_timing")
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert "#define SOMHIP_KNN_MAX 256" in hdr


def test_null_handles_are_errors_not_crashes(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 2)(), (C.c_double * 2)()
    assert lib.somhip_knn_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_knn_timing: null engine"
    idx, diff = (C.c_int32 * 9)(), (C.c_float * 9)()
    assert lib.somhip_find_winners(None, None, 0, 1, 9, TIE_KNN, idx, diff, None) != 0
    assert lib.somhip_last_error().decode() == "somhip_find_winners: null handle"
    out = (C.c_int32 * 8)()
    assert lib.somhip_debug_scan_plan(None, None, 1, 9, out) != 0
    assert lib.somhip_last_error().decode() == "somhip_debug_scan_plan: null handle"


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    e.set_scan_mode("direct")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def witness(oracle, codes, xs, knn, mask=None):
    """find_winner_knn by the oracle, in the engine's conventions"""
    widx, wdiff, wret = oracle.winners(codes, xs, knn, True, mask)
    wdiff = np.where(widx == -1, np.float32(-1.0), wdiff).astype(np.float32)
    return widx.astype(np.int32), wdiff, wret


def same(got, want, what=""):
    idx, diff, ret = got
    widx, wdiff, wret = want
    bad = np.nonzero((idx != widx).any(axis=1) | (bits(diff) != bits(wdiff)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d samples differ; first at %d: got %s %s, oracle %s %s" % (
        what, bad.size, idx.shape[0], bad[0], idx[bad[0]], diff[bad[0]], widx[bad[0]], wdiff[bad[0]])
    assert np.array_equal(ret, wret), what


def search(E, eng, codes, x, knn, mask=None, first=0, count=None, **cbkw):
    cb = E.Codebook(eng, codes, **cbkw)
    ds = E.Dataset(eng, x, mask=mask)
    try:
        return E.find_winners(cb, ds, first, count, knn=knn, tie=TIE_KNN)
    finally:
        cb.close()
        ds.close()


@pytest.fixture(scope="module")
def edge_data():
    rs = np.random.RandomState(20)
    return rs.standard_normal((max(ROWS), 5)).astype(np.float32), rs.standard_normal((33, 5)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("knn", KNNS)
@pytest.mark.parametrize("rows", ROWS)
def test_rows_and_knn_at_the_selects_edges(E, eng, oracle, edge_data, rows, knn):
    codes, x = edge_data[0][:rows], edge_data[1]
    got = search(E, eng, codes, x, knn)
    same(got, witness(oracle, codes, x, knn), "%d rows, knn %d" % (rows, knn))
    if rows < knn:                              # fewer rows than neighbours: the rest of every list is empty
        assert (got[0][:, rows:] == -1).all() and (got[1][:, rows:] == -1.0).all() and (got[0][:, :rows] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (9, 64))
@pytest.mark.parametrize("dim", (1, 3, 4, 5, 37))
def test_dims_and_sample_counts(E, eng, oracle, dim, knn):
    rs = np.random.RandomState(100 + dim)
    codes = rs.standard_normal((300, dim)).astype(np.float32)
    x = rs.standard_normal((40, dim)).astype(np.float32)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    try:
        want = witness(oracle, codes, x, knn)
        for first, count in ((0, 1), (0, 31), (0, 32), (0, 33), (3, 33), (30, 25)):     # the last one wraps: 30 + 25 > 40
            win = (first + np.arange(count)) % 40
            got = E.find_winners(cb, ds, first, count, knn=knn, tie=TIE_KNN)
            same(got, tuple(w[win] for w in want), "dim %d, rows [%d, +%d)" % (dim, first, count))
    finally:
        cb.close()
        ds.close()


def pattern(name, n=1300, m=16, d=5):
    rs = np.random.RandomState(7)
    x = rs.standard_normal((m, d)).astype(np.float32)
    if name == "identical":
        codes = np.tile(rs.standard_normal((1, d)).astype(np.float32), (n, 1))
    elif name in ("falling", "rising"):
        # the rows on a line beyond every sample, integer coordinates: exact distances, strictly monotone in the row
        codes = np.zeros((n, d), dtype=np.float32)
        codes[:, 0] = 100.0 + (np.arange(n)[::-1] if name == "falling" else np.arange(n))
        x = rs.randint(-20, 21, size=(m, d)).astype(np.float32)
    elif name == "blocks":
        codes = rs.standard_normal((n // 70 + 1, d)).astype(np.float32)[np.arange(n) // 70]
    elif name == "integers":
        codes = rs.randint(-2, 3, size=(n, d)).astype(np.float32)
        x = rs.randint(-2, 3, size=(m, d)).astype(np.float32)
    else:
        codes = rs.standard_normal((n, d)).astype(np.float32)
    return codes, x


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (9, 64, 256))
@pytest.mark.parametrize("name", ("identical", "falling", "rising", "blocks", "integers", "gaussian"))
def test_value_patterns(E, eng, oracle, name, knn):
    codes, x = pattern(name)
    n = codes.shape[0]
    got = search(E, eng, codes, x, knn)
    same(got, witness(oracle, codes, x, knn), "%s, knn %d" % (name, knn))
    if name in ("identical", "falling"):        # the later row first / the nearest rows are the last ones
        assert (got[0] == n - 1 - np.arange(knn)[None, :]).all()
    if name == "rising":
        assert (got[0] == np.arange(knn)[None, :]).all()
    if name == "blocks":                         # ties inside a block of duplicates: descending rows
        d0 = got[1][:, :-1] == got[1][:, 1:]
        assert d0.any() and (got[0][:, :-1][d0] > got[0][:, 1:][d0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (9, 64))
def test_masked_data(E, eng, oracle, knn):
    rs = np.random.RandomState(31)
    codes = rs.standard_normal((300, 7)).astype(np.float32)
    x = rs.standard_normal((35, 7)).astype(np.float32)
    mask = (rs.random_sample((35, 7)) < 0.3).astype(np.uint8)
    mask[4] = 1
    mask[4, 2] = 0                               # a single live component
    mask[11] = 1                                 # nothing live: ret 0, index -2
    mask[20] = 0
    got = search(E, eng, codes, x, knn, mask=mask)
    same(got, witness(oracle, codes, x, knn, mask), "masked, knn %d" % knn)
    assert got[2][11] == 0 and (got[0][11] == -2).all() and (got[1][11] == -1.0).all()
    assert (np.delete(got[2], 11) == knn).all()
    # a masked component is skipped, not added as zero: the single live component alone gives the distances
    t = codes[got[0][4], 2] - x[4, 2]
    assert np.array_equal(bits(got[1][4]), bits(t * t))


@pytest.mark.gpu
def test_chunks_and_their_timing(E, eng, oracle):
    """32768 rows: 4 * 512 groups * 64 bytes of distances per sample, 2048 samples per chunk of the 256 MiB budget; 2100
    samples are a whole chunk and a partial one, with one launch of each stage per chunk"""
    rs = np.random.RandomState(5)
    n, m, knn = 32768, 2100, 9
    codes = rs.standard_normal((n, 2)).astype(np.float32)
    x = rs.standard_normal((m, 2)).astype(np.float32)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    try:
        plan = E.scan_plan(cb, ds, m, knn)
        assert plan == {"route": "wide", "chunk": DIST_BUDGET // (4 * n)} and plan["chunk"] == 2048
        assert plan["chunk"] < m and m % plan["chunk"] != 0
        eng.timing(True)
        eng.timing_reset()
        got = E.find_winners(cb, ds, 0, m, knn=knn, tie=TIE_KNN)
        t = eng.knn_timing()
        assert t["k_knn_dist"][0] == 2 and t["k_knn_select"][0] == 2
        assert t["k_knn_dist"][1] > 0.0 and t["k_knn_select"][1] > 0.0
        eng.timing_reset()
        E.find_winners(cb, ds, 0, 33, knn=knn, tie=TIE_KNN)
        t = eng.knn_timing()
        assert t["k_knn_dist"][0] == 1 and t["k_knn_select"][0] == 1
        assert "k_knn_dist" not in eng.timing_table()                    # the published kernel table is closed
    finally:
        eng.timing(False)
        cb.close()
        ds.close()
    same(got, witness(oracle, codes, x, knn), "two chunks")


@pytest.mark.gpu
def test_patch_storage_and_row_shards(E, eng, oracle):
    """a 16 x 8 hexa map is stored in 8x8 patches: indices come back as units; its two halves as row shards answer with
    their own 20 nearest under global indices, and merged by (diff, later row first) they are the whole map's answer"""
    rs = np.random.RandomState(77)
    knn = 20
    codes = rs.randint(-3, 4, size=(128, 6)).astype(np.float32)          # many ties, also across the shards
    x = rs.randint(-3, 4, size=(33, 6)).astype(np.float32)
    want = witness(oracle, codes, x, knn)
    whole = search(E, eng, codes, x, knn, topol=TOPOL_HEXA, neigh=1, xdim=16, ydim=8)
    same(whole, want, "8x8-patch map")
    parts = [search(E, eng, codes[o:o + 64], x, knn, topol=TOPOL_HEXA, neigh=1, xdim=16, ydim=8, row_offset=o, n_global=128)
             for o in (0, 64)]
    assert parts[0][0].max() < 64 <= parts[1][0].min()
    idx = np.concatenate([p[0] for p in parts], axis=1).astype(np.int64)
    diff = np.concatenate([p[1] for p in parts], axis=1)
    key = (bits(diff).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64))
    order = np.argsort(key, axis=1)[:, :knn]
    merged = (np.take_along_axis(idx, order, 1).astype(np.int32), np.take_along_axis(diff, order, 1), parts[0][2])
    same(merged, want, "two row shards merged")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("direct", "mfma_bf16"))
def test_no_change_below_nine(E, oracle, mode):
    rs = np.random.RandomState(9)
    codes = rs.standard_normal((3000, 24)).astype(np.float32)
    x = rs.standard_normal((64, 24)).astype(np.float32)
    e = E.Engine(0)
    try:
        e.set_scan_mode(mode)
        cb, ds = E.Codebook(e, codes), E.Dataset(e, x)
        i8, d8, r8 = E.find_winners(cb, ds, knn=8, tie=TIE_KNN)
        i9, d9, r9 = E.find_winners(cb, ds, knn=9, tie=TIE_KNN)
        assert np.array_equal(i9[:, :8], i8) and np.array_equal(bits(d9[:, :8]), bits(d8))
        assert (r8 == 8).all() and (r9 == 9).all()
        same((i8, d8, r8), witness(oracle, codes, x, 8), "knn 8")
        # the plans of the top-8 search as the code before the wide route answered them
        bf16 = mode == "mfma_bf16"
        none = {"kth": 1, "bf16": bf16, "l1_ring": False, "by_group": False, "l2_global": False, "fused_gmin": False}
        assert E.scan_plan(cb, ds, 64, 8) == dict(none, route="direct")
        assert E.scan_plan(cb, ds, 64, 9) == {"route": "wide", "chunk": 4096}
        big = E.Codebook(e, np.zeros((8192, 32), dtype=np.float32))
        ds32 = E.Dataset(e, np.zeros((256, 32), dtype=np.float32))
        assert E.scan_plan(big, ds32, 256, 8) == dict(none, route="one_level" if bf16 else "direct")
    finally:
        e.close()


@pytest.mark.gpu
def test_refusals_and_plan(E, eng):
    from som_lvq_pak_amd import _lib
    lib = eng.lib
    rs = np.random.RandomState(1)
    cb = E.Codebook(eng, rs.standard_normal((100, 3)).astype(np.float32))
    ds = E.Dataset(eng, rs.standard_normal((10, 3)).astype(np.float32))
    try:
        for knn, tie, text in ((0, TIE_KNN, "knn 0 not in 1..256"), (257, TIE_KNN, "knn 257 not in 1..256"),
                               (-1, TIE_KNN, "not in 1..256"), (9, TIE_FIRST, "needs SOMHIP_TIE_KNN")):
            with pytest.raises(_lib.SomhipError, match=text):
                _call(cb, ds, knn, tie)
        idx = np.zeros((10, 9), np.int32)
        diff = np.zeros((10, 9), np.float32)
        for pi, pd in ((None, diff.ctypes.data_as(_lib.c_float_p)), (idx.ctypes.data_as(_lib.c_i32_p), None)):
            assert lib.somhip_find_winners(cb.h, ds.h, 0, 10, 9, TIE_KNN, pi, pd, None) != 0
            assert "null output" in lib.somhip_last_error().decode()
        assert E.scan_plan(cb, ds, 10, 9)["route"] == "wide" and E.scan_plan(cb, ds, 10, 256)["route"] == "wide"
        for want in (3, 5, 6, 7, 0, 257):
            with pytest.raises(_lib.SomhipError):
                E.scan_plan(cb, ds, 10, want)
        assert E.scan_plan(cb, ds, 10, 8)["route"] == "direct"
        # ret may be NULL on the wide route too
        assert lib.somhip_find_winners(cb.h, ds.h, 0, 10, 9, TIE_KNN, idx.ctypes.data_as(_lib.c_i32_p),
                                       diff.ctypes.data_as(_lib.c_float_p), None) == 0
        assert (idx >= 0).all() and (np.diff(diff, axis=1) >= 0).all()
    finally:
        cb.close()
        ds.close()


def _call(cb, ds, knn, tie):
    """find_winners with output arrays of a harmless size whatever knn says"""
    from som_lvq_pak_amd import _lib
    idx = np.zeros((10, 300), np.int32)
    diff = np.zeros((10, 300), np.float32)
    ret = np.zeros(10, np.int32)
    _lib.check(cb.e.lib.somhip_find_winners(cb.h, ds.h, 0, 10, knn, tie, idx.ctypes.data_as(_lib.c_i32_p),
                                            diff.ctypes.data_as(_lib.c_float_p), ret.ctypes.data_as(_lib.c_i32_p)))
