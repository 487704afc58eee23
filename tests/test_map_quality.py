"""somhip_map_quality (K1q): topographic error, hit counts and error sums per unit, formed on the device behind the
top-2 search under SOMHIP_TIE_FIRST, against the CPU replay in map_quality_replay.py (the oracle's find_winner_euc twice,
the reference's lattice arithmetic, ordered np.float64 / float chains).  Every comparison is exact: integers equal,
doubles and floats by bit pattern."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from map_quality_replay import Replay, adjacent

HEXA, RECT = 3, 4
BUBBLE = 1


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    assert hasattr(lib, "somhip_map_quality") and hasattr(lib, "somhip_map_quality_timing")
    assert _lib.SIGNATURES["somhip_map_quality"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _lib.c_u32_p,
                                                               _lib.c_double_p, C.c_float, C.POINTER(_lib.QualityTotals)])
    assert _lib.SIGNATURES["somhip_map_quality_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.QualityTotals._fields_] == ["searched", "topo_defined", "topo_errors", "qerror"]
    assert C.sizeof(_lib.QualityTotals) == 32
    assert hasattr(engine, "map_quality") and hasattr(engine.Engine, "map_quality_timing")
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert "typedef struct { int64_t searched, topo_defined, topo_errors; float qerror; } somhip_quality_totals;" in hdr
    assert "somhip_map_quality(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count," in hdr
    assert "somhip_map_quality_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]);" in hdr


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


def same(got, want):
    """(totals, hits, qsum) equal: integers as integers, floats and doubles by their bits"""
    gt, gh, gq = got
    wt, wh, wq = want
    for k in ("searched", "topo_defined", "topo_errors"):
        assert int(gt[k]) == int(wt[k]), (k, gt, wt)
    assert np.float32(gt["qerror"]).view(np.uint32) == np.float32(wt["qerror"]).view(np.uint32), (gt, wt)
    assert gh.dtype == np.uint32 and gq.dtype == np.float64
    assert np.array_equal(gh, wh)
    assert np.array_equal(gq.view(np.uint64), wq.view(np.uint64))


def mixture(seed, n, d, xdim, ydim, noise=0.4):
    """a map laid out as a noisy sheet in the data space and data scattered around the sheet: an ordered map with some
    folds, so that neighbouring and distant (b1, b2) both occur"""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((2, d)).astype(np.float32)
    u = np.arange(xdim * ydim)
    pos = np.stack([u % xdim, u // xdim], axis=1).astype(np.float32)
    codes = (pos @ v + noise * rs.standard_normal((xdim * ydim, d))).astype(np.float32)
    at = (rs.uniform(size=(n, 2)) * [xdim, ydim]).astype(np.float32)
    x = (at @ v + 0.5 * rs.standard_normal((n, d))).astype(np.float32)
    return x, codes


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol", [(1, 1, HEXA), (2, 1, RECT), (1, 2, HEXA), (63, 1, HEXA), (1, 64, RECT),
                                             (13, 5, HEXA), (16, 16, RECT), (16, 16, HEXA), (257, 1, RECT), (1030, 1, HEXA)])
def test_unit_pass_edges(E, eng, oracle, xdim, ydim, topol):
    """1, 2, 63, 64, 65, 256 and 257 units and more than 1024: one lane, a wave less one, a wave, a wave and one, a
    workgroup, a workgroup and one, five workgroups; a map of one unit has no second-best unit"""
    units = xdim * ydim
    x, codes = mixture(100 + units, 700, 3, xdim, ydim)
    cb = E.Codebook(eng, codes, topol, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x)
    want = Replay(oracle, codes, xdim, ydim, topol, x).run()
    got = E.map_quality(cb, ds)
    same(got, want)
    assert got[0]["searched"] == 700 and got[0]["topo_defined"] == (700 if units > 1 else 0)
    if units == 1:
        assert got[0]["topo_errors"] == 0 and got[1][0] == 700
    cb.close(); ds.close()


@pytest.fixture(scope="module")
def chunked(E, eng, oracle):
    """a 13 x 5 map of dim 5 over 6000 rows: runs of more than 6000 samples wrap past the data's end"""
    x, codes = mixture(7, 6000, 5, 13, 5)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    ds = E.Dataset(eng, x)
    yield cb, ds, Replay(oracle, codes, 13, 5, HEXA, x)
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first,count", [(0, 1), (5990, 1), (0, 4095), (5990, 4095), (0, 4096), (5990, 4096), (3, 4097),
                                         (5990, 4097), (0, 8193), (5990, 8193)])
def test_chunk_edges(E, chunked, first, count):
    """one sample, a chunk of 4096 less one, whole, and one more, two chunks and one; from row 0 and from a row near the
    end, so that the run wraps"""
    cb, ds, rep = chunked
    same(E.map_quality(cb, ds, first, count), rep.run(first, count))


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 4096, 5000])
def test_a_run_cut_in_two_gives_the_bits_of_the_whole(E, chunked, cut):
    cb, ds, rep = chunked
    first, count = 5990, 8193
    whole = E.map_quality(cb, ds, first, count)
    same(whole, rep.run(first, count))
    t1, h, q = E.map_quality(cb, ds, first, cut)
    t2, h, q = E.map_quality(cb, ds, first + cut, count - cut, hits=h, qsum=q, qerror=t1["qerror"])
    for k in ("searched", "topo_defined", "topo_errors"):
        t2[k] += t1[k]
    same((t2, h, q), whole)


@pytest.mark.gpu
def test_ties_follow_the_first_rule(E, eng, oracle):
    """integer-valued data and a 6 x 5 map with equal rows: 7 = 8 (neighbours), 3 = 20 (not neighbours), 11 = 12 = 25 (three
    equal rows); sample 0 equals unit 14.  b2 is the lowest index among equal distances, where find_winner_knn takes a
    later row."""
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 4, size=(30, 3)).astype(np.float32)
    codes[8] = codes[7]; codes[20] = codes[3]; codes[12] = codes[11]; codes[25] = codes[11]
    x = rs.randint(0, 4, size=(600, 3)).astype(np.float32)
    x[0] = codes[14]; x[1] = codes[7]; x[2] = codes[3]; x[3] = codes[11]
    for topol in (HEXA, RECT):
        rep = Replay(oracle, codes, 6, 5, topol, x)
        knn2 = oracle.winners(codes, x, 2, True)[0][:, 1]
        differ = np.nonzero(knn2 != rep.b2)[0]
        assert len(differ) > 0, "no sample of this case tells the FIRST rule from find_winner_knn's"
        assert rep.d1[0] == 0.0 and np.any(rep.b2[differ] >= 0)
        # equal distances to the best and the second-best unit, and three equal rows, do occur
        d = ((x[:, None, :] - codes[None, :, :]) ** 2).sum(axis=2)
        srt = np.sort(d, axis=1)
        assert np.any(srt[:, 0] == srt[:, 1]) and np.any(srt[:, 0] == srt[:, 2])
        cb = E.Codebook(eng, codes, topol, BUBBLE, 6, 5)
        ds = E.Dataset(eng, x)
        same(E.map_quality(cb, ds), rep.run())
        # per sample: the error flag is the FIRST rule's
        for s in differ[:40]:
            t, h, _ = E.map_quality(cb, ds, int(s), 1)
            assert t["topo_errors"] == int(rep.error[s]) and h[rep.b1[s]] == 1
        cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("topol", [HEXA, RECT])
def test_adjacency_of_every_ordered_pair(E, eng, oracle, topol):
    """(b1, b2) over every ordered pair of the units of a 5 x 4 map of dim 2, each as a run of one sample: all six
    neighbours of a hexagonal lattice from even and odd rows, the diagonals of a rectangular one (2.0), the hexagonal
    pairs at 3.0.  No single set of 20 points of the plane has every ordered pair as somebody's two nearest (the pairs
    with a non-empty order-2 Voronoi cell are at most 3 * 20 - 6), so the pair is made by the codebook: unit a at the
    sample, unit b next to it, every other unit far away; the sample stays the same."""
    xdim, ydim, units = 5, 4, 20
    x = np.array([[0.25, 0.0]], dtype=np.float32)
    ds = E.Dataset(eng, x)
    far = np.stack([100.0 + 3.0 * np.arange(units), 50.0 + 0.0 * np.arange(units)], axis=1).astype(np.float32)
    cb = E.Codebook(eng, far, topol, BUBBLE, xdim, ydim)
    seen, errors = set(), 0
    for a in range(units):
        for b in range(units):
            if a == b:
                continue
            codes = far.copy()
            codes[a] = (0.0, 0.0)
            codes[b] = (1.0, 0.0)
            cb.upload(codes)
            rep = Replay(oracle, codes, xdim, ydim, topol, x)
            assert (rep.b1[0], rep.b2[0]) == (a, b)
            seen.add((a, b))
            t, h, q = E.map_quality(cb, ds, 0, 1)
            want = not adjacent(topol, xdim, a, b)
            assert bool(rep.error[0]) == want
            assert (t["searched"], t["topo_defined"], t["topo_errors"]) == (1, 1, int(want)), (a, b, t)
            assert h[a] == 1 and h.sum() == 1 and q[a] == 0.25
            errors += int(want)
    assert len(seen) == units * (units - 1)
    # neighbours of the lattice: rect 2 * (4 * 4 + 5 * 3) ordered pairs; hexa those and the 2 * 4 * 3 diagonal ones
    assert units * (units - 1) - errors == (62 if topol == RECT else 62 + 24)
    if topol == HEXA:
        # unit (2, 1) on an odd row and unit (2, 2) on an even row have six neighbours each
        for u, nb in ((7, {6, 8, 2, 3, 12, 13}), (12, {11, 13, 6, 7, 16, 17})):
            assert {v for v in range(units) if v != u and adjacent(HEXA, xdim, u, v)} == nb
    cb.close(); ds.close()


@pytest.mark.gpu
def test_masked_samples(E, eng, oracle):
    """data with missing components, rows with nothing left at the first and last position of both chunks of a run of
    4100 samples and elsewhere: searched < count, and the chains skip exactly those rows"""
    rs = np.random.RandomState(5)
    x, codes = mixture(21, 4100, 5, 13, 5)
    mask = (rs.uniform(size=x.shape) < 0.2).astype(np.uint8)
    empty = [0, 4095, 4096, 4099, 17, 2048, 2049]
    mask[empty] = 1
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    ds = E.Dataset(eng, x, mask=mask)
    assert E.scan_plan(cb, ds, 4096, 2)["route"] == "masked"
    rep = Replay(oracle, codes, 13, 5, HEXA, x, mask)
    want = rep.run()
    n_empty = int(mask.all(axis=1).sum())
    assert n_empty >= len(empty) and want[0]["searched"] == 4100 - n_empty
    got = E.map_quality(cb, ds)
    same(got, want)
    assert got[1].sum() == 4100 - n_empty
    same(E.map_quality(cb, ds, 4090, 20), rep.run(4090, 20))          # wraps over rows 4095, 4096, 4099 and 0
    t, h, q = E.map_quality(cb, ds, 4095, 2)                           # nothing but empty rows
    assert (t["searched"], t["topo_defined"], t["topo_errors"], float(t["qerror"])) == (0, 0, 0, 0.0)
    assert not h.any() and not q.any()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_prefilter_route(E, eng, oracle):
    """64 x 64 units of dim 128: the top-2 search goes through the MFMA pre-filter and the exact re-rank"""
    x, codes = mixture(31, 200, 128, 64, 64, noise=1.6)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 64, 64)
    ds = E.Dataset(eng, x)
    assert E.scan_plan(cb, ds, 200, 2)["route"] in ("one_level", "two_level")
    same(E.map_quality(cb, ds), Replay(oracle, codes, 64, 64, HEXA, x).run())
    cb.close(); ds.close()


@pytest.mark.gpu
def test_direct_route_and_agreement_with_the_winner_search(E, eng, oracle):
    """a small map takes the direct scan; qerror is the float the qerror path sums from somhip_find_winners, and hits the
    histogram of its winners"""
    x, codes = mixture(41, 900, 7, 8, 6)
    cb = E.Codebook(eng, codes, RECT, BUBBLE, 8, 6)
    ds = E.Dataset(eng, x)
    assert E.scan_plan(cb, ds, 900, 2)["route"] == "direct"
    got = E.map_quality(cb, ds)
    same(got, Replay(oracle, codes, 8, 6, RECT, x).run())
    idx, diff, ret = E.find_winners(cb, ds, knn=1)
    q = np.float32(0.0)
    for d, r in zip(diff[:, 0], ret):
        if r:
            q = np.float32(np.float64(q) + np.sqrt(np.float64(d)))
    assert got[0]["qerror"].view(np.uint32) == q.view(np.uint32)
    assert got[0]["qerror"] == np.float32(oracle.qerror_from_diffs(diff[:, 0], ret))
    assert int(got[1].sum()) == got[0]["searched"] == 900
    assert np.array_equal(got[1], np.bincount(idx[ret != 0, 0], minlength=48).astype(np.uint32))
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_and_the_no_op(E, eng):
    from som_lvq_pak_amd import _lib
    lib = eng.lib
    x, codes = mixture(51, 40, 4, 4, 3)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 4, 3)
    ds = E.Dataset(eng, x)
    tot = _lib.QualityTotals()

    def refused(cbh, dsh, first, count, out, what):
        assert lib.somhip_map_quality(cbh, dsh, first, count, None, None, 0.0, out) != 0
        msg = lib.somhip_last_error().decode()
        assert msg.startswith("somhip_map_quality: ") and what in msg, msg

    refused(None, ds.h, 0, 1, C.byref(tot), "null handle")
    refused(cb.h, None, 0, 1, C.byref(tot), "null handle")
    refused(cb.h, ds.h, 0, 1, None, "null output")
    other = E.Engine(0)
    ds_other = E.Dataset(other, x)
    refused(cb.h, ds_other.h, 0, 1, C.byref(tot), "different engines")
    ds_other.close(); other.close()
    ds3 = E.Dataset(eng, x[:, :3].copy())
    refused(cb.h, ds3.h, 0, 1, C.byref(tot), "dimension")
    ds3.close()
    shard = E.Codebook(eng, codes[4:8], HEXA, BUBBLE, 4, 3, row_offset=4, n_global=12)
    refused(shard.h, ds.h, 0, 1, C.byref(tot), "shard")
    shard.close()
    plain = E.Codebook(eng, codes)                                       # an LVQ codebook: no lattice
    refused(plain.h, ds.h, 0, 1, C.byref(tot), "lattice")
    plain.close()
    refused(cb.h, ds.h, 0, 1 << 32, C.byref(tot), "count")
    # count <= 0: success, the totals zero, the chain where it was, hits and qsum untouched
    hits = np.arange(12, dtype=np.uint32) + 5
    qsum = np.arange(12, dtype=np.float64) + 0.5
    for count in (0, -3):
        tot.searched = tot.topo_defined = tot.topo_errors = 9
        assert lib.somhip_map_quality(cb.h, ds.h, 0, count, hits.ctypes.data_as(_lib.c_u32_p),
                                      qsum.ctypes.data_as(_lib.c_double_p), 2.5, C.byref(tot)) == 0
        assert (tot.searched, tot.topo_defined, tot.topo_errors, tot.qerror) == (0, 0, 0, 2.5)
        assert np.array_equal(hits, np.arange(12) + 5) and np.array_equal(qsum, np.arange(12) + 0.5)
    # null arrays are allowed: the totals alone
    assert lib.somhip_map_quality(cb.h, ds.h, 0, 40, None, None, 0.0, C.byref(tot)) == 0
    assert tot.searched == 40 and tot.topo_defined == 40
    n, ms = (C.c_int64 * 2)(), (C.c_double * 2)()
    assert lib.somhip_map_quality_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_map_quality_timing: null engine"
    cb.close(); ds.close()


@pytest.mark.gpu
def test_python_mirror_continues_a_run_and_times_its_kernels(E, eng, oracle):
    x, codes = mixture(61, 500, 6, 7, 5)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 7, 5)
    ds = E.Dataset(eng, x)
    rep = Replay(oracle, codes, 7, 5, HEXA, x)
    eng.timing(True)
    eng.timing_reset()
    t, h, q = E.map_quality(cb, ds, 0, 123)
    same((t, h, q), rep.run(0, 123))
    h0, q0 = h.copy(), q.copy()
    t2, h2, q2 = E.map_quality(cb, ds, 123, 377, hits=h, qsum=q, qerror=t["qerror"])
    assert np.array_equal(h, h0) and np.array_equal(q, q0)              # the arrays passed in are left alone
    want = rep.run()
    for k in ("searched", "topo_defined", "topo_errors"):
        t2[k] += t[k]
    same((t2, h2, q2), want)
    tm = eng.map_quality_timing()
    eng.timing(False)
    assert tm["k_quality_pairs"][0] == 2 and tm["k_quality_units"][0] == 2
    assert tm["k_quality_pairs"][1] > 0 and tm["k_quality_units"][1] > 0
    assert "k_quality_pairs" not in eng.timing_table()                  # the published table is closed
    cb.close(); ds.close()
