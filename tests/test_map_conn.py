"""somhip_map_connectivity (K1c): per ordered pair (best unit, second-best unit) the number of samples that have it, counted
on the device behind the top-2 search under SOMHIP_TIE_FIRST and kept in a pair table (somhip_conn), against the CPU replay
in map_conn_replay.py (map_quality_replay.pairs -- the oracle's find_winner_euc twice -- and np.unique).  Every result is
an integer and every comparison is array_equal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from map_conn_replay import ConnReplay, add_tables, apart, table_of
from test_map_quality import mixture, same

HEXA, RECT = 3, 4
BUBBLE = 1
SLAB = 1 << 20
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


def equal(got, want):
    """two tables: the same pairs in the same order with the same counts, in the ABI's types"""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint64
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    word = got[0].astype(np.int64) << 32 | got[1].astype(np.int64)
    assert np.all(word[1:] > word[:-1]) and np.all(got[2] > 0)            # ascending by (b1, b2), no pair twice, no zero


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    P = C.c_void_p
    want = {
        "somhip_conn_create": (C.c_int, [P, C.POINTER(P)]),
        "somhip_conn_destroy": (None, [P]),
        "somhip_conn_clear": (C.c_int, [P]),
        "somhip_conn_size": (C.c_int, [P, _lib.c_i64_p, _lib.c_u64_p]),
        "somhip_conn_read": (C.c_int, [P, C.c_int64, C.c_int64, _lib.c_u32_p, _lib.c_u32_p, _lib.c_u64_p]),
        "somhip_map_connectivity": (C.c_int, [P, P, C.c_int64, C.c_int64, P, _lib.c_u32_p, _lib.c_double_p, C.c_float,
                                              C.POINTER(_lib.QualityTotals)]),
        "somhip_conn_timing": (C.c_int, [P, _lib.c_i64_p, _lib.c_double_p]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == sig, name
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert "typedef struct somhip_conn somhip_conn;" in hdr
    m = re.search(r"^#define SOMHIP_CONN_SLAB (\d+)$", hdr, flags=re.M)
    assert m and int(m.group(1)) == engine.CONN_SLAB == SLAB and SLAB % 4096 == 0
    assert "int  somhip_map_connectivity(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, somhip_conn *c," in hdr
    assert "int  somhip_conn_read(somhip_conn *c, int64_t first, int64_t n, uint32_t *b1, uint32_t *b2, uint64_t *count);" in hdr
    for name in ("Conn", "map_connectivity"):
        assert hasattr(engine, name), name
    for name in ("clear", "size", "read", "close"):
        assert hasattr(engine.Conn, name), name
    assert hasattr(engine.Engine, "conn_timing")
    # null handles are refused without a device, by name
    assert lib.somhip_conn_create(None, None) != 0 and lib.somhip_last_error().decode().startswith("somhip_conn_create: null")
    assert lib.somhip_conn_clear(None) != 0 and lib.somhip_last_error().decode().startswith("somhip_conn_clear: null")
    assert lib.somhip_conn_read(None, 0, 0, None, None, None) != 0
    assert lib.somhip_last_error().decode().startswith("somhip_conn_read: null")
    assert lib.somhip_map_connectivity(None, None, 0, 1, None, None, None, 0.0, None) != 0
    assert lib.somhip_last_error().decode() == "somhip_map_connectivity: null handle"
    n, ms = (C.c_int64 * 4)(), (C.c_double * 4)()
    assert lib.somhip_conn_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_conn_timing: null engine"
    lib.somhip_conn_destroy(None)


def test_somqual_help_names_the_flag():
    if not os.path.exists(os.path.join(BIN, "somqual")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    p = subprocess.run([os.path.join(BIN, "somqual"), "-help"], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "-conn file" in p.stdout and "-uout file" in p.stdout and "-buffer N" in p.stdout


def test_replay_against_a_brute_force_count(oracle):
    """a 3 x 2 map: the two nearest units of every sample by a full sort of float64 distances (data without ties), counted
    pair by pair in a dict"""
    rs = np.random.RandomState(3)
    codes = rs.standard_normal((6, 4)).astype(np.float32)
    x = rs.standard_normal((500, 4)).astype(np.float32)
    d = ((x[:, None, :].astype(np.float64) - codes[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    order = np.argsort(d, axis=1, kind="stable")
    srt = np.sort(d, axis=1)
    assert np.all(srt[:, 1] - srt[:, 0] > 1e-4) and np.all(srt[:, 2] - srt[:, 1] > 1e-4)     # float32 sums agree on the order
    brute = {}
    for s in range(500):
        key = (int(order[s, 0]), int(order[s, 1]))
        brute[key] = brute.get(key, 0) + 1
    rep = ConnReplay(oracle, codes, x)
    b1, b2, cnt = rep.table()
    assert sorted(brute) == list(zip(b1.tolist(), b2.tolist()))
    assert [brute[k] for k in sorted(brute)] == cnt.tolist() and int(cnt.sum()) == 500
    # a window that wraps, and tables added up
    w = rep.table(490, 30)
    rows = (490 + np.arange(30)) % 500
    want = {}
    for s in rows:
        key = (int(order[s, 0]), int(order[s, 1]))
        want[key] = want.get(key, 0) + 1
    assert sorted(want) == list(zip(w[0].tolist(), w[1].tolist())) and [want[k] for k in sorted(want)] == w[2].tolist()
    both = add_tables(6, rep.table(), w)
    assert int(both[2].sum()) == 530 and np.array_equal(both[0], b1) and np.array_equal(both[1], b2)
    # no second-best unit on a map of one unit
    one = table_of(np.zeros(5, dtype=np.int64), np.full(5, -1, dtype=np.int64), 1)
    assert all(len(a) == 0 for a in one)


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


def run(E, eng, cb, ds, first=0, count=None, conn=None):
    """the table after one call on an empty table (or on `conn`)"""
    own = conn is None
    conn = E.Conn(eng) if own else conn
    assert E.map_connectivity(cb, ds, conn, first, count) is None
    out = conn.read()
    pairs, samples = conn.size()
    assert pairs == len(out[0]) and samples == int(out[2].sum())
    if own:
        conn.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,dim", [(1, 1, HEXA, 3), (2, 1, RECT, 3), (1, 2, HEXA, 3), (5, 4, HEXA, 3), (5, 4, RECT, 3),
                                                 (13, 5, HEXA, 5), (16, 16, HEXA, 3), (16, 16, RECT, 3), (1030, 1, HEXA, 3)])
def test_map_shapes(E, eng, oracle, xdim, ydim, topol, dim):
    """1 unit (no pair), 2 units (one bit per unit), small maps of both lattices, 16 x 16 in 8x8-patch storage (the pairs
    are unit indices y * xdim + x all the same), more than 1024 units in a row"""
    units = xdim * ydim
    x, codes = mixture(200 + units, 700, dim, xdim, ydim)
    cb = E.Codebook(eng, codes, topol, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x)
    want = ConnReplay(oracle, codes, x).table()
    got = run(E, eng, cb, ds)
    equal(got, want)
    assert int(got[2].sum()) == (700 if units > 1 else 0)
    if units == 1:
        assert len(got[0]) == 0
    if units == 2:
        assert set(zip(got[0].tolist(), got[1].tolist())) <= {(0, 1), (1, 0)}
    cb.close(); ds.close()


@pytest.mark.gpu
def test_words_wider_than_32_bits(E, oracle):
    """260 x 260 units of dim 2: a unit takes 17 bits, a pair 34.  The top-2 search takes the map; the engine is put in the
    direct scan mode so that the test is about the width of the words and not about a pre-filter at dim 2.  1500 samples
    give more pairs than the table's first 1024 entries, in one merge and in two."""
    xdim = ydim = 260
    x, codes = mixture(77, 1500, 2, xdim, ydim, noise=0.05)
    eng = E.Engine(0)
    eng.set_scan_mode("direct")
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, xdim, ydim)
    ds = E.Dataset(eng, x)
    rep = ConnReplay(oracle, codes, x)
    want = rep.table()
    assert int(want[0].max()) >= 1 << 15 and len(want[0]) > 1024 and len(rep.table(0, 600)[0]) <= 1024
    equal(run(E, eng, cb, ds), want)
    conn = E.Conn(eng)
    equal(run(E, eng, cb, ds, 0, 600, conn), rep.table(0, 600))
    equal(run(E, eng, cb, ds, 600, 900, conn), want)                     # the table outgrows its first buffers
    eng.close()


@pytest.fixture(scope="module")
def small(E, eng, oracle):
    """a 5 x 4 map of dim 3 over 3000 rows: a slab of samples wraps the data some 350 times"""
    x, codes = mixture(9, 3000, 3, 5, 4)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 5, 4)
    ds = E.Dataset(eng, x)
    yield cb, ds, ConnReplay(oracle, codes, x)
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("first,count", [(0, 1), (0, 4095), (0, 4096), (0, 4097), (0, SLAB - 1), (0, SLAB), (0, SLAB + 1),
                                         (0, 2 * SLAB + 1), (2990, 4097), (2990, SLAB + 1)])
def test_counts(E, eng, small, first, count):
    """a sample, a chunk less one, whole and one more; a slab less one, whole, one more, two slabs and one; from row 0 and
    from a row near the data's end"""
    cb, ds, rep = small
    got = run(E, eng, cb, ds, first, count)
    equal(got, rep.table(first, count))
    assert int(got[2].sum()) == count and int(got[2].max()) > (65535 if count >= SLAB - 1 else 0)


@pytest.fixture(scope="module")
def chunked(E, eng, oracle):
    """a 13 x 5 map of dim 5 over 6000 rows (test_map_quality's)"""
    x, codes = mixture(7, 6000, 5, 13, 5)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    ds = E.Dataset(eng, x)
    yield cb, ds, ConnReplay(oracle, codes, x), codes
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 4096, 5000])
def test_a_run_cut_in_two_gives_the_table_of_the_whole(E, eng, chunked, cut):
    cb, ds, rep, _ = chunked
    first, count = 5990, 8193
    want = rep.table(first, count)
    equal(run(E, eng, cb, ds, first, count), want)
    conn = E.Conn(eng)
    equal(run(E, eng, cb, ds, first, cut, conn), rep.table(first, cut))
    equal(run(E, eng, cb, ds, first + cut, count - cut, conn), want)
    conn.close()


@pytest.mark.gpu
def test_tables_accumulate_and_clear(E, eng, oracle, chunked):
    """a second data set behind the first; merges whose runs the table knows all, knows none of, and knows in part; clear"""
    cb, ds, rep, codes = chunked
    units = 65
    x2, _ = mixture(8, 900, 5, 13, 5)
    ds2 = E.Dataset(eng, x2)
    rep2 = ConnReplay(oracle, codes, x2)
    conn = E.Conn(eng)
    t1, t2 = rep.table(), rep2.table()
    equal(run(E, eng, cb, ds, conn=conn), t1)
    both = add_tables(units, t1, t2)
    known = set(zip(t1[0].tolist(), t1[1].tolist()))
    new = set(zip(t2[0].tolist(), t2[1].tolist())) - known
    assert new and len(new) < len(t2[0])                                 # interleaved: some runs are known, some are new
    equal(run(E, eng, cb, ds2, conn=conn), both)
    equal(run(E, eng, cb, ds2, conn=conn), add_tables(units, both, t2))  # every run is known: the counts grow, no pair is new
    conn.clear()
    assert conn.size() == (0, 0) and all(len(a) == 0 for a in conn.read())
    # every run is new: the rows whose best unit is in the lower half of the map, then the others
    low = rep.b1 < units // 2
    xa, xb = ds.rows(0, 6000)[low], ds.rows(0, 6000)[~low]
    dsa, dsb = E.Dataset(eng, xa), E.Dataset(eng, xb)
    ta = table_of(rep.b1[low], rep.b2[low], units)
    assert len(ta[0]) and len(ta[0]) < len(t1[0])
    equal(run(E, eng, cb, dsb, conn=conn), table_of(rep.b1[~low], rep.b2[~low], units))
    equal(run(E, eng, cb, dsa, conn=conn), t1)                           # the new runs all go in front of the table's
    # a cleared table takes a codebook of another size
    conn.clear()
    xs, cs = mixture(3, 50, 5, 3, 2)
    cbs = E.Codebook(eng, cs, RECT, BUBBLE, 3, 2)
    equal(run(E, eng, cbs, ds, 0, 500, conn), ConnReplay(oracle, cs, ds.rows(0, 500)).table())
    for h in (conn, ds2, dsa, dsb, cbs):
        h.close()


@pytest.mark.gpu
def test_every_sample_on_one_pair(E, eng, small):
    """one row, 3000 times over, taken 300 000 times: one entry, its count past 16 and 17 bits"""
    cb, ds, rep = small
    row = ds.rows(5, 1)
    one = E.Dataset(eng, np.repeat(row, 3000, axis=0))
    got = run(E, eng, cb, one, 7, 300000)
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ([int(rep.b1[5])], [int(rep.b2[5])], [300000])
    one.close()


@pytest.mark.gpu
def test_ties_follow_the_first_rule(E, eng, oracle):
    """integer data on a 6 x 5 map with equal rows (test_map_quality's case): b2 is the lowest index among equal distances,
    where find_winner_knn's order would give other pairs"""
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 4, size=(30, 3)).astype(np.float32)
    codes[8] = codes[7]; codes[20] = codes[3]; codes[12] = codes[11]; codes[25] = codes[11]
    x = rs.randint(0, 4, size=(600, 3)).astype(np.float32)
    x[0] = codes[14]; x[1] = codes[7]; x[2] = codes[3]; x[3] = codes[11]
    rep = ConnReplay(oracle, codes, x)
    knn = oracle.winners(codes, x, 2, True)[0]
    other = table_of(knn[:, 0].astype(np.int64), knn[:, 1].astype(np.int64), 30)
    want = rep.table()
    assert not (len(other[0]) == len(want[0]) and all(np.array_equal(a, b) for a, b in zip(other, want)))
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 6, 5)
    ds = E.Dataset(eng, x)
    equal(run(E, eng, cb, ds), want)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_masked_samples(E, eng, oracle):
    """data with missing components, rows with nothing left at the first and last position of both chunks of a run of
    4100 samples: they have no pair"""
    rs = np.random.RandomState(5)
    x, codes = mixture(21, 4100, 5, 13, 5)
    mask = (rs.uniform(size=x.shape) < 0.2).astype(np.uint8)
    empty = [0, 4095, 4096, 4099, 17, 2048, 2049]
    mask[empty] = 1
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    ds = E.Dataset(eng, x, mask=mask)
    rep = ConnReplay(oracle, codes, x, mask)
    n_empty = int(mask.all(axis=1).sum())
    got = run(E, eng, cb, ds)
    equal(got, rep.table())
    assert int(got[2].sum()) == 4100 - n_empty
    equal(run(E, eng, cb, ds, 4090, 20), rep.table(4090, 20))            # wraps over rows 4095, 4096, 4099 and 0
    assert all(len(a) == 0 for a in run(E, eng, cb, ds, 4095, 2))        # nothing but empty rows
    cb.close(); ds.close()


@pytest.mark.gpu
def test_a_codebook_without_a_lattice(E, eng, oracle):
    """the pairs alone need no lattice: an LVQ codebook (the edges competitive Hebbian learning draws)"""
    x, codes = mixture(12, 800, 4, 9, 1)
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, x)
    equal(run(E, eng, cb, ds), ConnReplay(oracle, codes, x).table())
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("topol", [HEXA, RECT])
def test_identities_and_the_fused_call(E, eng, chunked, topol):
    """the counts add up to topo_defined and, over the pairs further apart than 1, to topo_errors; the fused call leaves
    map_quality's bits and the pairs-only call's table, in one call and cut in two"""
    _, ds, rep, codes = chunked
    cb = E.Codebook(eng, codes, topol, BUBBLE, 13, 5)
    first, count = 5990, 8193
    quality = E.map_quality(cb, ds, first, count)
    table = run(E, eng, cb, ds, first, count)
    far = apart(topol, 13, table[0], table[1])
    assert far.any() and not far.all()
    assert int(table[2].sum()) == quality[0]["topo_defined"]
    assert int(table[2][far].sum()) == quality[0]["topo_errors"] > 0
    conn = E.Conn(eng)
    fused = E.map_connectivity(cb, ds, conn, first, count, quality=True)
    same(fused, quality)
    equal(conn.read(), table)
    conn.clear()
    t1, h, q = E.map_connectivity(cb, ds, conn, first, 5000, quality=True)
    t2, h, q = E.map_connectivity(cb, ds, conn, first + 5000, count - 5000, quality=True, hits=h, qsum=q, qerror=t1["qerror"])
    for k in ("searched", "topo_defined", "topo_errors"):
        t2[k] += t1[k]
    same((t2, h, q), quality)
    equal(conn.read(), table)
    # the totals alone (null hits and qsum), as somhip_map_quality allows
    from som_lvq_pak_amd import _lib
    conn.clear()
    tot = _lib.QualityTotals()
    assert eng.lib.somhip_map_connectivity(cb.h, ds.h, first, count, conn.h, None, None, 0.0, C.byref(tot)) == 0
    assert (tot.searched, tot.topo_defined, tot.topo_errors) == tuple(quality[0][k] for k in ("searched", "topo_defined", "topo_errors"))
    assert np.float32(tot.qerror).view(np.uint32) == quality[0]["qerror"].view(np.uint32)
    equal(conn.read(), table)
    conn.close(); cb.close()


@pytest.mark.gpu
def test_windowed_reads(E, eng, chunked):
    cb, ds, rep, _ = chunked
    conn = E.Conn(eng)
    want = run(E, eng, cb, ds, conn=conn)
    pairs = len(want[0])
    assert pairs > 40
    for first, n in ((0, 1), (0, pairs), (7, 30), (pairs - 1, 1), (pairs, 0), (3, 0)):
        got = conn.read(first, n)
        assert all(np.array_equal(g, w[first:first + n]) for g, w in zip(got, want))
    # each array may be null
    cnt = np.zeros(5, dtype=np.uint64)
    from som_lvq_pak_amd import _lib
    assert eng.lib.somhip_conn_read(conn.h, 2, 5, None, None, cnt.ctypes.data_as(_lib.c_u64_p)) == 0
    assert np.array_equal(cnt, want[2][2:7])
    b2 = np.zeros(5, dtype=np.uint32)
    assert eng.lib.somhip_conn_read(conn.h, 2, 5, None, b2.ctypes.data_as(_lib.c_u32_p), None) == 0
    assert np.array_equal(b2, want[1][2:7])
    for first, n in ((-1, 1), (0, pairs + 1), (pairs, 1), (pairs + 1, 0), (0, -1)):
        assert eng.lib.somhip_conn_read(conn.h, first, n, None, None, cnt.ctypes.data_as(_lib.c_u64_p)) != 0
        msg = eng.lib.somhip_last_error().decode()
        assert msg.startswith("somhip_conn_read: ") and "outside" in msg, msg
    conn.close()


@pytest.mark.gpu
def test_refusals_leave_the_table_alone(E, eng):
    from som_lvq_pak_amd import _lib
    lib = eng.lib
    x, codes = mixture(51, 40, 4, 4, 3)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 4, 3)
    ds = E.Dataset(eng, x)
    conn = E.Conn(eng)
    before = run(E, eng, cb, ds, conn=conn)
    assert len(before[0]) > 0
    tot = _lib.QualityTotals()
    hits = np.zeros(12, dtype=np.uint32)

    def refused(cbh, dsh, first, count, ch, what, out=None, h=None):
        assert lib.somhip_map_connectivity(cbh, dsh, first, count, ch, h, None, 0.0, out) != 0
        msg = lib.somhip_last_error().decode()
        assert msg.startswith("somhip_map_connectivity: ") and what in msg, msg
        got = conn.read()
        assert all(np.array_equal(g, b) for g, b in zip(got, before)) and conn.size() == (len(before[0]), 40)

    refused(None, ds.h, 0, 1, conn.h, "null handle")
    refused(cb.h, None, 0, 1, conn.h, "null handle")
    refused(cb.h, ds.h, 0, 1, None, "null handle")
    refused(cb.h, ds.h, 0, 1, conn.h, "null output", h=hits.ctypes.data_as(_lib.c_u32_p))
    other = E.Engine(0)
    ds_other, conn_other = E.Dataset(other, x), E.Conn(other)
    refused(cb.h, ds_other.h, 0, 1, conn.h, "different engines")
    refused(cb.h, ds.h, 0, 1, conn_other.h, "different engines")
    # a destroyed engine: the table's handle stays valid for its destroy, every other call on it is refused by name
    raw = C.c_void_p()
    assert lib.somhip_conn_create(other.h, C.byref(raw)) == 0
    ds_other.close(); conn_other.close(); other.close()
    refused(cb.h, ds.h, 0, 1, raw, "destroyed")
    for call, args in (("somhip_conn_clear", ()), ("somhip_conn_size", (C.byref(C.c_int64()), None)),
                       ("somhip_conn_read", (0, 0, None, None, None))):
        assert getattr(lib, call)(raw, *args) != 0
        msg = lib.somhip_last_error().decode()
        assert msg.startswith(call + ": ") and "destroyed" in msg, msg
    lib.somhip_conn_destroy(raw)
    ds3 = E.Dataset(eng, x[:, :3].copy())
    refused(cb.h, ds3.h, 0, 1, conn.h, "dimension")
    ds3.close()
    shard = E.Codebook(eng, codes[4:8], HEXA, BUBBLE, 4, 3, row_offset=4, n_global=12)
    refused(shard.h, ds.h, 0, 1, conn.h, "shard")
    shard.close()
    refused(cb.h, ds.h, -1, 1, conn.h, "first row")
    refused(cb.h, ds.h, 0, 1 << 32, conn.h, "count")
    six = E.Codebook(eng, codes[:6], RECT, BUBBLE, 3, 2)
    refused(six.h, ds.h, 0, 1, conn.h, "12 units")
    six.close()
    # with the totals asked for, somhip_map_quality's refusal of a codebook without a lattice; without them it is taken
    plain = E.Codebook(eng, codes)
    refused(plain.h, ds.h, 0, 1, conn.h, "lattice", out=C.byref(tot))
    plain.close()
    # count <= 0: success, nothing changes; with the totals, they are zero and the chain is where it was
    for count in (0, -3):
        assert lib.somhip_map_connectivity(cb.h, ds.h, 0, count, conn.h, None, None, 0.0, None) == 0
        tot.searched = tot.topo_defined = tot.topo_errors = 9
        assert lib.somhip_map_connectivity(cb.h, ds.h, 0, count, conn.h, None, None, 2.5, C.byref(tot)) == 0
        assert (tot.searched, tot.topo_defined, tot.topo_errors, tot.qerror) == (0, 0, 0, 2.5)
        assert all(np.array_equal(g, b) for g, b in zip(conn.read(), before))
    for h in (conn, cb, ds):
        h.close()


@pytest.mark.gpu
def test_timed_launches(E, eng, small):
    """the key pass once per chunk; per slab one sort and three timed scopes each for the runs and the merge; map_quality
    still launches its two kernels per chunk and none of these"""
    cb, ds, rep = small
    eng.timing(True)
    eng.timing_reset()
    E.map_quality(cb, ds, 0, 8193)
    assert [v[0] for v in eng.conn_timing().values()] == [0, 0, 0, 0]
    tm = eng.map_quality_timing()
    assert tm["k_quality_pairs"][0] == 3 and tm["k_quality_units"][0] == 3
    conn = E.Conn(eng)
    eng.timing_reset()
    E.map_connectivity(cb, ds, conn, 0, 8193)
    tm = eng.conn_timing()
    assert list(tm) == ["k_conn_keys", "sort", "runs", "merge"]
    assert [v[0] for v in tm.values()] == [3, 1, 3, 3] and all(v[1] > 0 for v in tm.values())
    assert [v[0] for v in eng.map_quality_timing().values()] == [0, 0]
    eng.timing_reset()
    conn.clear()
    E.map_connectivity(cb, ds, conn, 0, SLAB + 1, quality=True)
    chunks = SLAB // 4096 + 1
    assert [v[0] for v in eng.conn_timing().values()] == [chunks, 2, 6, 6]
    assert [v[0] for v in eng.map_quality_timing().values()] == [chunks, chunks]
    assert "k_conn_keys" not in eng.timing_table()                       # the published table is closed
    eng.timing(False)
    equal(conn.read(), rep.table(0, SLAB + 1))
    conn.close()
