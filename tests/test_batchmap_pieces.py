"""The batch map over data in pieces: somhip_batchmap_begin / _accumulate / _finish / _end / _state (engine.batchmap_*),
somhip_comm_broadcast and somhip_som_batchmap_ranks behind `bsom -gpus G`, and `bsom -buffer N`.

A per-unit sum is one chain of fp64 additions in data order, and a chain can be continued: a piece's sums start from what
the pieces before it left.  So every cut of the data -- into calls, buffers or the row blocks of ranks -- must leave the
bits of one call over the rows in that order.  Every comparison here is by bit pattern: no tolerance is involved."""
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
NEW = ("somhip_batchmap_begin", "somhip_batchmap_accumulate", "somhip_batchmap_finish", "somhip_batchmap_end",
       "somhip_batchmap_state", "somhip_comm_broadcast", "somhip_som_batchmap_ranks")
TOOL_TIMEOUT = 120


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("bsom", "datconv")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args, env=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=TOOL_TIMEOUT, env=dict(os.environ, **(env or {})))


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    S = _lib.SIGNATURES
    assert S["somhip_batchmap_begin"] == (C.c_int, [C.c_void_p])
    assert S["somhip_batchmap_accumulate"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int])
    assert S["somhip_batchmap_finish"] == (C.c_int, [C.c_void_p, C.c_float, C.c_int64, C.c_int64, _lib.c_float_p])
    assert S["somhip_batchmap_end"] == (C.c_int, [C.c_void_p])
    assert S["somhip_batchmap_state"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _lib.c_i64_p])
    assert S["somhip_comm_broadcast"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int])
    assert S["somhip_som_batchmap_ranks"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.BatchmapParams), C.c_void_p, _lib.c_float_p])
    for name in ("batchmap_begin", "batchmap_accumulate", "batchmap_finish", "batchmap_end", "batchmap_state"):
        assert callable(getattr(engine, name)), name


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for decl in ("int somhip_batchmap_begin(somhip_codebook *cb);",
                 "int somhip_batchmap_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror);",
                 "int somhip_batchmap_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count, float *qerror_out);",
                 "int somhip_batchmap_end(somhip_codebook *cb);",
                 "int somhip_batchmap_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);",
                 "int somhip_comm_broadcast(somhip_comm *c, void *dev_buf, int64_t bytes, int root);",
                 "int somhip_som_batchmap_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_batchmap_params *p, "
                 "somhip_comm *c, float *qerror_out );"):
        assert decl in hdr, decl


def test_null_handles_are_errors(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    assert lib.somhip_batchmap_begin(None) != 0
    assert lib.somhip_last_error().decode().startswith("somhip_batchmap_begin:")
    assert lib.somhip_batchmap_accumulate(None, None, 0, 1, 0) != 0
    assert lib.somhip_last_error().decode().startswith("somhip_batchmap_accumulate:")
    assert lib.somhip_batchmap_finish(None, 1.0, 0, 0, None) != 0
    assert lib.somhip_batchmap_end(None) != 0
    assert lib.somhip_comm_broadcast(None, None, 8, 0) != 0
    assert lib.somhip_last_error().decode().startswith("somhip_comm_broadcast:")


def test_bsom_help_and_refusals(tools, tmp_path):
    """-help names the two flags; -gpus with -buffer, -gpus < 1 and -buffer < 0 are refused before an engine is asked for,
    so they hold without a GPU and no file is written"""
    p = run("bsom", "-help")
    assert p.returncode == 0 and "-buffer" in p.stdout and "-gpus" in p.stdout
    cod = tmp_path / "m.cod"
    cod.write_text("2 hexa 2 2 bubble\n0 0\n1 0\n0 1\n1 1\n")
    dat = tmp_path / "d.dat"
    dat.write_text("2\n0.25 0.5\n0.75 0.5\n")
    out = tmp_path / "o.cod"
    for args, word in ((("-gpus", 2, "-buffer", 1), "-gpus together with -buffer"), (("-buffer", 5, "-gpus", 1), "-gpus together with -buffer"),
                       (("-gpus", 0), "-gpus 0"), (("-gpus", -2), "-gpus -2"), (("-buffer", -1), "-buffer -1")):
        p = run("bsom", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 2, "-radius", 2, *args)
        assert p.returncode == 1 and p.stderr.startswith("bsom: " + word), (args, p.stderr)
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


N = 9000
ONE_UNIT = (3000, 500)      # rows [3000, 3500) all win one unit
# map, lattice, neighbourhood, dim, radius: 5 x 3 is one partial row group, 9 x 8 two groups, 32 x 8 and 8 x 24 patch order;
# dims below, at and past the sums' 64 columns and the combine's 64; radius 1, 2.5 and beyond the map
CONFIGS = [(5, 3, HEXA, BUBBLE, 1, 1.0), (5, 3, RECT, GAUSSIAN, 17, 2.5), (9, 8, HEXA, BUBBLE, 64, 2.5), (9, 8, RECT, GAUSSIAN, 65, 100.0),
           (32, 8, HEXA, GAUSSIAN, 129, 1.0), (32, 8, RECT, BUBBLE, 17, 100.0), (8, 24, HEXA, BUBBLE, 65, 2.5), (8, 24, HEXA, GAUSSIAN, 64, 100.0),
           (8, 24, RECT, BUBBLE, 1, 1.0)]


def make(xdim, ydim, d, n=N, seed=None):
    """test_batchmap.py's generator, restated: a map laid out as a noisy sheet in the data space and data scattered around
    the sheet; rows ONE_UNIT lie next to one model vector"""
    rs = np.random.RandomState(1000 * xdim + 10 * ydim + d if seed is None else seed)
    units = xdim * ydim
    v = rs.standard_normal((2, d)).astype(np.float32)
    u = np.arange(units)
    pos = np.stack([u % xdim, u // xdim], axis=1).astype(np.float32)
    codes = (pos @ v + 0.4 * rs.standard_normal((units, d))).astype(np.float32)
    at = (rs.uniform(size=(n, 2)) * [xdim, ydim]).astype(np.float32)
    x = (at @ v + 0.5 * rs.standard_normal((n, d))).astype(np.float32)
    if n >= sum(ONE_UNIT):
        a, c = ONE_UNIT
        x[a:a + c] = codes[units // 2] + np.float32(1e-3) * rs.standard_normal((c, d)).astype(np.float32)
    return x, codes


def read_state(E, eng, cb):
    """(S float64[n, dim], counts float64[n], q float32, samples) from the state blob"""
    addr, nbytes = E.batchmap_state(cb)
    assert nbytes == 8 * cb.n * (cb.dim + 1) + 16
    raw = eng.copy_to_host(addr, nbytes)
    body = raw[:-16].view(np.float64).reshape(cb.n, cb.dim + 1)
    return body[:, :cb.dim].copy(), body[:, cb.dim].copy(), raw[-16:-12].view(np.float32)[0], int(raw[-8:].view(np.uint64)[0])


def cuts(E, eng, x):
    """name -> the pieces (dataset, first, n) whose rows, in order, are the rows of x; and the data sets to close"""
    n = len(x)
    whole = E.Dataset(eng, x)
    tail = E.Dataset(eng, x[5000:])                                      # a second Dataset object
    rolled = E.Dataset(eng, np.roll(x[5000:], 2500, axis=0))             # rows (2500 + s) % 4000 of it are x[5000 + s]

    def at(edges):
        edges = [0] + list(edges) + [n]
        return [(whole, a, b - a) for a, b in zip(edges[:-1], edges[1:])]

    seven = np.cumsum([1000, 1, 2500, 37, 4096, 300])                    # seven uneven pieces, one a single row; 1066 left
    a, c = ONE_UNIT
    out = {"row 1": at([1]), "4096": at([4096]), "4095": at([4095]), "4097": at([4097]), "seven": at(seven),
           "one unit": at([a, a + c]), "second data set": [(whole, 0, 5000), (tail, 0, n - 5000)],
           "wraps": [(whole, 0, 5000), (rolled, 2500, n - 5000)]}
    assert len(out["seven"]) == 7 and n - 5000 == 4000 and 2500 + 4000 > rolled.n
    return out, (whole, tail, rolled)


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", CONFIGS)
def test_pieces_equal_one_call(E, eng, xdim, ydim, topol, neigh, d, radius):
    """every cut of 9000 rows leaves the codebook, q, S and the counts of one som_batchmap epoch over them"""
    x, codes = make(xdim, ydim, d)
    pieces, sets = cuts(E, eng, x)
    whole = sets[0]
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    hits, S = E.batchmap_sums(ref, whole)
    a, c = ONE_UNIT
    one = E.batchmap_sums(ref, whole, a, c)[0]
    assert one.max() == c                                                # the piece's samples all win one unit
    q_ref = E.som_batchmap(ref, whole, 1, radius, count=1)[0]
    want = ref.download()
    assert not same(want, codes)
    r = E.batchmap_radius(radius, 1, 0)
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    for name, cut in pieces.items():
        cb.upload(codes)
        E.batchmap_begin(cb)
        s0, c0, q0, n0 = read_state(E, eng, cb)
        assert not bits(s0).any() and not bits(c0).any() and bits(np.float32(q0)) == 0 and n0 == 0      # all +0.0
        for ds, first, n in cut:
            E.batchmap_accumulate(cb, ds, first, n)
        s1, c1, q1, n1 = read_state(E, eng, cb)
        assert same(s1, S), name
        assert np.array_equal(c1, hits.astype(np.float64)), name
        assert n1 == N and bits(np.float32(q1)) == bits(np.float32(q_ref)), name
        q = E.batchmap_finish(cb, r)
        assert bits(np.float32(q)) == bits(np.float32(q_ref)), (name, q, q_ref)
        assert same(cb.download(), want), name
    E.batchmap_end(cb)
    for o in (cb, ref) + sets:
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", [CONFIGS[2], CONFIGS[4]])
def test_qerror_is_optional_per_piece(E, eng, xdim, ydim, topol, neigh, d, radius):
    """qerror=False: the same rows and sums, no q chain, no per-sample copy"""
    x, codes = make(xdim, ydim, d)
    ds = E.Dataset(eng, x)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.som_batchmap(ref, ds, 1, radius, qerror=False)
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 4097, qerror=False)
    E.batchmap_accumulate(cb, ds, 4097, N - 4097, qerror=False)
    assert read_state(E, eng, cb)[2:] == (0.0, N)
    assert E.batchmap_finish(cb, E.batchmap_radius(radius, 1, 0), qerror=False) is None
    assert same(cb.download(), ref.download())
    for o in (cb, ref, ds):
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", [CONFIGS[1], CONFIGS[3], CONFIGS[6]])
def test_hand_off_between_codebooks(E, eng, xdim, ydim, topol, neigh, d, radius):
    """A accumulates piece 1, its blob goes into B (same rows, its own state opened), B accumulates piece 2 and finishes: the
    one call.  Other engine calls between the pieces (a search, a one-call epoch on a third codebook) leave the state alone."""
    x, codes = make(xdim, ydim, d)
    ds = E.Dataset(eng, x)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    q_ref = E.som_batchmap(ref, ds, 1, radius, count=1)[0]
    A = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    B = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    other = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_begin(A)
    E.batchmap_accumulate(A, ds, 0, 4100)
    E.som_batchmap(other, ds, 2, radius)                                 # uses the engine's batch-map scratch
    E.batchmap_sums(other, ds, 5, 77)
    E.batchmap_begin(B)
    (a_addr, a_bytes), (b_addr, b_bytes) = E.batchmap_state(A), E.batchmap_state(B)
    assert a_bytes == b_bytes and a_addr != b_addr
    eng.copy_to_device(b_addr, eng.copy_to_host(a_addr, a_bytes))
    E.batchmap_accumulate(B, ds, 4100, N - 4100)
    q = E.batchmap_finish(B, E.batchmap_radius(radius, 1, 0))
    assert bits(np.float32(q)) == bits(np.float32(q_ref))
    assert same(B.download(), ref.download())
    assert same(A.download(), codes)                                     # A never finished
    for o in (A, B, other, ref, ds):
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", [CONFIGS[2], CONFIGS[3], CONFIGS[4], CONFIGS[6]])
def test_finish_by_group_ranges(E, eng, xdim, ydim, topol, neigh, d, radius):
    """finish over (0, 1) and then (1, ngroups - 1) equals finish over everything; after the first call the rows of the
    other groups still have their old bits"""
    x, codes = make(xdim, ydim, d)
    ds = E.Dataset(eng, x)
    ngroups = (xdim * ydim + 63) // 64
    assert ngroups >= 2
    r = E.batchmap_radius(radius, 1, 0)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.som_batchmap(ref, ds, 1, radius)
    want = ref.download()
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 10)
    E.batchmap_accumulate(cb, ds, 10, N - 10)
    q0 = E.batchmap_finish(cb, r, 0, 1)
    part = cb.download()
    changed = (bits(part) != bits(codes)).any(axis=1)
    assert changed.sum() > 0 and changed.sum() <= 64
    assert same(part[changed], want[changed]) and same(part[~changed], codes[~changed])
    # the rows of storage group 0: in patch order an 8 x 8 patch of the lattice, else the first 64 units
    if xdim % 8 == 0 and ydim % 8 == 0:
        u = np.arange(xdim * ydim)
        group0 = (u % xdim < 8) & (u // xdim < 8)
    else:
        group0 = np.arange(xdim * ydim) < 64
    assert not changed[~group0].any() and same(part[group0], want[group0])
    q1 = E.batchmap_finish(cb, r, 1, ngroups - 1)
    assert q0 == q1
    assert same(cb.download(), want)
    E.batchmap_finish(cb, r, ngroups, 0)                                  # an empty range at the end: legal, writes nothing
    assert same(cb.download(), want)
    # ... and does not count as a move: after begin and an empty finish, pieces are still taken
    cb.upload(codes)
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 10)
    E.batchmap_finish(cb, r, 0, 0)
    E.batchmap_accumulate(cb, ds, 10, N - 10)
    E.batchmap_finish(cb, r)
    assert same(cb.download(), want)
    for o in (cb, ref, ds):
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", [CONFIGS[1], CONFIGS[6], CONFIGS[7]])
def test_five_epochs_in_pieces(E, eng, xdim, ydim, topol, neigh, d, radius):
    """begin / pieces / finish five times = som_batchmap with 5 epochs, the per-epoch q included"""
    x, codes = make(xdim, ydim, d)
    ds = E.Dataset(eng, x)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    q_ref = E.som_batchmap(ref, ds, 5, radius)
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    for t in range(5):
        E.batchmap_begin(cb)
        for first in range(0, N, 2000 + 7 * t):
            E.batchmap_accumulate(cb, ds, first, min(2000 + 7 * t, N - first))
        q = E.batchmap_finish(cb, E.batchmap_radius(radius, 5, t))
        assert bits(np.float32(q)) == bits(np.float32(q_ref[t])), t
    E.batchmap_end(cb)
    assert same(cb.download(), ref.download())
    for o in (cb, ref, ds):
        o.close()


def device_free_bytes():
    """free device memory, as the HIP runtime the engine runs on reports it (hipMemGetInfo)"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng):
    x, codes = make(13, 5, 6, n=700)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    lvq = E.Codebook(eng, codes, E.TOPOL_LVQ)
    shard = E.Codebook(eng, codes[:26], HEXA, BUBBLE, 13, 5, row_offset=13, n_global=65)
    other = E.Dataset(eng, x[:, :5])
    ngroups = 2

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    # nothing is open yet
    refused(lambda: E.batchmap_accumulate(cb, ds), "somhip_batchmap_accumulate", "somhip_batchmap_begin")
    refused(lambda: E.batchmap_finish(cb, 2.0), "somhip_batchmap_finish", "somhip_batchmap_begin")
    refused(lambda: E.batchmap_state(cb), "somhip_batchmap_state", "somhip_batchmap_begin")
    refused(lambda: E.batchmap_begin(lvq), "somhip_batchmap_begin", "without a lattice")
    refused(lambda: E.batchmap_begin(shard), "somhip_batchmap_begin", "sharded")
    E.batchmap_end(cb)                                                   # nothing to free: fine

    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 300)
    before = eng.copy_to_host(*E.batchmap_state(cb))
    who = "somhip_batchmap_accumulate"
    refused(lambda: E.batchmap_accumulate(cb, masked), who, "masked components")
    refused(lambda: E.batchmap_accumulate(shard, ds), who, "sharded")
    refused(lambda: E.batchmap_accumulate(lvq, ds), who, "without a lattice")
    refused(lambda: E.batchmap_accumulate(cb, other), who, "dimension")
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, 0), who, "n 0")
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, -5), who, "n -5")
    refused(lambda: E.batchmap_accumulate(cb, ds, -1, 5), who, "first row")
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, 2 ** 32), who, "32-bit")
    free_before = device_free_bytes()
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, 2 ** 32 - 300), who, "32-bit")       # 300 taken: the total would be 2^32
    # ... refused before any room is made: the lists of 2^32 samples would be 64 GiB, and engine scratch never shrinks (half
    # of that as the line, so that another process's allocations on the same device in these microseconds do not decide)
    assert device_free_bytes() > free_before - (32 << 30)
    who = "somhip_batchmap_finish"
    refused(lambda: E.batchmap_finish(cb, -1.0), who, "radius")
    refused(lambda: E.batchmap_finish(cb, float("nan")), who, "radius")
    refused(lambda: E.batchmap_finish(cb, 2.0, -1, 1), who, "row groups")
    refused(lambda: E.batchmap_finish(cb, 2.0, 0, ngroups + 1), who, "row groups")
    refused(lambda: E.batchmap_finish(cb, 2.0, ngroups, 1), who, "row groups")
    refused(lambda: E.batchmap_finish(cb, 2.0, 1, -1), who, "row groups")
    assert np.array_equal(eng.copy_to_host(*E.batchmap_state(cb)), before)
    for c, rows in ((cb, codes), (lvq, codes), (shard, codes[:26])):
        assert same(c.download(), rows)

    # the refused calls changed nothing: the accumulation goes on and ends as the one call
    ref = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    q_ref = E.som_batchmap(ref, ds, 1, 2.0)[0]
    E.batchmap_accumulate(cb, ds, 300, 400)
    q = E.batchmap_finish(cb, 2.0)
    assert bits(np.float32(q)) == bits(np.float32(q_ref)) and same(cb.download(), ref.download())
    # the codebook has moved
    refused(lambda: E.batchmap_accumulate(cb, ds, 0, 10), "somhip_batchmap_accumulate", "the codebook has moved")
    assert same(cb.download(), ref.download())
    E.batchmap_begin(cb)                                                 # ... until the next begin
    E.batchmap_accumulate(cb, ds, 0, 10)

    # a writer of the rows closes the state: upload, som_train, som_batchmap
    for writer in (lambda: cb.upload(codes), lambda: E.som_train(cb, ds, 20, 0.05, 2.0, trace=False), lambda: E.som_batchmap(cb, ds, 1, 2.0)):
        E.batchmap_begin(cb)
        E.batchmap_accumulate(cb, ds, 0, 10)
        writer()
        rows = cb.download()
        refused(lambda: E.batchmap_accumulate(cb, ds, 10, 10), "somhip_batchmap_accumulate", "somhip_batchmap_begin")
        refused(lambda: E.batchmap_finish(cb, 2.0), "somhip_batchmap_finish", "somhip_batchmap_begin")
        assert same(cb.download(), rows)
    E.batchmap_begin(cb)
    E.batchmap_end(cb)
    refused(lambda: E.batchmap_accumulate(cb, ds), "somhip_batchmap_accumulate", "somhip_batchmap_begin")
    for o in (cb, ref, lvq, shard, ds, masked, other):
        o.close()


@pytest.mark.gpu
def test_destroying_the_codebook_frees_an_open_state(E, eng):
    x, codes = make(9, 8, 17, n=700)
    ds = E.Dataset(eng, x)
    for _ in range(3):
        cb = E.Codebook(eng, codes, HEXA, BUBBLE, 9, 8)
        E.batchmap_begin(cb)
        E.batchmap_accumulate(cb, ds)
        cb.close()
    ds.close()


@pytest.mark.gpu
def test_timing_counts_under_the_three_ids(E, eng):
    """the new launches are counted under the three existing ids; the published kernel table has no new name"""
    x, codes = make(13, 5, 6, n=700)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, GAUSSIAN, 13, 5)
    eng.timing(True)
    eng.timing_reset()
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 300, qerror=False)
    E.batchmap_accumulate(cb, ds, 300, 400, qerror=False)
    E.batchmap_finish(cb, 2.0, 0, 1)
    E.batchmap_finish(cb, 2.0, 1, 1)
    t = eng.batchmap_timing()
    names = set(eng.timing_table())
    eng.timing(False)
    assert t["k_batchmap_sums"][0] == 2 and t["k_batchmap_combine"][0] == 4 and t["group"][0] == 6   # (table + combine; winners, scan, sort)
    assert all(ms > 0 for _, ms in t.values())
    assert not [n for n in names if "batchmap" in n]
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", CONFIGS)
def test_parent_paths_unchanged(E, eng, oracle, xdim, ydim, topol, neigh, d, radius):
    """som_batchmap and batchmap_sums keep their bits: the sums against the CPU replay's data-order chains, the epoch
    against a second run (and with an accumulation open on another codebook in between)"""
    x, codes = make(xdim, ydim, d, n=1500)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    win, _ = R.winners(oracle, codes, x)
    for first, n in ((0, 1500), (1499, 1), (700, 1500)):
        hits, S = E.batchmap_sums(cb, ds, first, n)
        wh, ws = R.sums(win, x, codes.shape[0], first, n)
        assert np.array_equal(hits, wh) and same(S, ws), (first, n)
    q1 = E.som_batchmap(cb, ds, 3, radius)
    rows1 = cb.download()
    busy = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    E.batchmap_begin(busy)
    E.batchmap_accumulate(busy, ds, 0, 100)
    cb.upload(codes)
    q2 = E.som_batchmap(cb, ds, 3, radius)
    assert same(q1, q2) and same(cb.download(), rows1)
    for o in (cb, busy, ds):
        o.close()


# ---- the rank loop inside one process: a communicator of one rank over the socket transport
@pytest.fixture()
def comm1(eng):
    h = C.c_void_p()
    assert eng.lib.somhip_comm_create_sockets(eng.h, 0, 1, None, C.byref(h)) == 0
    yield h
    eng.lib.somhip_comm_destroy(h)


def ranks(E, cb, ds, comm, epochs, radius, first=0, n=None, start_epoch=0, count=None):
    from som_lvq_pak_amd import _lib
    count = epochs - start_epoch if count is None else count
    p = _lib.BatchmapParams(epochs, radius, start_epoch, count, first, (ds.n if ds is not None else 0) if n is None else n)
    q = np.zeros(max(count, 0), dtype=np.float32)
    _lib.check(cb.e.lib.somhip_som_batchmap_ranks(cb.h, ds.h if ds is not None else None, C.byref(p), comm, q.ctypes.data_as(_lib.c_float_p)))
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,topol,neigh,d,radius", [CONFIGS[1], CONFIGS[2], CONFIGS[4]])
def test_one_rank_equals_one_call(E, eng, comm1, xdim, ydim, topol, neigh, d, radius):
    """somhip_som_batchmap_ranks with one rank is somhip_som_batchmap; it leaves no state open behind it; an empty block
    (n == 0, no data set) moves no row"""
    x, codes = make(xdim, ydim, d, n=1500)
    ds = E.Dataset(eng, x)
    ref = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    q_ref = E.som_batchmap(ref, ds, 3, radius, first=700, n=1500)
    cb = E.Codebook(eng, codes, topol, neigh, xdim, ydim)
    q = ranks(E, cb, ds, comm1, 3, radius, first=700, n=1500)
    assert same(q, q_ref) and same(cb.download(), ref.download())
    with pytest.raises(Exception, match="somhip_batchmap_begin"):
        E.batchmap_finish(cb, 2.0)
    rows = cb.download()
    q = ranks(E, cb, None, comm1, 2, radius, n=0)
    assert not bits(q).any() and same(cb.download(), rows)
    for o in (cb, ref, ds):
        o.close()


@pytest.mark.gpu
def test_rank_loop_and_broadcast_refusals(E, eng, comm1):
    x, codes = make(13, 5, 6, n=700)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    lvq = E.Codebook(eng, codes, E.TOPOL_LVQ)
    other = E.Dataset(eng, x[:, :5])
    eng2 = E.Engine(0)
    far = E.Codebook(eng2, codes, HEXA, BUBBLE, 13, 5)
    far_ds = E.Dataset(eng2, x)

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    who = "somhip_som_batchmap_ranks"
    refused(lambda: ranks(E, cb, masked, comm1, 3, 2.0), who, "masked components")
    refused(lambda: ranks(E, lvq, ds, comm1, 3, 2.0), who, "without a lattice")
    refused(lambda: ranks(E, cb, other, comm1, 3, 2.0), who, "dimension")
    refused(lambda: ranks(E, far, far_ds, comm1, 3, 2.0), who, "different engines")
    refused(lambda: ranks(E, cb, ds, comm1, 3, 2.0, n=-5), who, "n -5")
    refused(lambda: ranks(E, cb, ds, comm1, 3, 2.0, n=2 ** 32), who, "32-bit")
    refused(lambda: ranks(E, cb, ds, comm1, 3, 2.0, first=-1), who, "first row")
    refused(lambda: ranks(E, cb, ds, comm1, 0, 2.0, count=0), who, "epochs 0")
    refused(lambda: ranks(E, cb, ds, comm1, 3, 0.5), who, "radius")
    refused(lambda: ranks(E, cb, ds, comm1, 3, 2.0, start_epoch=2, count=2), who, "outside")
    assert same(cb.download(), codes) and same(far.download(), codes)
    # the broadcast on a live communicator: a root outside the ranks is refused, the one rank's own is nothing to do
    from som_lvq_pak_amd import _lib
    buf = eng.device_alloc(64)
    eng.copy_to_device(buf.value, np.arange(16, dtype=np.float32))
    for root in (1, -1):
        assert eng.lib.somhip_comm_broadcast(comm1, buf, 64, root) != 0
        assert eng.lib.somhip_last_error().decode().startswith("somhip_comm_broadcast: root %d" % root)
    assert eng.lib.somhip_comm_broadcast(comm1, buf, 64, 0) == 0
    assert np.array_equal(eng.copy_to_host(buf.value, 64).view(np.float32), np.arange(16, dtype=np.float32))
    eng.device_free(buf)
    for o in (cb, lvq, ds, masked, other):
        o.close()
    eng2.close()


# ---- the tool
def write_inputs(tmp_path, x, codes, topol, neigh, xdim, ydim):
    from som_lvq_pak_amd import textio
    dat, cod = tmp_path / "d.dat", tmp_path / "m.cod"
    d = textio.Entries()
    d.dim, d.points = x.shape[1], x
    textio.write_entries(str(dat), d)
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = x.shape[1], topol, neigh, xdim, ydim, codes
    textio.write_entries(str(cod), m)
    return dat, cod


@pytest.fixture(scope="module")
def tool_runs(tools, tmp_path_factory):
    """the plain runs every flag is compared with: a text file of 700 rows on a 9 x 8 map, a gen: source of 9000 rows on a
    16 x 8 one; each (arguments, .cod bytes, -v lines)"""
    tmp = tmp_path_factory.mktemp("bsom_pieces")
    rs = np.random.RandomState(43)
    x = (np.round(rs.standard_normal((700, 5)) * 16) / 16).astype(np.float32)       # values that "%g" keeps
    codes = (np.round(rs.standard_normal((9 * 8, 5)) * 16) / 16).astype(np.float32)
    dat, cod = write_inputs(tmp, x, codes, HEXA, GAUSSIAN, 9, 8)
    gcodes = (np.round(rs.standard_normal((16 * 8, 6)) * 16) / 4).astype(np.float32)
    (tmp / "g").mkdir()
    _, gcod = write_inputs(tmp / "g", x[:2, :1].repeat(6, axis=1), gcodes, RECT, BUBBLE, 16, 8)
    two = tmp / "two.dat"
    two.write_text("5\n" + "\n".join(" ".join("%g" % v for v in row) for row in x[:2]) + "\n")
    runs = {"file": ["-cin", cod, "-din", dat, "-epochs", 3, "-radius", 3, "-v"],
            "gen": ["-cin", gcod, "-din", "gen:k=5,dim=6,n=9000,seed=11", "-epochs", 2, "-radius", 4, "-v"],
            "two": ["-cin", cod, "-din", two, "-epochs", 2, "-radius", 2, "-v"]}
    plain = {}
    for name, args in runs.items():
        out = tmp / (name + "_plain.cod")
        p = run("bsom", *args, "-cout", out)
        assert p.returncode == 0, p.stderr
        assert len(p.stdout.strip().split("\n")) == int(args[5])
        plain[name] = (args, out.read_bytes(), p.stdout)
    return tmp, plain


def same_run(tool_runs, name, extra, env=None):
    tmp, plain = tool_runs
    args, cod_bytes, lines = plain[name]
    out = tmp / ("%s_%s.cod" % (name, "_".join(str(a).strip("-") for a in extra) + ("_env" if env else "")))
    p = run("bsom", *args, "-cout", out, *extra, env=env)
    assert p.returncode == 0, (name, extra, p.stderr)
    assert out.read_bytes() == cod_bytes, (name, extra)
    got = p.stdout
    if (env or {}).get("SOMHIP_COMM") == "rccl":                         # librccl prints a banner of its own to stdout: not the tool's lines
        got = "".join(s for s in got.splitlines(True) if s.startswith("epoch "))
    assert got == lines, (name, extra)


@pytest.mark.gpu
@pytest.mark.parametrize("buffer", [1, 7, 4096, 8999, 100000])
def test_bsom_buffer_writes_the_plain_bytes(tool_runs, buffer):
    """-buffer 1 (every piece one row, generated in place from its own first row for the gen: source), 7, the search's chunk,
    one row short of the gen: source (a last piece of one row) and larger than either source"""
    same_run(tool_runs, "file", ["-buffer", buffer])
    same_run(tool_runs, "gen", ["-buffer", buffer])


@pytest.mark.gpu
def test_bsom_buffer_without_v(tool_runs):
    tmp, plain = tool_runs
    args, cod_bytes, _ = plain["file"]
    out = tmp / "file_quiet.cod"
    p = run("bsom", *args[:-1], "-cout", out, "-buffer", 100)
    assert p.returncode == 0 and p.stdout == "" and out.read_bytes() == cod_bytes


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [2, 3])
def test_bsom_gpus_writes_the_plain_bytes(tool_runs, gpus):
    """the ranks share the one GPU: the state and the tiles travel over the host sockets"""
    env = {"SOMHIP_COMM": "sockets"}
    same_run(tool_runs, "file", ["-gpus", gpus], env)
    same_run(tool_runs, "gen", ["-gpus", gpus], env)


@pytest.mark.gpu
def test_bsom_gpus_with_an_empty_rank(tool_runs):
    same_run(tool_runs, "two", ["-gpus", 3], {"SOMHIP_COMM": "sockets"})


@pytest.mark.gpu
def test_bsom_one_rank_through_rccl(tool_runs):
    """SOMHIP_COMM=rccl with one rank sends the loop through ncclBroadcast / ncclAllGather on the engine's stream"""
    same_run(tool_runs, "file", ["-gpus", 1], {"SOMHIP_COMM": "rccl"})     # (one run: opening the communicator is most of its time)


@pytest.mark.gpu
def test_bsom_two_ranks_through_rccl(E, tool_runs):
    from som_lvq_pak_amd import _lib
    count = C.c_int(0)
    assert _lib.load().somhip_device_count(C.byref(count)) == 0
    if count.value < 2:
        pytest.skip("one device: RCCL refuses ranks that share it")
    same_run(tool_runs, "file", ["-gpus", 2], {"SOMHIP_COMM": "rccl"})
    same_run(tool_runs, "gen", ["-gpus", 2], {"SOMHIP_COMM": "rccl"})
