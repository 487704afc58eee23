"""Batch GLVQ over data in pieces: somhip_glvq_begin / _accumulate / _finish / _end / _state (engine.glvq_*),
somhip_glvq_train_ranks behind `glvq -gpus G`, and `glvq -buffer N` (include/somhip_glvq_pieces.h).

The per-row sums of a GLVQ epoch are chains of fp64 additions in data order, and a chain can be continued: a piece's sums
start from what the pieces before it left.  So every cut of the data -- into calls, buffers or the row blocks of ranks --
must leave the bits of one call of somhip_glvq_train / engine.glvq_sums over the rows in that order.  Every comparison
here is by bit pattern: no tolerance is involved.  The one-call side is held to tests/glvq_replay.py with the identity.

The header has a file of its own, as include/somhip_rslvq.h has, so it is held here to what tests/test_build.py and
tests/test_prepared_state.py ask of somhip.h: every declaration exported and mirrored (_lib.GLVQ_PIECES_SIGNATURES), every
entry point that takes a codebook a writer or a reader of the tables below, checked against the prepared copies."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glvq_replay as R
import test_prepared_state as PS
from conftest import ROOT
from test_prepared_state import E, data, ds, eng  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
f32, f64 = np.float32, np.float64
HEXA, BUBBLE = 3, 1                                                      # include/somhip.h SOMHIP_TOPOL_HEXA, SOMHIP_NEIGH_BUBBLE
NEW = ("somhip_glvq_begin", "somhip_glvq_accumulate", "somhip_glvq_finish", "somhip_glvq_end", "somhip_glvq_state",
       "somhip_glvq_train_ranks")
TOOL_TIMEOUT = 120
CHUNK = 16384                                                            # GLVQ_CHUNK of host_proto.inc: samples of a class-wise scan launch
N = 16500
ALPHA = 30.0


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("glvq",)):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args, env=None):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=TOOL_TIMEOUT, env=dict(os.environ, **(env or {})))


def header():
    hdr = open(os.path.join(ROOT, "include", "somhip_glvq_pieces.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


# ------------------------------------------------------------------------------------------------ without a GPU
def test_somhip_h_includes_the_header():
    top = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r'^#include "somhip_glvq_pieces.h"$', top, flags=re.M)
    assert "somhip_glvq_begin" not in re.sub(r"/\*.*?\*/", "", top, flags=re.S)        # declared once, in its own header


def test_header_symbols_exported_and_mirrored(built):
    from som_lvq_pak_amd import _lib, engine
    declared = set(re.findall(r"\b(somhip_[a-z0-9_]+)\s*\(", header()))
    assert declared == set(NEW)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), "libsomhip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.GLVQ_PIECES_SIGNATURES[name][1], name
    assert declared == set(_lib.GLVQ_PIECES_SIGNATURES)
    assert not (set(_lib.GLVQ_PIECES_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.RSLVQ_SIGNATURES)))
    S = _lib.GLVQ_PIECES_SIGNATURES
    assert S["somhip_glvq_accumulate"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float])
    assert S["somhip_glvq_finish"] == (C.c_int, [C.c_void_p, C.c_float, _lib.c_double_p, _lib.c_i64_p, _lib.c_i64_p])
    assert S["somhip_glvq_state"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _lib.c_i64_p])
    assert S["somhip_glvq_train_ranks"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.GlvqParams), C.c_void_p, _lib.c_double_p,
                                                      _lib.c_i64_p])
    for name in ("glvq_begin", "glvq_accumulate", "glvq_finish", "glvq_end", "glvq_state", "glvq_train_ranks"):
        assert callable(getattr(engine, name)), name


def test_header_declares_the_entry_points():
    hdr = header()
    for decl in ("int somhip_glvq_begin(somhip_codebook *cb);",
                 "int somhip_glvq_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta);",
                 "int somhip_glvq_finish(somhip_codebook *cb, float alpha_t, double *cost_out, int64_t *correct_out, int64_t *samples_out);",
                 "int somhip_glvq_end(somhip_codebook *cb);",
                 "int somhip_glvq_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);",
                 "int somhip_glvq_train_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_glvq_params *p, somhip_comm *c, "
                 "double *cost_out , int64_t *correct_out );"):
        assert decl in hdr, decl


def test_null_handles_are_refused_by_name(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    addr, nbytes = C.c_void_p(), C.c_int64(0)
    p = _lib.GlvqParams(1, 0, 1, 0, 5, 1.0, 0.0)
    for name, call in (("somhip_glvq_begin", lambda: lib.somhip_glvq_begin(None)),
                       ("somhip_glvq_accumulate", lambda: lib.somhip_glvq_accumulate(None, None, 0, 1, 0.0)),
                       ("somhip_glvq_finish", lambda: lib.somhip_glvq_finish(None, 1.0, None, None, None)),
                       ("somhip_glvq_end", lambda: lib.somhip_glvq_end(None)),
                       ("somhip_glvq_state", lambda: lib.somhip_glvq_state(None, C.byref(addr), C.byref(nbytes))),
                       ("somhip_glvq_train_ranks", lambda: lib.somhip_glvq_train_ranks(None, None, C.byref(p), None, None, None))):
        assert call() != 0, name
        msg = lib.somhip_last_error().decode()
        assert msg.startswith(name + ": null"), msg


def test_glvq_help_and_refusals(tools, tmp_path):
    """-help names the two options; -gpus with -buffer, -gpus < 1 and a -buffer below 1 are refused before an engine is asked
    for, so they hold without a GPU and no file is written"""
    p = run("glvq", "-help")
    assert p.returncode == 0 and "-buffer" in p.stdout and "-gpus" in p.stdout
    cod, dat, out = tmp_path / "c.cod", tmp_path / "d.dat", tmp_path / "o.cod"
    cod.write_text("2\n0 0 a\n1 1 b\n")
    dat.write_text("2\n0.25 0.5 a\n0.75 0.5 b\n")
    for args, word in ((("-gpus", 2, "-buffer", 1), "-gpus together with -buffer"), (("-buffer", 5, "-gpus", 1), "-gpus together with -buffer"),
                       (("-gpus", 0), "-gpus 0"), (("-gpus", -2), "-gpus -2"), (("-buffer", 0), "-buffer 0"), (("-buffer", -1), "-buffer -1")):
        p = run("glvq", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 2, "-alpha", 1, *args)
        assert p.returncode == 1 and p.stderr.startswith("glvq: " + word), (args, p.stderr)
        assert not out.exists()


def w_glvq_pieces(E, eng, cb, ds, data):
    E.glvq_begin(cb)
    E.glvq_accumulate(cb, ds, 0, 1000)
    E.glvq_accumulate(cb, ds, 1000, PS.M - 1000)
    E.glvq_finish(cb, 50.0)
    E.glvq_end(cb)


def w_glvq_ranks(E, eng, cb, ds, data):
    comm = C.c_void_p()
    E.check(eng.lib.somhip_comm_create_sockets(eng.h, 0, 1, None, C.byref(comm)))
    try:
        E.glvq_train_ranks(cb, ds, comm, 2, 50.0, n=PS.M, stats=False)
    finally:
        eng.lib.somhip_comm_destroy(comm)


def r_glvq_open(E, eng, cb, ds):
    E.glvq_begin(cb)
    E.glvq_accumulate(cb, ds, 0, PS.M)
    E.glvq_state(cb)
    E.glvq_end(cb)


# id -> (entry points that write rows, the writer, the flags (prep_valid, rowmajor_valid) it must leave)
WRITERS = {
    "glvq_pieces": (("somhip_glvq_finish",), w_glvq_pieces, (0, 0)),
    "glvq_train_ranks": (("somhip_glvq_train_ranks",), w_glvq_ranks, (0, 0)),
}
# id -> (entry points, the reader)
READERS = {
    "glvq_begin_accumulate": (("somhip_glvq_begin", "somhip_glvq_accumulate", "somhip_glvq_state", "somhip_glvq_end"), r_glvq_open),
}


def test_every_writer_has_a_case():
    """every entry point of the header that takes a codebook it may write to is in the writers' table or the readers'"""
    takes = set()
    for name, args in re.findall(r"\b(somhip_[a-z0-9_]+) ?\(([^;{}]*?)\) ?;", header()):
        if re.search(r"(?<!const )somhip_codebook \*(?!\*)", args):
            takes.add(name)
    assert takes == set(NEW)
    writers = {s for syms, _, _ in WRITERS.values() for s in syms}
    readers = {s for syms, _ in READERS.values() for s in syms}
    assert not (writers & readers)
    assert takes == writers | readers, takes ^ (writers | readers)


# ------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("case", sorted(WRITERS))
def test_writer_leaves_a_true_state(E, eng, oracle, data, ds, case):
    _, writer, flags = WRITERS[case]
    cb = PS.make_plain(E, eng, data)
    try:
        PS.prime(E, eng, cb, ds)
        before = cb.download()
        writer(E, eng, cb, ds, data)
        after = cb.download()
        assert (PS.bits(after) != PS.bits(before)).any(), "no row moved"
        st = E.debug_prepared_state(cb)
        assert st["bm_open"] == 0 and (st["prep_valid"], st["rowmajor_valid"]) == flags
        PS.check_state(E, eng, oracle, cb, ds, data[0], split_rows=None)
    finally:
        cb.close()


@gpu
def test_readers_keep_the_cache(E, eng, oracle, data, ds):
    cb = PS.make_plain(E, eng, data)
    try:
        st0 = PS.prime(E, eng, cb, ds)
        rows = cb.download()
        for case in sorted(READERS):
            READERS[case][1](E, eng, cb, ds)
            st = E.debug_prepared_state(cb)
            assert (st["prep_valid"], st["rowmajor_valid"], st["bm_open"]) == (1, 1, 0), case
            for name in ("chi", "clo"):
                assert np.array_equal(st[name], st0[name]), (case, name)
            assert np.array_equal(st["rowmajor"].view(np.uint32), st0["rowmajor"].view(np.uint32)), case
            assert np.array_equal(PS.bits(cb.download()), PS.bits(rows)), "%s moved rows" % case
            PS.check_state(E, eng, oracle, cb, ds, data[0], split_rows=rows)
    finally:
        cb.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# The regions of the 16 500 rows that the cuts below are made around
ONE_PLUS = (3000, 500)          # rows [3000, 3500): next to one prototype and of its class -- all choose it in role +
SPARSE = (8000, 40)             # rows [8000, 8040): next to two prototypes -- a piece that leaves most prototypes unchosen
AHEAD = (10000, 7, 8, 9)        # rows [10000, 10024): next to one prototype; pieces of 7, 8 and 9 rows are its whole lists
# rows, classes, dim, map (xdim, ydim: stored in 8x8 patches, as test_lvq_family_layouts builds it) or None.  Dims put the sp
# and cost columns d, d + 1 at the end of a 64-column sums block (62), across its edge (63), at the start of the next (64)
CONFIGS = [(3, 2, 1, None), (3, 2, 64, None), (70, 5, 62, None), (70, 2, 63, None), (130, 5, 64, None), (130, 2, 65, None),
           (70, 5, 129, None), (128, 5, 65, (16, 8)), (130, 5, 1, None)]
_cases = {}


def case(rows, classes, dim):
    """Gaussian classes and prototypes near the shrunken centres (test_glvq.clusters), with the regions above.  Built once
    per shape and left unchanged."""
    key = (rows, classes, dim)
    if key in _cases:
        return _cases[key]
    rs = np.random.RandomState(100 * rows + 10 * classes + dim)
    cen = (2.0 * rs.standard_normal((classes, dim))).astype(f32)
    dl = (np.arange(N) % classes).astype(np.int32)
    x = (cen[dl] + rs.standard_normal((N, dim))).astype(f32)
    cl = (np.arange(rows) % classes).astype(np.int32)
    c = (cen[cl] * 0.3 + rs.standard_normal((rows, dim))).astype(f32)
    near = lambda u, count, scale: (c[u] + f32(scale) * rs.standard_normal((count, dim))).astype(f32)
    a, cnt = ONE_PLUS
    u0 = rows // 2
    x[a:a + cnt] = near(u0, cnt, 1e-5)
    dl[a:a + cnt] = cl[u0]
    a, cnt = SPARSE
    x[a:a + cnt:2], x[a + 1:a + cnt:2] = near(0, cnt // 2, 1e-5), near(1, cnt // 2, 1e-5)
    dl[a:a + cnt:2], dl[a + 1:a + cnt:2] = cl[0], cl[1]
    a, cnt = AHEAD[0], sum(AHEAD[1:])
    u1 = rows - 1
    x[a:a + cnt] = near(u1, cnt, 1e-5)
    dl[a:a + cnt] = cl[u1]
    _cases[key] = (x, dl, c, cl, u0, u1)
    for arr in (x, dl, c, cl):
        arr.setflags(write=False)
    return _cases[key]


def codebook(E, eng, c, cl, on_map):
    return E.Codebook(eng, c, HEXA, BUBBLE, on_map[0], on_map[1], labels=cl) if on_map else E.Codebook(eng, c, labels=cl)


def cuts(E, eng, x, dl):
    """name -> the pieces (dataset, first, n) whose rows, in order, are the rows of x; and the data sets to close"""
    whole = E.Dataset(eng, x, labels=dl)
    tail = E.Dataset(eng, x[9000:], labels=dl[9000:])                    # a second Dataset object
    rolled = E.Dataset(eng, np.roll(x[9000:], 2500, axis=0), labels=np.roll(dl[9000:], 2500))   # rows (2500 + s) % 7500 of it are x[9000 + s]

    def at(edges):
        edges = [0] + list(edges) + [N]
        return [(whole, a, b - a) for a, b in zip(edges[:-1], edges[1:])]

    seven = np.cumsum([1000, 1, 2500, 37, 8192, 300])                    # seven uneven pieces, one a single row; 4470 left
    out = {"row 1": at([1]), "chunk - 1": at([CHUNK - 1]), "chunk": at([CHUNK]), "chunk + 1": at([CHUNK + 1]), "seven": at(seven),
           "one prototype in role +": at([ONE_PLUS[0], sum(ONE_PLUS)]), "most unchosen": at([SPARSE[0], sum(SPARSE)]),
           "lists of 7, 8, 9": at(np.cumsum(AHEAD)), "second data set": [(whole, 0, 9000), (tail, 0, N - 9000)],
           "wraps": [(whole, 0, 9000), (rolled, 2500, N - 9000)]}
    assert len(out["seven"]) == 7 and len(out["lists of 7, 8, 9"]) == 5 and 2500 + (N - 9000) > rolled.n
    return out, (whole, tail, rolled)


def state_equals(st, want, n, what):
    for key in ("sums_plus", "sums_minus", "cost", "n_plus", "n_minus"):
        assert same(st[key], want[key]), (what, key)
    assert (st["samples"], st["correct"]) == (n, want["correct"]), what


@gpu
@pytest.mark.parametrize("rows,classes,dim,on_map", CONFIGS)
def test_pieces_equal_one_call(E, eng, rows, classes, dim, on_map):
    """every cut of 16 500 rows leaves the rows, cost and correct of one glvq_train epoch, and Sp, Sm, cost[], np, nm and the
    tail of engine.glvq_sums of the whole; identity and sigmoid_beta = 2"""
    x, dl, c, cl, u0, u1 = case(rows, classes, dim)
    pieces, sets = cuts(E, eng, x, dl)
    whole = sets[0]
    ref = codebook(E, eng, c, cl, on_map)
    cb = codebook(E, eng, c, cl, on_map)
    # the regions are what their names say
    one = E.glvq_sums(ref, whole, *ONE_PLUS)
    assert one["n_plus"][u0] == ONE_PLUS[1]
    if rows >= 70:
        few = E.glvq_sums(ref, whole, *SPARSE)
        assert ((few["n_plus"] > 0) | (few["n_minus"] > 0)).sum() <= rows // 8
    at = AHEAD[0]
    for k in AHEAD[1:]:
        assert E.glvq_sums(ref, whole, at, k)["n_plus"][u1] == k
        at += k
    for beta in (0.0, 2.0):
        want = E.glvq_sums(ref, whole, 0, N, beta)
        cost, correct = E.glvq_train(ref, whole, 1, ALPHA, beta)
        rows_want = ref.download()
        ref.upload(c)
        assert not same(rows_want, np.asarray(c)) and correct[0] == want["correct"]
        for name, cut in pieces.items():
            cb.upload(c)
            E.glvq_begin(cb)
            addr, nbytes = E.glvq_state(cb)
            assert nbytes == 8 * (2 * rows * (dim + 1) + rows) + 4 * 2 * rows + 16
            assert not eng.copy_to_host(addr, nbytes).any()              # opens as all-zero bits
            for piece, first, n in cut:
                E.glvq_accumulate(cb, piece, first, n, beta)
            state_equals(E.glvq_state_arrays(cb), want, N, (name, beta))
            got = E.glvq_finish(cb, E.glvq_alpha(ALPHA, 1, 0))
            assert bits(f64(got[0])) == bits(cost)[0] and got[1:] == (correct[0], N), (name, beta, got, cost, correct)
            assert same(cb.download(), rows_want), (name, beta)
    E.glvq_end(cb)
    for o in (cb, ref) + sets:
        o.close()


@gpu
def test_the_one_call_is_the_replay(E, eng):
    """the side every piece is compared with, held to glvq_replay with the identity: rows, cost and correct of an epoch over
    the 16 500 rows by bit pattern, and so the pieces'"""
    rows, classes, dim, _ = CONFIGS[3]
    x, dl, c, cl, _, _ = case(rows, classes, dim)
    want, rcost, rcorrect = R.train(np.array(c), cl, x, dl, 1, ALPHA)
    cb, whole = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.glvq_train(cb, whole, 1, ALPHA)
    assert same(cb.download(), want) and same(cost, rcost) and (correct == rcorrect).all()
    cb.upload(c)
    E.glvq_begin(cb)
    E.glvq_accumulate(cb, whole, 0, CHUNK + 1)
    E.glvq_accumulate(cb, whole, CHUNK + 1, N - CHUNK - 1)
    got = E.glvq_finish(cb, E.glvq_alpha(ALPHA, 1, 0))
    assert same(cb.download(), want) and bits(f64(got[0])) == bits(rcost)[0] and got[1] == rcorrect[0]
    cb.close(); whole.close()


@gpu
def test_pieces_on_either_search_route(E, eng):
    """32768 x 512 and the smallest n for which the plan answers LIST: the one call over 70 rows takes the list route, the
    same rows as a piece below that n and the rest take the direct route for the first piece.  Keys, sums and rows are equal."""
    rows, dim, total = 32768, 512, 70
    n_list = next(n for n in range(1, 100) if E.glvq_plan(rows, dim, n) == E.GLVQ_LIST)
    assert n_list > 1 and E.glvq_plan(rows, dim, n_list - 1) == E.GLVQ_DIRECT and E.glvq_plan(rows, dim, total) == E.GLVQ_LIST
    assert E.glvq_plan(rows, dim, total - (n_list - 1)) == E.GLVQ_LIST
    rs = np.random.RandomState(512)
    cen = (0.5 * rs.standard_normal((3, dim))).astype(f32)
    dl = (np.arange(total) % 3).astype(np.int32)
    x = (cen[dl] + rs.standard_normal((total, dim))).astype(f32)
    cl = (np.arange(rows) % 3).astype(np.int32)
    c = (cen[cl] * 0.3 + rs.standard_normal((rows, dim))).astype(f32)
    c[:3] = x[:3]; cl[:3] = dl[:3]                                       # d+ = 0 for three samples
    cb, ref, whole = E.Codebook(eng, c, labels=cl), E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    a = n_list - 1
    keys = E.glvq_search(ref, whole, 0, total)                            # the plan's route: LIST
    for lo, n in ((0, a), (a, total - a)):
        part = E.glvq_search(ref, whole, lo, n)                          # the plan's route for the piece
        for k in range(4):
            assert same(part[k], keys[k][lo:lo + n]), (lo, k)
    assert E.glvq_search(ref, whole, 0, a)[4] == a                       # direct: every sample through the class-wise scan
    for beta in (0.0, 2.0):
        want = E.glvq_sums(ref, whole, 0, total, beta)
        cost, correct = E.glvq_train(ref, whole, 1, ALPHA, beta)
        cb.upload(c)
        E.glvq_begin(cb)
        E.glvq_accumulate(cb, whole, 0, a, beta)
        E.glvq_accumulate(cb, whole, a, total - a, beta)
        state_equals(E.glvq_state_arrays(cb), want, total, beta)
        got = E.glvq_finish(cb, E.glvq_alpha(ALPHA, 1, 0))
        assert bits(f64(got[0])) == bits(cost)[0] and got[1:] == (correct[0], total)
        assert same(cb.download(), ref.download())
        ref.upload(c)
    for o in (cb, ref, whole):
        o.close()


@gpu
@pytest.mark.parametrize("rows,classes,dim,on_map", [CONFIGS[2], CONFIGS[5], CONFIGS[7]])
def test_five_epochs_in_pieces(E, eng, rows, classes, dim, on_map):
    """begin / pieces / finish five times = glvq_train with 5 epochs, the per-epoch cost and correct included"""
    x, dl, c, cl, _, _ = case(rows, classes, dim)
    whole = E.Dataset(eng, x, labels=dl)
    ref, cb = codebook(E, eng, c, cl, on_map), codebook(E, eng, c, cl, on_map)
    cost, correct = E.glvq_train(ref, whole, 5, ALPHA, 2.0)
    for t in range(5):
        E.glvq_begin(cb)
        for first in range(0, N, 4000 + 7 * t):
            E.glvq_accumulate(cb, whole, first, min(4000 + 7 * t, N - first), 2.0)
        got = E.glvq_finish(cb, E.glvq_alpha(ALPHA, 5, t))
        assert bits(f64(got[0])) == bits(cost)[t] and got[1:] == (correct[t], N), t
    E.glvq_end(cb)
    assert same(cb.download(), ref.download())
    for o in (cb, ref, whole):
        o.close()


@gpu
@pytest.mark.parametrize("rows,classes,dim,on_map", [CONFIGS[3], CONFIGS[4], CONFIGS[7]])
def test_hand_off_between_codebooks(E, eng, rows, classes, dim, on_map):
    """A accumulates piece 1, its blob goes into B (same rows, its own state opened), B accumulates piece 2 and finishes: the
    one call.  Other engine calls between the pieces (a one-call run and the stages on a third codebook, which use the
    engine's GLVQ scratch) leave the state alone."""
    x, dl, c, cl, _, _ = case(rows, classes, dim)
    whole = E.Dataset(eng, x, labels=dl)
    ref = codebook(E, eng, c, cl, on_map)
    cost, correct = E.glvq_train(ref, whole, 1, ALPHA, 2.0)
    A, B, other = (codebook(E, eng, c, cl, on_map) for _ in range(3))
    E.glvq_begin(A)
    E.glvq_accumulate(A, whole, 0, 9100, 2.0)
    E.glvq_train(other, whole, 2, ALPHA, 2.0)
    E.glvq_sums(other, whole, 5, 77, 2.0)
    E.glvq_search(other, whole, 3, 500)
    E.glvq_begin(B)
    (a_addr, a_bytes), (b_addr, b_bytes) = E.glvq_state(A), E.glvq_state(B)
    assert a_bytes == b_bytes and a_addr != b_addr
    eng.copy_to_device(b_addr, eng.copy_to_host(a_addr, a_bytes))
    E.glvq_accumulate(B, whole, 9100, N - 9100, 2.0)
    got = E.glvq_finish(B, E.glvq_alpha(ALPHA, 1, 0))
    assert bits(f64(got[0])) == bits(cost)[0] and got[1:] == (correct[0], N)
    assert same(B.download(), ref.download())
    assert same(A.download(), np.asarray(c))                             # A never finished
    for o in (A, B, other, ref, whole):
        o.close()


@pytest.fixture()
def comm1(eng):
    h = C.c_void_p()
    assert eng.lib.somhip_comm_create_sockets(eng.h, 0, 1, None, C.byref(h)) == 0
    yield h
    eng.lib.somhip_comm_destroy(h)


@gpu
@pytest.mark.parametrize("rows,classes,dim,on_map", [CONFIGS[2], CONFIGS[7]])
def test_one_rank_equals_one_call(E, eng, comm1, rows, classes, dim, on_map):
    """somhip_glvq_train_ranks with one rank is somhip_glvq_train, a wrapped range and a slice of the epochs included; it
    leaves no state open behind it"""
    x, dl, c, cl, _, _ = case(rows, classes, dim)
    small = E.Dataset(eng, x[:1500], labels=dl[:1500])
    ref, cb = codebook(E, eng, c, cl, on_map), codebook(E, eng, c, cl, on_map)
    cost, correct = E.glvq_train(ref, small, 4, ALPHA, 2.0, start_epoch=1, count=3, first=700, n=1500)
    got = E.glvq_train_ranks(cb, small, comm1, 4, ALPHA, 2.0, start_epoch=1, count=3, first=700, n=1500)
    assert same(got[0], cost) and (got[1] == correct).all() and same(cb.download(), ref.download())
    with pytest.raises(Exception, match="somhip_glvq_begin"):
        E.glvq_finish(cb, 1.0)
    for o in (cb, ref, small):
        o.close()


def refused(fn, who, word):
    with pytest.raises(Exception) as ei:
        fn()
    assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)


@gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng, comm1):
    rs = np.random.RandomState(3)
    cen = (2.0 * rs.standard_normal((3, 4))).astype(f32)
    dl = (np.arange(700) % 3).astype(np.int32)
    x = (cen[dl] + rs.standard_normal((700, 4))).astype(f32)
    cl = (np.arange(6) % 3).astype(np.int32)
    c = (cen[cl] * 0.3 + rs.standard_normal((6, 4))).astype(f32)
    cb, whole = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 1] = 1
    masked = E.Dataset(eng, x, mask=mask, labels=dl)
    bare_ds, bare_cb = E.Dataset(eng, x), E.Codebook(eng, c)
    alien = E.Dataset(eng, x, labels=dl + 1)                             # label 3: no row of the codebook carries it
    one_class = E.Codebook(eng, c, labels=np.zeros(6, dtype=np.int32))
    zeros = E.Dataset(eng, x, labels=np.zeros(700, dtype=np.int32))
    shard = E.Codebook(eng, c[:3], labels=cl[:3], row_offset=0, n_global=6)
    other = E.Dataset(eng, x[:, :3], labels=dl)

    # nothing is open yet
    refused(lambda: E.glvq_accumulate(cb, whole), "somhip_glvq_accumulate", "somhip_glvq_begin")
    refused(lambda: E.glvq_finish(cb, 2.0), "somhip_glvq_finish", "somhip_glvq_begin")
    refused(lambda: E.glvq_state(cb), "somhip_glvq_state", "somhip_glvq_begin")
    refused(lambda: E.glvq_begin(bare_cb), "somhip_glvq_begin", "no labels")
    refused(lambda: E.glvq_begin(shard), "somhip_glvq_begin", "sharded")
    E.glvq_end(cb)                                                       # nothing to free: fine

    E.glvq_begin(cb)
    refused(lambda: E.glvq_finish(cb, 2.0), "somhip_glvq_finish", "holds no sample")
    E.glvq_accumulate(cb, whole, 0, 300)
    E.glvq_begin(one_class)
    before = eng.copy_to_host(*E.glvq_state(cb))
    who = "somhip_glvq_accumulate"
    refused(lambda: E.glvq_accumulate(cb, masked), who, "masked components")
    refused(lambda: E.glvq_accumulate(cb, bare_ds), who, "no labels")
    refused(lambda: E.glvq_accumulate(bare_cb, whole), who, "no labels")
    refused(lambda: E.glvq_accumulate(shard, whole), who, "sharded")
    refused(lambda: E.glvq_accumulate(cb, alien), who, "no row of the codebook carries")
    refused(lambda: E.glvq_accumulate(one_class, zeros), who, "every row of the codebook carries")
    refused(lambda: E.glvq_accumulate(cb, other), who, "dimension")
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 0), who, "n 0")
    refused(lambda: E.glvq_accumulate(cb, whole, 0, -5), who, "n -5")
    refused(lambda: E.glvq_accumulate(cb, whole, -1, 5), who, "first row")
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 2 ** 32), who, "32-bit")
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 2 ** 32 - 300), who, "32-bit")         # 300 taken: the total would be 2^32
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 10, -0.5), who, "sigmoid_beta")
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 10, float("nan")), who, "sigmoid_beta")
    who = "somhip_glvq_finish"
    refused(lambda: E.glvq_finish(cb, -1.0), who, "alpha_t")
    refused(lambda: E.glvq_finish(cb, float("nan")), who, "alpha_t")
    assert np.array_equal(eng.copy_to_host(*E.glvq_state(cb)), before)
    assert not eng.copy_to_host(*E.glvq_state(one_class)).any()
    for book, rows in ((cb, c), (one_class, c), (shard, c[:3]), (bare_cb, c)):
        assert same(book.download(), rows)

    # the rank loop refuses what the one call refuses, and a run in which no rank holds a row
    who = "somhip_glvq_train_ranks"
    refused(lambda: E.glvq_train_ranks(cb, masked, comm1, 3, 1.0), who, "masked components")
    refused(lambda: E.glvq_train_ranks(bare_cb, whole, comm1, 3, 1.0), who, "no labels")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 3, 1.0, n=-5), who, "n -5")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 3, 1.0, n=2 ** 32), who, "32-bit")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 0, 1.0, count=0), who, "epochs 0")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 3, -1.0), who, "alpha")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 3, 1.0, -1.0), who, "sigmoid_beta")
    refused(lambda: E.glvq_train_ranks(cb, whole, comm1, 3, 1.0, start_epoch=2, count=2), who, "outside")
    refused(lambda: E.glvq_train_ranks(cb, None, comm1, 3, 1.0, n=0), who, "no rank holds a row")
    assert np.array_equal(eng.copy_to_host(*E.glvq_state(cb)), before) and same(cb.download(), c)

    # the refused calls changed nothing: the accumulation goes on and ends as the one call
    ref = E.Codebook(eng, c, labels=cl)
    cost, correct = E.glvq_train(ref, whole, 1, 2.0)
    E.glvq_accumulate(cb, whole, 300, 400)
    got = E.glvq_finish(cb, 2.0)
    assert bits(f64(got[0])) == bits(cost)[0] and got[1:] == (correct[0], 700) and same(cb.download(), ref.download())
    # the codebook has moved
    refused(lambda: E.glvq_accumulate(cb, whole, 0, 10), "somhip_glvq_accumulate", "the codebook has moved")
    refused(lambda: E.glvq_finish(cb, 2.0), "somhip_glvq_finish", "the codebook has moved")
    assert same(cb.download(), ref.download())
    E.glvq_begin(cb)                                                     # ... until the next begin
    E.glvq_accumulate(cb, whole, 0, 10)

    # a writer of the rows closes the state: upload, the trainings, the batch map on a map
    for writer in (lambda: cb.upload(c), lambda: E.glvq_train(cb, whole, 1, 1.0), lambda: E.lvq_train(cb, whole, E.LVQ1, 20, 0.05),
                   lambda: E.glvq_update(cb, 1.0, 10, np.zeros((6, 5)), np.ones(6), np.zeros((6, 5)), np.ones(6))):
        E.glvq_begin(cb)
        E.glvq_accumulate(cb, whole, 0, 10)
        writer()
        rows = cb.download()
        refused(lambda: E.glvq_accumulate(cb, whole, 10, 10), "somhip_glvq_accumulate", "somhip_glvq_begin")
        refused(lambda: E.glvq_finish(cb, 2.0), "somhip_glvq_finish", "somhip_glvq_begin")
        refused(lambda: E.glvq_state(cb), "somhip_glvq_state", "somhip_glvq_begin")
        assert same(cb.download(), rows)
    rs = np.random.RandomState(5)
    mc = rs.standard_normal((16 * 8, 4)).astype(f32)
    on_map = E.Codebook(eng, mc, HEXA, BUBBLE, 16, 8, labels=(np.arange(128) % 3).astype(np.int32))
    for writer in (lambda: E.som_batchmap(on_map, whole, 1, 2.0), lambda: E.som_train(on_map, whole, 20, 0.05, 2.0, trace=False)):
        E.glvq_begin(on_map)
        E.glvq_accumulate(on_map, whole, 0, 10)
        writer()
        refused(lambda: E.glvq_finish(on_map, 2.0), "somhip_glvq_finish", "somhip_glvq_begin")
    E.glvq_begin(on_map)
    E.glvq_accumulate(on_map, whole, 0, 10)
    E.batchmap_begin(on_map)                                             # the batch map's pieces: the accumulate reads, the finish writes
    E.batchmap_accumulate(on_map, whole, 0, 100)
    E.glvq_state(on_map)
    E.batchmap_finish(on_map, 2.0)
    refused(lambda: E.glvq_finish(on_map, 2.0), "somhip_glvq_finish", "somhip_glvq_begin")
    E.glvq_begin(cb)
    E.glvq_end(cb)
    refused(lambda: E.glvq_accumulate(cb, whole), "somhip_glvq_accumulate", "somhip_glvq_begin")
    for o in (cb, ref, on_map, whole, masked, bare_ds, bare_cb, alien, one_class, zeros, shard, other):
        o.close()


@gpu
def test_destroying_the_codebook_frees_an_open_state(E, eng):
    x, dl, c, cl, _, _ = case(*CONFIGS[2][:3])
    small = E.Dataset(eng, x[:700], labels=dl[:700])
    for _ in range(3):
        cb = E.Codebook(eng, c, labels=cl)
        E.glvq_begin(cb)
        E.glvq_accumulate(cb, small)
        cb.close()
    small.close()


@gpu
def test_timing_counts_under_the_four_ids(E, eng):
    """the new launches are counted under K9's ids: per piece one search, the five of terms and grouping, the continued sums
    and the counts; the finish is one update"""
    x, dl, c, cl, _, _ = case(*CONFIGS[2][:3])
    small = E.Dataset(eng, x[:700], labels=dl[:700])
    cb = E.Codebook(eng, c, labels=cl)
    eng.timing(True)
    eng.timing_reset()
    E.glvq_begin(cb)
    E.glvq_accumulate(cb, small, 0, 300)
    E.glvq_accumulate(cb, small, 300, 400)
    E.glvq_finish(cb, 2.0)
    t = eng.glvq_timing()
    names = set(eng.timing_table())
    eng.timing(False)
    assert t["search"][0] == 2 and t["terms"][0] == 2 * 5 and t["k_glvq_sums"][0] == 2 * 2 and t["k_glvq_update"][0] == 1
    assert all(ms > 0 for _, ms in t.values())
    assert not [n for n in names if "glvq" in n]
    cb.close(); small.close()


# ---- the tool
def write_labelled(path, x, labels):
    with open(path, "w") as fh:
        fh.write("%d\n" % x.shape[1])
        for row, l in zip(x, labels):
            fh.write(" ".join("%g" % v for v in row) + " c%d\n" % int(l))


@pytest.fixture(scope="module")
def tool_runs(tools, tmp_path_factory):
    """the plain runs every option is compared with: a text file of 700 rows on 9 prototypes, a labelled gen: source of
    16 500 rows on 70, and a file of two rows; each (arguments, .cod bytes, -v lines)"""
    tmp = tmp_path_factory.mktemp("glvq_pieces")
    rs = np.random.RandomState(43)
    quant = lambda a: (np.round(a * 16) / 16).astype(f32)               # values that "%g" keeps
    cen = quant(2.0 * rs.standard_normal((3, 5)))
    dl = np.arange(700) % 3
    x = quant(cen[dl] + rs.standard_normal((700, 5)))
    cl = np.arange(9) % 3
    c = quant(cen[cl] * 0.3 + rs.standard_normal((9, 5)))
    dat, cod, two, gcod = tmp / "d.dat", tmp / "c.cod", tmp / "two.dat", tmp / "g.cod"
    write_labelled(dat, x, dl)
    write_labelled(cod, c, cl)
    write_labelled(two, x[:2], dl[:2])
    write_labelled(gcod, quant(4.0 * rs.standard_normal((70, 6))), np.arange(70) % 5)
    runs = {"file": ["-cin", cod, "-din", dat, "-epochs", 3, "-alpha", 2.5, "-sigmoid", 2, "-v"],
            "gen": ["-cin", gcod, "-din", "gen:k=5,dim=6,n=16500,seed=11,labels=1", "-epochs", 1, "-alpha", 20, "-v"],
            "two": ["-cin", cod, "-din", two, "-epochs", 2, "-alpha", 2.5, "-v"]}
    plain = {}
    for name, args in runs.items():
        out = tmp / (name + "_plain.cod")
        p = run("glvq", *args, "-cout", out)
        assert p.returncode == 0, p.stderr
        assert len(p.stdout.strip().split("\n")) == int(args[5])
        plain[name] = (args, out.read_bytes(), p.stdout)
    assert plain["file"][1] != cod.read_bytes()
    return tmp, plain


def same_run(tool_runs, name, extra, env=None):
    tmp, plain = tool_runs
    args, cod_bytes, lines = plain[name]
    out = tmp / ("%s_%s.cod" % (name, "_".join(str(a).strip("-") for a in extra) + ("_env" if env else "")))
    p = run("glvq", *args, "-cout", out, *extra, env=env)
    assert p.returncode == 0, (name, extra, p.stderr)
    assert out.read_bytes() == cod_bytes, (name, extra)
    got = p.stdout
    if (env or {}).get("SOMHIP_COMM") == "rccl":                         # librccl prints a banner of its own to stdout: not the tool's lines
        got = "".join(s for s in got.splitlines(True) if s.startswith("epoch "))
    assert got == lines, (name, extra)


@gpu
@pytest.mark.parametrize("buffer", [7, 16384, 100000])
def test_glvq_buffer_writes_the_plain_bytes(tool_runs, buffer):
    """-buffer 7, the class-wise scan's chunk and larger than either source"""
    same_run(tool_runs, "file", ["-buffer", buffer])
    same_run(tool_runs, "gen", ["-buffer", buffer])


@gpu
def test_glvq_buffer_of_one_row_and_one_row_short(tool_runs):
    """-buffer 1 on the file (every piece one row) and n - 1 on both sources (a last piece of one row)"""
    same_run(tool_runs, "file", ["-buffer", 1])
    same_run(tool_runs, "file", ["-buffer", 699])
    same_run(tool_runs, "gen", ["-buffer", 16499])


@gpu
def test_glvq_buffer_of_one_row_on_the_generated_source(tool_runs):
    """16 500 pieces of one row an epoch"""
    same_run(tool_runs, "gen", ["-buffer", 1])


@gpu
def test_glvq_buffer_without_v(tool_runs):
    tmp, plain = tool_runs
    args, cod_bytes, _ = plain["file"]
    out = tmp / "file_quiet.cod"
    p = run("glvq", *args[:-1], "-cout", out, "-buffer", 100)
    assert p.returncode == 0 and p.stdout == "" and out.read_bytes() == cod_bytes


@gpu
@pytest.mark.parametrize("gpus", [2, 3])
def test_glvq_gpus_writes_the_plain_bytes(tool_runs, gpus):
    """the ranks share the one GPU (at most three processes hold it): the state travels over the host sockets"""
    env = {"SOMHIP_COMM": "sockets"}
    same_run(tool_runs, "file", ["-gpus", gpus], env)
    same_run(tool_runs, "gen", ["-gpus", gpus], env)


@gpu
def test_glvq_gpus_with_an_empty_rank(tool_runs):
    same_run(tool_runs, "two", ["-gpus", 3], {"SOMHIP_COMM": "sockets"})


@gpu
def test_glvq_one_rank_through_rccl(tool_runs):
    """SOMHIP_COMM=rccl with one rank sends the loop through ncclAllReduce / ncclBroadcast on the engine's stream"""
    same_run(tool_runs, "file", ["-gpus", 1], {"SOMHIP_COMM": "rccl"})
