"""Dense batch neural gas (K10d: somhip_ng_train_dense and its stages, engine.ng_train_dense / ng_dense_schedule /
ng_dense_ranks / ng_dense_sums, bng -dense) against the numpy replay in ngas_dense_replay.py.

The ranks are integers and are compared exactly -- with the replay's lexsort and, up to 256 rows, with K10's own rank
search.  The sums come from the fp64 MFMA, which no numpy expression follows bit for bit: they are held to the bound
rslvq_replay.sums_longdouble derives for k_rslvq_sums, and to themselves by bit pattern across cuts and runs.  The
schedule is the library's own host arithmetic on both sides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ngas_dense_replay as D
import ngas_replay as R
from conftest import ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
HEXA, RECT, BUBBLE, GAUSSIAN = 3, 4, 1, 2
f32, f64 = np.float32, np.float64
CAP = 4096
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("bng", "qerror")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:8]


def gauss(seed, n, units, dim):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, dim)).astype(f32), rs.standard_normal((units, dim)).astype(f32)


def tied(seed, n, units, dim=2):
    """integer-valued data and a codebook with every row twice: equal distances everywhere"""
    rs = np.random.RandomState(seed)
    x = rs.randint(-2, 3, size=(n, dim)).astype(f32)
    half = rs.randint(-2, 3, size=((units + 1) // 2, dim)).astype(f32)
    return x, np.concatenate([half, half])[:units].copy()


# ------------------------------------------------------------------------------------------------ without a GPU
def header():
    hdr = open(os.path.join(ROOT, "include", "somhip_ng_dense.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def test_header_symbols_exported_and_mirrored(built):
    """what tests/test_build.py asks of somhip.h, of the header somhip.h includes: every declaration exported and mirrored
    (_lib.NG_DENSE_SIGNATURES), the mirror naming nothing else; the engine module has the wrappers"""
    from som_lvq_pak_amd import _lib, engine
    top = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r'^#include "somhip_ng_dense.h"$', top, flags=re.M)
    assert "somhip_ng_train_dense" not in re.sub(r"/\*.*?\*/", "", top, flags=re.S)     # declared once, in its own header
    declared = set(re.findall(r"\b(somhip_[a-z0-9_]+)\s*\(", header()))
    assert declared == {"somhip_ng_train_dense", "somhip_debug_ng_dense_schedule", "somhip_debug_ng_dense_ranks",
                        "somhip_debug_ng_dense_sums", "somhip_ng_dense_timing"}
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), "libsomhip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.NG_DENSE_SIGNATURES[name][1], name
    assert declared == set(_lib.NG_DENSE_SIGNATURES)
    assert not (set(_lib.NG_DENSE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.RSLVQ_SIGNATURES) | set(_lib.GLVQ_PIECES_SIGNATURES)))
    assert re.search(r"#define SOMHIP_NG_DENSE_MAX %d\b" % CAP, header()) and engine.NG_DENSE_MAX == CAP
    for name in ("ng_train_dense", "ng_dense_schedule", "ng_dense_ranks", "ng_dense_sums"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "ng_dense_timing")
    n, ms = (C.c_int64 * 3)(), (C.c_double * 3)()
    assert lib.somhip_ng_dense_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_ng_dense_timing: null engine"


def test_replay_ranks_are_a_permutation_and_k10s_order():
    """small integer data with duplicated rows: per sample the replay's ranks are a permutation of 0 .. units - 1, the
    inverse of ngas_replay.ranks at K = units, and among equal distances the later row has the smaller rank"""
    for seed, n, units in ((5, 30, 6), (6, 40, 13), (7, 10, 1), (8, 25, 64)):
        x, codes = tied(seed, n, units)
        rank, d = D.ranks(codes, x)
        assert rank.dtype == np.int32 and rank.shape == (n, units)
        assert (np.sort(rank, axis=1) == np.arange(units)[None, :]).all()
        u, dist = R.ranks(codes, x, units)
        assert (np.take_along_axis(rank, u.astype(np.int64), axis=1) == np.arange(units)[None, :]).all()
        same(np.take_along_axis(d, u.astype(np.int64), axis=1), dist)
        for s in range(n):
            for j in range(1, units):
                eq = np.nonzero(d[s, :j] == d[s, j])[0]
                assert (rank[s, eq] > rank[s, j]).all()
    codes = np.zeros((5, 2), dtype=f32)                                 # all rows identical: the ranks count down
    rank, _ = D.ranks(codes, np.ones((3, 2), dtype=f32))
    assert (rank == np.arange(4, -1, -1)[None, :]).all()


def test_schedule_weights(built):
    """the weight of every rank, answered without a GPU: lambda_t is K10's, w[0] == 1.0, the weights fall monotonically,
    no rule cuts them (at lambda 128 the 257th rank and the 4096th still weigh), within 2 ulp of numpy's exp, and at a small
    lambda the tail underflows to +0.0"""
    from som_lvq_pak_amd import engine as E
    for units in (1, 2, 256, 257, 1000, CAP):
        lam, w = E.ng_dense_schedule(units, 1, 0, 128.0, 0.01)
        assert lam == 128.0 and w.shape == (units,) and w[0] == 1.0
        assert (np.diff(w) < 0).all() and (w > 0).all()
        ref = np.exp(-np.arange(units, dtype=f64) / lam)
        assert (np.abs(w - ref) <= 2 * np.spacing(ref)).all()
    assert E.ng_dense_schedule(CAP, 1, 0, 128.0, 0.01)[1][256] == np.exp(-2.0)         # what K10 drops at the default lambda
    lam, w = E.ng_dense_schedule(CAP, 1, 0, 0.5, 0.01)
    assert w[0] == 1.0 and (np.diff(w) <= 0).all()
    dead = np.nonzero(w == 0.0)[0]
    assert len(dead) and dead[0] <= 380 and (bits(w[dead[0]:]) == 0).all()              # exp(-745.2) is the last double above 0
    T, l0, le = 7, 300.0, 0.01
    for t in range(T):
        assert E.ng_dense_schedule(600, T, t, l0, le)[0] == E.ng_schedule(600, T, t, l0, le)[0]
    assert E.ng_dense_schedule(1000, 1, 0)[0] == 128.0                                  # the default lambda0
    for bad, word in ((dict(epochs=0, t=0), "epochs 0"), (dict(epochs=3, t=3), "epoch 3"), (dict(lambda0=0.0), "lambda0"),
                      (dict(lambda_end=7.0), "lambda_end"), (dict(units=0), "units")):
        a = dict(units=10, epochs=3, t=1, lambda0=5.0, lambda_end=0.5)
        a.update(bad)
        with pytest.raises(Exception, match="somhip_debug_ng_dense_schedule: .*" + re.escape(word)):
            E.ng_dense_schedule(**a)


def test_bng_dense_refusals_need_no_engine(tools, tmp_path):
    """-dense with -ranks, a codebook above the cap and masked data: refused before an engine is asked for, so they hold
    without a GPU; and everything bng refuses is refused with -dense too"""
    p = run("bng", "-help")
    assert p.returncode == 0 and "-dense" in p.stdout
    cod = tmp_path / "m.cod"
    cod.write_text("2\n0 0\n1 0\n0 1\n1 1\n")
    dat = tmp_path / "d.dat"
    dat.write_text("2\n0.25 0.5\n0.75 0.5\n")
    out = tmp_path / "o.cod"
    p = run("bng", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 2, "-dense", "-ranks", 4)
    assert p.returncode == 1 and p.stderr.startswith("bng: -dense") and "-ranks" in p.stderr, p.stderr
    big = tmp_path / "big.cod"
    big.write_text("2\n" + "".join("%d %d\n" % (i % 64, i // 64) for i in range(CAP + 1)))
    p = run("bng", "-cin", big, "-din", dat, "-cout", out, "-epochs", 2, "-dense")
    assert p.returncode == 1 and p.stderr.startswith("bng: ") and "%d rows" % (CAP + 1) in p.stderr and str(CAP) in p.stderr, p.stderr
    xdat = tmp_path / "x.dat"
    xdat.write_text("2\nx 0.5\n0.75 0.5\n")
    p = run("bng", "-cin", cod, "-din", xdat, "-cout", out, "-epochs", 2, "-dense")
    assert p.returncode == 1 and p.stderr.startswith("bng: ") and "masked components" in p.stderr, p.stderr
    xcod = tmp_path / "x.cod"
    xcod.write_text("2\nx 0\n1 0\n0 1\n1 1\n")
    p = run("bng", "-cin", xcod, "-din", dat, "-cout", out, "-epochs", 2, "-dense")
    assert p.returncode == 1 and p.stderr.startswith("bng: ") and "masked components" in p.stderr, p.stderr
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3\n4 5 6\n")
    p = run("bng", "-cin", cod, "-din", dim3, "-cout", out, "-epochs", 2, "-dense")
    assert p.returncode == 1 and "different dimensions" in p.stderr
    for args, word in ((("-epochs", 0), "-epochs"), (("-epochs", 2, "-lambda", 0), "-lambda"), (("-epochs", 2, "-lambda_end", 5), "-lambda_end")):
        p = run("bng", "-cin", cod, "-din", dat, "-cout", out, "-dense", *args)
        assert p.returncode == 1 and p.stderr.startswith("bng: " + word), (args, p.stderr)
    assert not out.exists()


BEHAVIOUR_SEED = 4


def far_start(seed=BEHAVIOUR_SEED):
    """three Gaussian clusters of 100 samples each in the plane, spread 0.5 and 8 apart, and 512 units started around the
    centre of the first one at a spread of 4: the units on the side that faces no other cluster are farther from every
    sample than 256 others are -- at the start, and after the fed units have moved towards the data (the settings were
    tried on the CPU at seeds 1 .. 3 and left 27 .. 33 such units; clusters 14 apart left none after three epochs)"""
    rs = np.random.RandomState(seed)
    cen = np.array([[0, 0], [8, 0], [0, 8]], dtype=f32)
    which = np.arange(300) % 3
    x = (cen[which] + 0.5 * rs.standard_normal((300, 2))).astype(f32)
    start = (rs.standard_normal((512, 2)) * 4.0).astype(f32)
    return x, start


def test_replay_the_dense_form_moves_what_truncation_leaves_behind(built):
    """the definition's point, in the replay alone: three epochs at lambda 128 on 512 units.  Truncated at 256 ranks, some
    units are among no sample's 256 nearest in any epoch and keep the bits they started with; the dense form feeds and
    moves every one of them"""
    from som_lvq_pak_amd import engine as E
    x, start = far_start()
    w = E.ng_dense_schedule(512, 3, 0, 128.0, 128.0)[1]
    assert all(E.ng_dense_schedule(512, 3, t, 128.0, 128.0)[0] == 128.0 for t in range(3))
    dense = D.train(start, x, lambda t: w, 3)
    cut = D.train(start, x, lambda t: w, 3, truncate=256)
    stayed = (bits(cut) == bits(start)).all(axis=1)
    assert stayed.sum() >= 1, stayed.sum()
    assert (bits(dense) != bits(start)).any(axis=1).all()
    rank0, _ = D.ranks(start, x)
    assert (rank0[:, stayed] >= 256).all()                              # no sample ranks them among its 256 nearest
    # (a figure, not a claim: three epochs at a lambda this wide pull every fed unit towards the mean of the data)
    qd = R.qerror_chain(R.distances(dense, x).min(axis=1))
    qc = R.qerror_chain(R.distances(cut, x).min(axis=1))
    print("qerror after 3 epochs: dense %g, truncated at 256 %g; %d units never fed" % (qd, qc, stayed.sum()))


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


def check_ranks(E, eng, codes, x, windows=None, lattice=None):
    cb = E.Codebook(eng, codes, *(lattice or ()))
    ds = E.Dataset(eng, x)
    units = codes.shape[0]
    for first, n in windows or [(0, x.shape[0])]:
        xs = R.rows_of(x, first, n)
        want, wd = D.ranks(codes, xs)
        got, gd = E.ng_dense_ranks(cb, ds, first, n)
        assert got.dtype == np.int32 and np.array_equal(got, want), (first, n, np.argwhere(got != want)[:8])
        same(gd, wd)
        if units <= 256:                                                # K10's own search, inverted
            u, dist = E.ng_ranks(cb, ds, units, first, n)
            inv = np.empty_like(u)
            np.put_along_axis(inv, u.astype(np.int64), np.broadcast_to(np.arange(units, dtype=np.int32), u.shape), axis=1)
            assert np.array_equal(got, inv)
            same(np.take_along_axis(gd, u.astype(np.int64), axis=1), dist)
    same(cb.download(), codes)                                          # the stage writes no row
    cb.close(); ds.close()


# ---- the ranks, exact
@gpu
@pytest.mark.parametrize("units", [1, 2, 63, 64, 65, 257, 1023, 1024, 1025, CAP])
def test_ranks_units(E, eng, units):
    """both sides of the wave, of a power of two of the sort, and the cap; small dims at the large unit counts"""
    x, codes = gauss(200 + units, 70 if units > 300 else 150, units, 3 if units > 300 else 5)
    check_ranks(E, eng, codes, x)


@gpu
@pytest.mark.parametrize("dim", [1, 63, 65, 129])
def test_ranks_dims(E, eng, dim):
    x, codes = gauss(300 + dim, 100, 70, dim)
    check_ranks(E, eng, codes, x)


@gpu
def test_ranks_sample_counts_and_wrap(E, eng):
    """1, 63 and 65 samples and one more than the distance stage's chunk, with first wrapping round the data set"""
    x, codes = gauss(7, 700, 12, 3)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    chunk = E.scan_plan(cb, ds, 10 ** 6, 9)["chunk"]
    cb.close(); ds.close()
    assert chunk % 64 == 0 and chunk >= E.rslvq_chunk(12)[0]
    check_ranks(E, eng, codes, x, [(0, 1), (699, 1), (0, 63), (5, 65), (690, 65), (650, chunk + 1)])


@gpu
@pytest.mark.parametrize("units", [1, 2, 6, 65, 300])
def test_ranks_ties_take_the_later_row_first(E, eng, units):
    """duplicated rows and integer-valued data: equal distances at every rank; all rows identical: the ranks count down"""
    x, codes = tied(11 + units, 200, units)
    check_ranks(E, eng, codes, x)
    flat = np.full((units, 2), 1.5, dtype=f32)
    check_ranks(E, eng, flat, x[:10])
    cb, ds = E.Codebook(eng, flat), E.Dataset(eng, x[:10])
    assert (E.ng_dense_ranks(cb, ds)[0] == np.arange(units - 1, -1, -1)[None, :]).all()
    cb.close(); ds.close()


@gpu
def test_ranks_on_patch_stored_maps_are_by_unit(E, eng):
    """a 32 x 8 and an 8 x 24 map are stored patch by patch: a column of the ranks is a unit, not a storage row"""
    for xdim, ydim in ((32, 8), (8, 24)):
        x, codes = gauss(90 + xdim, 80, xdim * ydim, 5)
        check_ranks(E, eng, codes, x, lattice=(HEXA, BUBBLE, xdim, ydim))


# ---- the sums, within the bound and by bit pattern among themselves
def check_sums(E, eng, codes, x, lam, windows=None, chunks=(0,), lattice=None):
    cb = E.Codebook(eng, codes, *(lattice or ()))
    ds = E.Dataset(eng, x)
    units = codes.shape[0]
    w = E.ng_dense_schedule(units, 1, 0, lam, lam)[1]                    # (one epoch: lambda0 itself, the library's own exp)
    out = []
    for first, n in windows or [(0, x.shape[0])]:
        wS, wW, bS, bW = D.sums_bound(codes, x, w, first, n)
        runs = [E.ng_dense_sums(cb, ds, lam, first, n, c) for c in chunks]
        S, W = runs[0]
        eS, eW = np.abs(S - wS).astype(f64), np.abs(W - wW).astype(f64)
        print("ng dense sums", (units, codes.shape[1], n, first), "largest difference / bound:", float((eS / bS).max()), float((eW / bW).max()))
        assert (eS <= bS).all() and (eW <= bW).all(), (float((eS / bS).max()), float((eW / bW).max()))
        for S2, W2 in runs[1:]:
            same(S2, S); same(W2, W)
        out.append((S, W))
    same(cb.download(), codes)
    cb.close(); ds.close()
    return out


@gpu
@pytest.mark.parametrize("shape", [(1, 3), (2, 1), (65, 63), (257, 65), (300, 129), (1025, 4)])
def test_sums_within_the_mfma_bound(E, eng, shape):
    units, dim = shape
    x, codes = gauss(400 + units, 330, units, dim)
    check_sums(E, eng, codes, x, 40.0, [(0, 330), (300, 100)])
    check_sums(E, eng, codes, x, 0.3)                                   # most weights underflow to +0.0


@gpu
def test_sums_cuts_and_runs_leave_the_same_bits(E, eng):
    """cut at 64, at 128, at one chunk and by the engine's own rule: the accumulators are continued, so every cut is the
    one run; a second call leaves the bits of the first"""
    x, codes = gauss(21, 4096 + 65, 70, 5)
    chunk = E.rslvq_chunk(70)[0]
    assert chunk == 4096
    (a,) = check_sums(E, eng, codes, x, 9.0, chunks=(0, 64, 128, chunk))
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    E.ng_dense_sums(cb, ds, 2.0, n=100)                                 # (another call in between: nothing of it stays)
    b = E.ng_dense_sums(cb, ds, 9.0)
    same(b[0], a[0]); same(b[1], a[1])
    with pytest.raises(Exception, match="somhip_debug_ng_dense_sums: chunk 100"):
        E.ng_dense_sums(cb, ds, 9.0, chunk=100)
    cb.close(); ds.close()


@gpu
def test_patch_stored_and_plain_codebooks_agree_by_unit(E, eng):
    """a patch-stored lattice codebook and a lattice-less one of the same rows: the same S, W and updated rows, by unit"""
    for xdim, ydim in ((32, 8), (8, 24)):
        x, codes = gauss(60 + xdim, 400, xdim * ydim, 6)
        ds = E.Dataset(eng, x)
        plain = E.Codebook(eng, codes)
        patch = E.Codebook(eng, codes, HEXA, GAUSSIAN, xdim, ydim)
        S, W = E.ng_dense_sums(plain, ds, 30.0)
        S2, W2 = E.ng_dense_sums(patch, ds, 30.0)
        same(S2, S); same(W2, W)
        q1 = E.ng_train_dense(plain, ds, 2, 30.0, 1.0)
        q2 = E.ng_train_dense(patch, ds, 2, 30.0, 1.0)
        same(patch.download(), plain.download()); same(q2, q1)
        assert (bits(plain.download()) != bits(codes)).any(axis=1).all()
        plain.close(); patch.close(); ds.close()


# ---- whole epochs
@pytest.fixture(scope="module")
def small_run():
    return gauss(51, 700, 300, 6)


@gpu
def test_epochs_in_one_call_or_many_or_by_hand(E, eng, small_run):
    """5 epochs in one call, in five calls, in two calls without q, and as the stages chained by hand (ng_dense_sums, then
    K10's ng_update) leave the same bits"""
    x, codes = small_run
    T = 5
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    wq = E.ng_train_dense(cb, ds, T)
    want = cb.download()
    assert wq.dtype == f32 and wq.shape == (T,) and (wq > 0).all()
    cb.upload(codes)
    qs = [E.ng_train_dense(cb, ds, T, start_epoch=t, count=1)[0] for t in range(T)]
    same(cb.download(), want); same(np.array(qs, dtype=f32), wq)
    cb.upload(codes)
    assert E.ng_train_dense(cb, ds, T, start_epoch=0, count=2, qerror=False) is None
    E.ng_train_dense(cb, ds, T, start_epoch=2, count=3, qerror=False)
    same(cb.download(), want)
    cb.upload(codes)
    for t in range(T):
        S, W = E.ng_dense_sums(cb, ds, E.ng_dense_schedule(300, T, t)[0])
        E.ng_update(cb, np.ones(300, dtype=np.uint32), S, W)
    same(cb.download(), want)
    cb.close(); ds.close()


@gpu
def test_qerror_is_the_qerror_routes_figure(E, eng, small_run):
    """qerror_out[t] is find_qerror's float chain over engine.find_winners' distances of the codebook epoch t started from,
    in the order of the run's samples"""
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    for t in range(3):
        _, diff, _ = E.find_winners(cb, ds)
        want = R.qerror_chain(np.roll(np.asarray(diff).reshape(-1), -5))           # (the chain runs in the run's order: from row 5 on)
        q = E.ng_train_dense(cb, ds, 3, start_epoch=t, count=1, first=5)
        assert bits(q)[0] == bits(np.array([want], dtype=f32))[0], (t, q, want)
    cb.close(); ds.close()


@gpu
def test_rows_are_within_the_carried_bound_of_the_replay(E, eng, small_run):
    """Epoch by epoch from the rows the device itself left (a row a rounding apart may rank differently, so the replay starts
    each epoch where the device did): every row is within ulp32 / 2 plus the sums' bound carried through the division of
    the replay's S / W.  With |S~ - S| <= bS and |W~ - W| <= bW (rslvq_replay.sums_longdouble's, on the library's own
    weights), q = S / W: |S~ / W~ - q| <= (bS + |q| bW) / (W - bW), the fp64 division adds
    2^-53 |q~|, the rounding to float ulp32(q) / 2."""
    x, codes = small_run
    n, units = x.shape[0], codes.shape[0]
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    T = 3
    for t in range(T):
        before = cb.download()
        lam, w = E.ng_dense_schedule(units, T, t, 40.0, 2.0)
        E.ng_train_dense(cb, ds, T, 40.0, 2.0, start_epoch=t, count=1, qerror=False)
        after = cb.download()
        q, S, W, A, _ = D.epoch(before, x, w)
        _, _, bS, bW = D.sums_bound(before, x, w)
        Wd = W.astype(f64)
        assert (Wd > 2 * bW).all()
        _, e = np.frexp(np.abs(q).astype(f64))
        ulp32 = np.ldexp(f64(1.0), np.maximum(e - 24, -149))
        carried = (bS + np.abs(q).astype(f64) * bW[:, None]) / (Wd - bW)[:, None] + 2.0 ** -52 * np.abs(q).astype(f64)
        err = np.abs(after.astype(np.longdouble) - q).astype(f64)
        print("ng dense epoch", t, "largest error / bound:", float((err / (ulp32 / 2 + carried)).max()))
        assert (err <= ulp32 / 2 + carried).all(), float((err / (ulp32 / 2 + carried)).max())
    cb.close(); ds.close()


@gpu
def test_the_dense_form_moves_what_truncation_leaves_behind(E, eng):
    """far_start's run on the device: after three epochs at lambda 128 somhip_ng_train leaves the bits of the units the
    replay says are never fed, and somhip_ng_train_dense has moved every unit"""
    x, start = far_start()
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, start)
    E.ng_train(cb, ds, 3, 128.0, 128.0, ranks=256, qerror=False)
    stayed = (bits(cb.download()) == bits(start)).all(axis=1)
    assert stayed.sum() >= 1
    cb.upload(start)
    E.ng_train_dense(cb, ds, 3, 128.0, 128.0, qerror=False)
    assert (bits(cb.download()) != bits(start)).any(axis=1).all()
    cb.close(); ds.close()


@gpu
def test_stage_timing_counts_launches(E, eng, small_run):
    x, codes = small_run
    ds, cb = E.Dataset(eng, x), E.Codebook(eng, codes)
    eng.timing(True)
    eng.timing_reset()
    E.ng_train_dense(cb, ds, 2, qerror=False)
    t, k10 = eng.ng_dense_timing(), eng.ng_timing()
    eng.timing(False)
    assert t["distances"][0] == 2 and t["k_ng_dense_weights"][0] == 2 and t["sums"][0] == 2 and k10["k_ng_update"][0] == 2
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


@gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng):
    x, codes = gauss(52, 200, 12, 6)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    shard = E.Codebook(eng, codes[:6], row_offset=3, n_global=12)
    other = E.Dataset(eng, x[:, :5])
    over = gauss(53, 1, CAP + 1, 6)[1]
    big = E.Codebook(eng, over)

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    who = "somhip_ng_train_dense"
    for ranks in (1, 4, 256, 257, -1):
        refused(lambda: E.ng_train_dense(cb, ds, 3, ranks=ranks), who, "ranks")
    refused(lambda: E.ng_train_dense(big, ds, 3), who, "SOMHIP_NG_DENSE_MAX")
    refused(lambda: E.ng_train_dense(cb, masked, 3), who, "masked components")
    refused(lambda: E.ng_train_dense(shard, ds, 3), who, "sharded")
    refused(lambda: E.ng_train_dense(cb, other, 3), who, "dimension")
    refused(lambda: E.ng_train_dense(cb, ds, 3, n=2 ** 32), who, "32-bit")
    refused(lambda: E.ng_train_dense(cb, ds, 3, n=0), who, "n 0")
    refused(lambda: E.ng_train_dense(cb, ds, 3, n=-5), who, "n -5")
    refused(lambda: E.ng_train_dense(cb, ds, 3, first=-1), who, "first row")
    refused(lambda: E.ng_train_dense(cb, ds, 0, count=0), who, "epochs 0")
    refused(lambda: E.ng_train_dense(cb, ds, 3, lambda0=0.0), who, "lambda0")
    refused(lambda: E.ng_train_dense(cb, ds, 3, lambda0=1.0, lambda_end=2.0), who, "lambda_end")
    refused(lambda: E.ng_train_dense(cb, ds, 3, start_epoch=-1, count=1), who, "outside")
    refused(lambda: E.ng_train_dense(cb, ds, 3, start_epoch=2, count=2), who, "outside")
    refused(lambda: E.ng_train_dense(cb, ds, 3, start_epoch=3, count=1), who, "outside")
    who = "somhip_debug_ng_dense_ranks"
    refused(lambda: E.ng_dense_ranks(big, ds, 0, 1), who, "SOMHIP_NG_DENSE_MAX")
    refused(lambda: E.ng_dense_ranks(cb, masked), who, "masked components")
    refused(lambda: E.ng_dense_ranks(shard, ds), who, "sharded")
    refused(lambda: E.ng_dense_ranks(cb, ds, 0, 0), who, "n 0")
    who = "somhip_debug_ng_dense_sums"
    refused(lambda: E.ng_dense_sums(big, ds, 3.0), who, "SOMHIP_NG_DENSE_MAX")
    refused(lambda: E.ng_dense_sums(cb, masked, 3.0), who, "masked components")
    refused(lambda: E.ng_dense_sums(shard, ds, 3.0), who, "sharded")
    refused(lambda: E.ng_dense_sums(cb, other, 3.0), who, "dimension")
    refused(lambda: E.ng_dense_sums(cb, ds, 0.0), who, "lambda")
    refused(lambda: E.ng_dense_sums(cb, ds, float("nan")), who, "lambda")
    refused(lambda: E.ng_dense_sums(cb, ds, 3.0, -1), who, "first row")
    # ... and the truncated form is refused beyond its ranks as before
    refused(lambda: E.ng_train(cb, ds, 3, ranks=257), "somhip_ng_train", "ranks 257 outside 0 .. 256")
    for c, rows in ((cb, codes), (shard, codes[:6]), (big, over)):
        same(c.download(), rows)
    for o in (cb, shard, big, ds, masked, other):
        o.close()


# ---- the tool
@gpu
def test_bng_dense_writes_the_engines_codebook(E, eng, tools, tmp_path):
    from som_lvq_pak_amd import textio
    rs = np.random.RandomState(71)
    x = (np.round(rs.standard_normal((700, 4)) * 16) / 16).astype(f32)              # values that "%g" keeps
    codes = (np.round(rs.standard_normal((300, 4)) * 16) / 16).astype(f32)
    dat, cod, out = tmp_path / "d.dat", tmp_path / "m.cod", tmp_path / "o.cod"
    d = textio.Entries()
    d.dim, d.points = 4, x
    textio.write_entries(str(dat), d)
    tab = textio.LabelTable()
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = 4, HEXA, GAUSSIAN, 20, 15, codes
    m.labels = [[tab.to_index("u%d" % (i % 4))] if i % 3 else [] for i in range(300)]
    textio.write_entries(str(cod), m, tab)

    p = run("bng", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 4, "-dense", "-v")
    assert p.returncode == 0, p.stderr
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, x)
    q = E.ng_train_dense(cb, ds, 4)
    rows = cb.download()
    tab2 = textio.LabelTable()
    got = textio.read_entries(str(out), tab2)[0]
    assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (4, HEXA, GAUSSIAN, 20, 15)        # the header it read
    assert [[tab2.names[l] for l in ls] for ls in got.labels] == [[tab.names[l] for l in ls] for ls in m.labels]
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=f32)
    same(got.points, printed)
    want = ["epoch %d lambda %.17g ranks %d qerror %f" % (t, E.ng_dense_schedule(300, 4, t)[0], 300, float(f32(q[t]) / f32(700)))
            for t in range(4)]
    assert p.stdout.strip().split("\n") == want
    # the options reach the engine; the qerror tool on the result prints the figure a further one-epoch run prints first
    out2 = tmp_path / "o2.cod"
    p = run("bng", "-cin", cod, "-din", dat, "-cout", out2, "-epochs", 3, "-lambda", 40, "-lambda_end", 0.5, "-dense")
    cb.upload(codes)
    E.ng_train_dense(cb, ds, 3, 40.0, 0.5, qerror=False)
    assert p.returncode == 0 and p.stdout == ""
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)
    same(textio.read_entries(str(out2))[0].points, printed)
    p = run("qerror", "-cin", out, "-din", dat)
    assert p.returncode == 0, p.stderr
    nxt = run("bng", "-cin", out, "-din", dat, "-cout", tmp_path / "o3.cod", "-epochs", 1, "-dense", "-v")
    figure = re.search(r" is (\d+\.\d{6}) per sample \(700 samples\)", p.stdout)
    assert figure and nxt.returncode == 0 and nxt.stdout.strip().split("\n")[0].split(" qerror ")[1] == figure.group(1)
    cb.close(); ds.close()
