"""Batch neural gas (K10: somhip_ng_train and its stages, engine.ng_train / ng_schedule / ng_ranks / ng_sums / ng_update, the
bng tool) against the numpy replay in ngas_replay.py.

Everything on the GPU is compared by bit pattern: the ranks are the engine's exact k-NN search under find_winner_knn's
order of ties, the sums are chains of fp64 additions in data order of products that round once, the update is one fp64
division and one rounding to float, and the schedule is the library's own host arithmetic on both sides.  The replay
itself is checked on the CPU against a dense np.longdouble form within a bound derived from the chain lengths."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ngas_replay as R
from conftest import ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
HEXA, RECT, BUBBLE, GAUSSIAN = 3, 4, 1, 2
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("bng", "qerror", "datconv")):
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
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.SIGNATURES
    for name in ("somhip_ng_train", "somhip_debug_ng_schedule", "somhip_debug_ng_ranks", "somhip_debug_ng_sums", "somhip_debug_ng_update",
                 "somhip_ng_timing"):
        assert hasattr(lib, name) and name in S, name
    assert S["somhip_ng_train"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.NgParams), _lib.c_float_p])
    assert S["somhip_ng_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.NgParams._fields_] == ["epochs", "lambda0", "lambda_end", "ranks", "start_epoch", "count", "first", "n"]
    assert C.sizeof(_lib.NgParams) == 64
    for name in ("ng_train", "ng_schedule", "ng_ranks", "ng_sums", "ng_update"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "ng_timing")
    assert lib.somhip_knn_max() == 256


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert "TRUNCATED at the 256 nearest units" in hdr
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int somhip_ng_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_ng_params *p, float *qerror_out );" in hdr
    assert "int somhip_ng_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);" in hdr
    m = re.search(r"typedef struct somhip_ng_params \{(.*?)\} somhip_ng_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int64_t epochs; double lambda0; double lambda_end; int64_t ranks; "
                                                            "int64_t start_epoch, count; int64_t first, n;")


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 3)(), (C.c_double * 3)()
    assert lib.somhip_ng_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_ng_timing: null engine"


def test_schedule_is_host_arithmetic(built):
    """lambda_t, K_t and the weights, answered without a GPU: the rule 1 + floor(17 lambda) on both sides of an integer, one
    epoch, the override, the caps at the codebook's rows and at 256, the end points of a run, and the weights within 2 ulp
    of numpy's exp (the library's exp and numpy's are each within an ulp of the true value; nothing tighter is claimed)"""
    from som_lvq_pak_amd import engine as E
    for lam0, want in ((2.999 / 17, 3), (3.001 / 17, 4), (0.01, 1), (1.0 / 17 - 1e-9, 1), (1.0 / 17 + 1e-9, 2), (1.0, 18)):
        lam, K, w = E.ng_schedule(100, 1, 0, lam0, lam0 / 2)
        assert lam == lam0 and K == want == 1 + int(np.floor(17.0 * lam0)) and w.shape == (K,), (lam0, lam, K)
    lam, K, w = E.ng_schedule(100, 1, 0, 3.0, 0.01)                      # T == 1: lambda0, whatever lambda_end is
    assert lam == 3.0 and K == 52
    assert E.ng_schedule(5, 1, 0, 100.0, 1.0)[1] == 5                    # the cap at the rows
    assert E.ng_schedule(256, 1, 0, 100.0, 1.0)[1] == 256 and E.ng_schedule(1000, 1, 0, 100.0, 1.0)[1] == 256
    assert E.ng_schedule(1000, 1, 0, 15.0 - 1e-9, 1.0)[1] == 255         # 17 * 15 = 255: just below, the rule; at it, the cap
    assert E.ng_schedule(1000, 1, 0, 15.0, 1.0)[1] == 256
    assert E.ng_schedule(12, 1, 0)[0] == 6.0 and E.ng_schedule(1000, 1, 0)[0] == 128.0      # the default lambda0
    for ranks, units in ((1, 100), (7, 100), (9, 5), (256, 3)):          # the override, also beyond the rows
        lam, K, w = E.ng_schedule(units, 4, 2, 50.0, 0.01, ranks=ranks)
        assert K == ranks and w.shape == (ranks,)
    T, l0, le = 7, 6.0, 0.01
    for t in range(T):
        lam, K, w = E.ng_schedule(40, T, t, l0, le)
        want = l0 * (le / l0) ** (t / (T - 1))
        assert abs(lam - want) <= 4 * np.spacing(want), (t, lam, want)
        assert K == min(40, 1 + int(np.floor(17.0 * lam)))
        ref = np.exp(-np.arange(K, dtype=f64) / lam)
        assert w[0] == 1.0 and (np.abs(w - ref) <= 2 * np.spacing(ref)).all(), (t, np.abs(w - ref) / np.spacing(ref))
    assert E.ng_schedule(40, T, 0, l0, le)[0] == l0 and E.ng_schedule(40, T, T - 1, l0, le)[0] == l0 * (le / l0)
    for bad, word in ((dict(epochs=0, t=0), "epochs 0"), (dict(epochs=3, t=3), "epoch 3"), (dict(epochs=3, t=-1), "epoch -1"),
                      (dict(lambda0=0.0), "lambda0"), (dict(lambda0=-1.0), "lambda0"), (dict(lambda0=float("nan")), "lambda0"),
                      (dict(lambda0=float("inf")), "lambda0"), (dict(lambda_end=0.0), "lambda_end"), (dict(lambda_end=7.0), "lambda_end"),
                      (dict(lambda_end=float("nan")), "lambda_end"), (dict(ranks=-1), "ranks"), (dict(ranks=257), "ranks"),
                      (dict(units=0), "units")):
        a = dict(units=10, epochs=3, t=1, lambda0=5.0, lambda_end=0.5, ranks=0)
        a.update(bad)
        with pytest.raises(Exception, match="somhip_debug_ng_schedule: .*" + re.escape(word)):
            E.ng_schedule(**a)


def test_replay_against_the_dense_form():
    """The replay on a 7 x 3 codebook and 40 samples against the dense np.longdouble form, every unit fed by every sample
    with w[rank].  The bound, with u = 2^-53, L = 40 (every unit is ranked by every sample: each chain has L entries),
    A = sum w |x| and q = S / W:  a product rounds once and a chain of L additions from 0 adds at most L - 1 roundings,
    |S~ - S| <= (L + 1) u A (1 + O(L u));  W~ the same without the products, |W~ - W| <= L u W;  the division rounds
    once and |q| <= A / W, so the fp64 quotient is within (2 L + 2) u A / W (1 + O(L u)), stated as (2 L + 6) u A / W;  the
    rounding to float adds ulp32(q) / 2."""
    x, codes = gauss(3, 40, 7, 3)
    lam = 2.0
    w = np.exp(-np.arange(7, dtype=f64) / lam)
    u, dist = R.ranks(codes, x, 7)
    assert sorted(u[0].tolist()) == list(range(7)) and (np.diff(dist.astype(f64), axis=1) >= 0).all()
    hits, S, W = R.sums(u, x, w, 7)
    assert (hits == 40).all()
    rows = R.update(codes, S, W)
    q, Sl, Wl, A = R.dense_longdouble(codes, x, w)
    L = 40
    _, e = np.frexp(np.abs(q).astype(f64))
    ulp32 = np.ldexp(f64(1.0), np.maximum(e - 24, -149))
    bound = ulp32.astype(np.longdouble) / 2 + np.longdouble((2 * L + 6) * 2.0 ** -53) * A / Wl[:, None]
    err = np.abs(rows.astype(np.longdouble) - q)
    assert (err <= bound).all(), (err / bound).max()
    assert (np.abs(S - Sl) <= np.longdouble((L + 2) * 2.0 ** -53) * A).all() and (np.abs(W - Wl) <= np.longdouble(L * 2.0 ** -53) * Wl).all()
    # ties: the later row first, at every K; K == 1 is the first of K == 2
    xt, ct = tied(5, 30, 6)
    u8, _ = R.ranks(ct, xt, 6)
    d = R.distances(ct, xt)
    for s in range(30):
        ds_ = d[s][u8[s]]
        assert (np.diff(ds_) >= 0).all()
        eq = np.nonzero(np.diff(ds_) == 0)[0]
        assert len(eq) and (u8[s][eq] > u8[s][eq + 1]).all()
    assert np.array_equal(R.ranks(ct, xt, 1)[0][:, 0], u8[:, 0])


CLUSTER_SEED = 2


def cluster_start(seed=CLUSTER_SEED):
    """three well-separated Gaussian clusters in dim 4, 600 samples, and 12 units started on samples of the first one"""
    rs = np.random.RandomState(seed)
    cen = np.array([[0, 0, 0, 0], [12, 0, 0, 0], [0, 12, 0, 0]], dtype=f32)
    which = np.arange(600) % 3
    x = (cen[which] + rs.standard_normal((600, 4))).astype(f32)
    start = x[np.nonzero(which == 0)[0][:12]].copy()
    return x, start


def replay_runs(E):
    x, start = cluster_start()
    gas, _ = R.train(start, x, lambda t: E.ng_schedule(12, 20, t), 20)
    kmeans, _ = R.train(start, x, lambda t: E.ng_schedule(12, 20, t, 0.01, 0.01), 20)
    return x, start, gas, kmeans


def final_state(rows, x):
    """(hits at rank 0, the quantization error) of a codebook"""
    u, dist = R.ranks(rows, x, 1)
    return np.bincount(u[:, 0], minlength=rows.shape[0]), float(R.qerror_chain(dist[:, 0]))


def test_replay_neural_gas_beats_kmeans_from_a_bad_start(built):
    """the definition itself, on the CPU: from a start inside one cluster of three, 20 epochs at the default lambda leave
    no dead unit and a lower quantization error than 20 epochs at lambda 0.01 (k-means), which leaves dead units"""
    from som_lvq_pak_amd import engine as E
    x, start, gas, kmeans = replay_runs(E)
    assert E.ng_schedule(12, 20, 0, 0.01, 0.01)[1] == 1
    gh, gq = final_state(gas, x)
    kh, kq = final_state(kmeans, x)
    assert (gh >= 1).all(), gh
    assert (kh == 0).any(), kh
    assert gq < kq, (gq, kq)


def test_bng_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("bng", "-help")
    assert p.returncode == 0 and p.stdout.startswith("bng - ") and all(o in p.stdout for o in ("-epochs", "-lambda", "-lambda_end", "-ranks"))
    cod = tmp_path / "m.cod"
    cod.write_text("2\n0 0\n1 0\n0 1\n1 1\n")
    dat = tmp_path / "d.dat"
    dat.write_text("2\n0.25 0.5\n0.75 0.5\n")
    out = tmp_path / "o.cod"
    for args, word in ((("-epochs", 0), "-epochs"), (("-epochs", -3), "-epochs"), (("-epochs", 2, "-lambda", 0), "-lambda"),
                       (("-epochs", 2, "-lambda", "nan"), "-lambda"), (("-epochs", 2, "-lambda_end", 0), "-lambda_end"),
                       (("-epochs", 2, "-lambda_end", -1), "-lambda_end"), (("-epochs", 2, "-lambda", 1, "-lambda_end", 2), "-lambda_end"),
                       (("-epochs", 2, "-lambda_end", 5), "-lambda_end"), (("-epochs", 2, "-ranks", -1), "-ranks"),
                       (("-epochs", 2, "-ranks", 257), "-ranks")):
        p = run("bng", "-cin", cod, "-din", dat, "-cout", out, *args)
        assert p.returncode == 1 and p.stderr.startswith("bng: " + word), (args, p.stderr)
        assert not out.exists()
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3\n4 5 6\n")
    p = run("bng", "-cin", cod, "-din", dim3, "-cout", out, "-epochs", 2)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    xcod = tmp_path / "x.cod"
    xcod.write_text("2\nx 0\n1 0\n0 1\n1 1\n")
    p = run("bng", "-cin", xcod, "-din", dat, "-cout", out, "-epochs", 2)
    assert p.returncode == 1 and "masked components" in p.stderr
    xdat = tmp_path / "x.dat"
    xdat.write_text("2\nx 0.5\n0.75 0.5\n")
    p = run("bng", "-cin", cod, "-din", xdat, "-cout", out, "-epochs", 2)
    assert p.returncode == 1 and "masked components" in p.stderr
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


def check_ranks(E, eng, codes, x, Ks, windows=None):
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, x)
    for first, n in windows or [(0, x.shape[0])]:
        xs = R.rows_of(x, first, n)
        wu, wd = R.ranks(codes, xs, max(Ks))
        for K in Ks:
            gu, gd = E.ng_ranks(cb, ds, K, first, n)
            assert np.array_equal(gu, wu[:, :K]), (K, first, n, np.argwhere(gu != wu[:, :K])[:8])
            same(gd, wd[:, :K].copy())
    same(cb.download(), codes)                                          # the stage writes no row
    cb.close(); ds.close()


# ---- the ranks, exact
@pytest.mark.gpu
@pytest.mark.parametrize("units", [1, 2, 8, 9, 255, 256, 257, 300, 1030])
def test_ranks_units(E, eng, units):
    """1, 2, 8 and 9 rows (the step from the top-K routes to the wide route), 255 / 256 / 257, 300 and 1030 rows (the cap),
    at K on both sides of every route's width, K beyond the rows included"""
    x, codes = gauss(200 + units, 150, units, 5)
    check_ranks(E, eng, codes, x, sorted({1, 2, 3, 8, 9, min(units + 3, 256), 256 if units > 9 else 12}))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 129])
def test_ranks_dims(E, eng, dim):
    x, codes = gauss(300 + dim, 100, 20, dim)
    check_ranks(E, eng, codes, x, [1, 3, 8, 20])


@pytest.mark.gpu
def test_ranks_sample_counts_and_wrap(E, eng):
    """1, 31 / 32 / 33, 700, a wrapped range and 4095 / 4096 / 4097 samples (the search's chunk), on the top-K routes and the
    wide one"""
    x, codes = gauss(7, 4097, 12, 3)
    check_ranks(E, eng, codes, x, [1, 5, 12], [(0, 1), (4096, 1), (0, 31), (0, 32), (0, 33), (5, 700), (4000, 300), (0, 4095), (0, 4096), (0, 4097),
                                               (3, 4097)])


@pytest.mark.gpu
@pytest.mark.parametrize("units", [2, 6, 12, 300])
def test_ranks_ties_take_the_later_row_first(E, eng, units):
    """duplicated rows and integer-valued data: equal distances at every rank, also at K = 1 on a two-row codebook"""
    x, codes = tied(11 + units, 200, units)
    check_ranks(E, eng, codes, x, sorted({1, 2, 4, 8, min(units, 9), min(units + 1, 256)}))
    if units == 2:
        cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
        assert (E.ng_ranks(cb, ds, 1)[0] == 1).all()                    # both rows are one point: the later row
        cb.close(); ds.close()


def check_sums(E, eng, codes, x, weights, windows=None, segments=(0,), lattice=None):
    cb = E.Codebook(eng, codes, *(lattice or ()))
    ds = E.Dataset(eng, x)
    out = []
    for first, n in windows or [(0, x.shape[0])]:
        xs = R.rows_of(x, first, n)
        for w in weights:
            w = np.asarray(w, dtype=f64)
            K = len(w)
            u, _ = R.ranks(codes, xs, K)
            wh, wS, wW = R.sums(u, xs, w, codes.shape[0])
            for seg in segments:
                gh, gS, gW = E.ng_sums(cb, ds, w, first, n, seg)
                assert np.array_equal(gh, wh), (K, seg, np.nonzero(gh != wh)[0][:8])
                same(gS, wS); same(gW, wW)
                assert int(gh.sum()) == n * min(K, codes.shape[0])
            out.append((wh, wS, wW))
    same(cb.download(), codes)
    cb.close(); ds.close()
    return out


def decaying(K, lam=3.0):
    return np.exp(-np.arange(K, dtype=f64) / lam)


def zero_tail(K):
    w = decaying(K, 1.5)
    w[K // 2:] = 0.0
    return w


# ---- the sums, exact
@pytest.mark.gpu
@pytest.mark.parametrize("units", [1, 5, 65, 300])
def test_sums_units_and_ranks(E, eng, units):
    """K = 1, 3, 8, 9, 64 and 256 on 1, 5, 65 and 300 units: decaying weights, and a table whose tail is exactly 0.0"""
    x, codes = gauss(400 + units, 300, units, 3)
    check_sums(E, eng, codes, x, [decaying(K) for K in (1, 3, 8, 9, 64, 256)] + [zero_tail(8), zero_tail(64)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 64, 65, 129])
def test_sums_dims(E, eng, dim):
    x, codes = gauss(500 + dim, 200, 20, dim)
    check_sums(E, eng, codes, x, [decaying(3), decaying(20, 0.7)], [(0, 200), (150, 100)])


@pytest.mark.gpu
def test_sums_segments_leave_the_same_bits(E, eng):
    """cut at 1 sample, at one chunk of the search, at an uneven size and beyond n: the chains are continued, so every cut
    is the one segment, which is the replay -- also over a run that goes round the data set more than twice"""
    x, codes = gauss(21, 37, 9, 5)
    check_sums(E, eng, codes, x, [decaying(4), decaying(9)], [(0, 37), (30, 20), (5, 100)], segments=(0, 1, 5, 36, 37, 1000))
    x, codes = gauss(22, 9000, 12, 3)
    check_sums(E, eng, codes, x, [decaying(3), decaying(12)], [(0, 9000), (8000, 5000)], segments=(0, 4096, 1234, 8999, 10 ** 6))


@pytest.mark.gpu
def test_sums_ones_at_rank_0_are_the_batch_maps_chains(E, eng):
    """a table of one 1.0 on distinct rows: hits, S and W = hits of somhip_debug_batchmap_sums (1.0 * x is x)"""
    x, codes = gauss(23, 700, 65, 6)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 13, 5)
    ds = E.Dataset(eng, x)
    bh, bS = E.batchmap_sums(cb, ds)
    gh, gS, gW = E.ng_sums(cb, ds, [1.0])
    assert np.array_equal(gh, bh)
    same(gS, bS); same(gW, bh.astype(f64))
    cb.close(); ds.close()
    check_sums(E, eng, codes, x, [np.ones(1), np.ones(7), np.ones(65)])


@pytest.mark.gpu
def test_sums_one_unit_nearest_everything_and_most_units_out(E, eng):
    """every sample nearest one unit; most units outside every list: hits 0, W +0.0 and sums of +0.0"""
    rs = np.random.RandomState(31)
    x = (rs.standard_normal((500, 4)) * 0.1).astype(f32)
    codes = (rs.standard_normal((40, 4)) + 50).astype(f32)
    codes[17] = 0
    codes[3], codes[29] = 5, -5                                         # ranks 1 and 2 go to two units, by sample
    (h, S, W), = check_sums(E, eng, codes, x, [decaying(3)])
    assert h[17] == 500 and set(np.nonzero(h)[0]) == {3, 17, 29}
    out = h == 0
    assert out.sum() == 37 and (bits(W[out]) == 0).all() and (bits(S[out]) == 0).all()
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    gh, gS, gW = E.ng_sums(cb, ds, decaying(3))
    assert (gh[out] == 0).all() and (bits(gW[out]) == 0).all() and (bits(gS[out]) == 0).all()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_sums_twice_the_same_bits(E, eng):
    x, codes = gauss(33, 3000, 70, 9)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    a = E.ng_sums(cb, ds, decaying(70, 9.0))
    E.ng_sums(cb, ds, decaying(2))                                      # (another call in between: nothing of it stays)
    b = E.ng_sums(cb, ds, decaying(70, 9.0))
    for g, w in zip(a, b):
        same(g, w)
    cb.close(); ds.close()


# ---- the update, exact
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(32, 8, 6), (8, 24, 5), (0, 70, 7), (0, 1, 1), (0, 300, 129)])
def test_update_is_one_division_and_one_rounding(E, eng, shape):
    """np.float32(S / W) element by element; rows with W == 0 keep their bits: patch-stored maps (32 x 8, 8 x 24), codebooks
    without a lattice, dims that are no multiple of 4"""
    xdim, ydim, dim = shape
    units = xdim * ydim if xdim else ydim
    rs = np.random.RandomState(40 + units + dim)
    codes = rs.standard_normal((units, dim)).astype(f32)
    S = rs.standard_normal((units, dim)) * 37.0
    W = np.abs(rs.standard_normal(units)) + 1e-3
    W[::3] = 0.0
    if units > 4:
        W[4] = 5e-324                                                   # the smallest weight there is still divides
        S[4] = 1e-320
    hits = (W > 0).astype(np.uint32)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, xdim, ydim) if xdim else E.Codebook(eng, codes)
    E.ng_update(cb, hits, S, W)
    same(cb.download(), R.update(codes, S, W))
    same(cb.download()[::3], codes[::3])
    cb.close()


# ---- whole runs
def schedule_of(E, units, T, **kw):
    return lambda t: E.ng_schedule(units, T, t, **kw)


@pytest.fixture(scope="module")
def small_run():
    return gauss(51, 700, 12, 6)


@pytest.mark.gpu
def test_epochs_in_one_call_or_many_by_hand_and_twice(E, eng, small_run):
    """5 epochs in one call, in five calls, and as the stages chained by hand through the schedule leave the replay's bits
    (K_t goes 12, 12, 5, 1, 1: the wide route, a top-K route, the nearest row); a second run leaves them again"""
    x, codes = small_run
    T = 5
    assert [E.ng_schedule(12, T, t)[1] for t in range(T)] == [12, 12, 5, 1, 1]
    want, wq = R.train(codes, x, schedule_of(E, 12, T), T)
    ds = E.Dataset(eng, x)
    for _ in range(2):
        cb = E.Codebook(eng, codes)
        q = E.ng_train(cb, ds, T)
        same(cb.download(), want); same(q, wq)
        cb.close()
    cb = E.Codebook(eng, codes)
    qs = [E.ng_train(cb, ds, T, start_epoch=t, count=1)[0] for t in range(T)]
    same(cb.download(), want); same(np.array(qs, dtype=f32), wq)
    cb.upload(codes)
    assert E.ng_train(cb, ds, T, start_epoch=0, count=2, qerror=False) is None
    E.ng_train(cb, ds, T, start_epoch=2, count=3, qerror=False)
    same(cb.download(), want)
    cb.upload(codes)
    for t in range(T):
        _, K, w = E.ng_schedule(12, T, t)
        E.ng_update(cb, *E.ng_sums(cb, ds, w))
    same(cb.download(), want)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_runs_over_a_window_and_with_fixed_ranks(E, eng, small_run):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    for kw, first, n in ((dict(ranks=3), 0, 700), (dict(lambda0=2.0, lambda_end=0.5), 650, 120), (dict(ranks=12, lambda0=1.0), 10, 33)):
        cb = E.Codebook(eng, codes)
        q = E.ng_train(cb, ds, 3, first=first, n=n, **kw)
        want, wq = R.train(codes, x, schedule_of(E, 12, 3, **kw), 3, first=first, n=n)
        same(cb.download(), want); same(q, wq)
        cb.close()
    ds.close()


@pytest.mark.gpu
def test_qerror_is_the_qerror_routes_figure(E, eng, small_run):
    """qerror_out[t] is find_qerror's float chain over engine.find_winners' distances of the codebook epoch t started from"""
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    for t in range(4):
        _, diff, _ = E.find_winners(cb, ds)
        want = R.qerror_chain(np.asarray(diff).reshape(-1))
        q = E.ng_train(cb, ds, 4, start_epoch=t, count=1)
        assert bits(q)[0] == bits(np.array([want], dtype=f32))[0], (t, q, want)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_lattice_labels_and_header_play_no_part(E, eng):
    """a lattice codebook and the same rows without a lattice end with the same rows; labels pass through"""
    x, codes = gauss(61, 400, 64, 5)
    ds = E.Dataset(eng, x)
    plain = E.Codebook(eng, codes)
    E.ng_train(plain, ds, 3)
    want = plain.download()
    lab = (np.arange(64) % 5).astype(np.int32)
    for cb in (E.Codebook(eng, codes, HEXA, GAUSSIAN, 8, 8), E.Codebook(eng, codes, RECT, BUBBLE, 16, 4), E.Codebook(eng, codes, labels=lab)):
        E.ng_train(cb, ds, 3)
        same(cb.download(), want)
        cb.close()
    plain.close(); ds.close()


@pytest.mark.gpu
def test_train_closes_an_open_batch_map_state(E, eng, small_run):
    x, _ = small_run
    codes = gauss(62, 1, 30, 6)[1]
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes, HEXA, BUBBLE, 6, 5)
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds, 0, 100)
    E.ng_train(cb, ds, 1)
    with pytest.raises(Exception, match="no accumulation is open"):
        E.batchmap_accumulate(cb, ds, 100, 100)
    E.batchmap_end(cb)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_stage_timing_counts_launches(E, eng, small_run):
    x, codes = small_run
    ds, cb = E.Dataset(eng, x), E.Codebook(eng, codes)
    eng.timing(True)
    eng.timing_reset()
    E.ng_train(cb, ds, 2, qerror=False)
    t = eng.ng_timing()
    eng.timing(False)
    assert t["k_ng_sums"][0] == 2 and t["k_ng_update"][0] == 2 and t["group"][0] == 6      # (entries, scan, sort)
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_touch_nothing(E, eng, small_run):
    x, codes = small_run
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, codes)
    mask = np.zeros(x.shape, dtype=np.uint8)
    mask[3, 2] = 1
    masked = E.Dataset(eng, x, mask=mask)
    shard = E.Codebook(eng, codes[:6], row_offset=3, n_global=12)
    other = E.Dataset(eng, x[:, :5])

    def refused(fn, who, word):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(who + ":") and word in str(ei.value), str(ei.value)

    who = "somhip_ng_train"
    refused(lambda: E.ng_train(cb, masked, 3), who, "masked components")
    refused(lambda: E.ng_train(shard, ds, 3), who, "sharded")
    refused(lambda: E.ng_train(cb, other, 3), who, "dimension")
    refused(lambda: E.ng_train(cb, ds, 3, n=2 ** 32), who, "32-bit")
    refused(lambda: E.ng_train(cb, ds, 3, n=0), who, "n 0")
    refused(lambda: E.ng_train(cb, ds, 3, n=-5), who, "n -5")
    refused(lambda: E.ng_train(cb, ds, 3, first=-1), who, "first row")
    refused(lambda: E.ng_train(cb, ds, 0, count=0), who, "epochs 0")
    refused(lambda: E.ng_train(cb, ds, 3, lambda0=0.0), who, "lambda0")
    refused(lambda: E.ng_train(cb, ds, 3, lambda0=float("nan")), who, "lambda0")
    refused(lambda: E.ng_train(cb, ds, 3, lambda_end=0.0), who, "lambda_end")
    refused(lambda: E.ng_train(cb, ds, 3, lambda0=1.0, lambda_end=2.0), who, "lambda_end")
    refused(lambda: E.ng_train(cb, ds, 3, ranks=-1), who, "ranks")
    refused(lambda: E.ng_train(cb, ds, 3, ranks=257), who, "ranks")
    refused(lambda: E.ng_train(cb, ds, 3, start_epoch=-1, count=1), who, "outside")
    refused(lambda: E.ng_train(cb, ds, 3, start_epoch=2, count=2), who, "outside")
    refused(lambda: E.ng_train(cb, ds, 3, start_epoch=3, count=1), who, "outside")
    who = "somhip_debug_ng_ranks"
    refused(lambda: E.ng_ranks(cb, masked, 3), who, "masked components")
    refused(lambda: E.ng_ranks(shard, ds, 3), who, "sharded")
    refused(lambda: E.ng_ranks(cb, ds, 0), who, "ranks")
    refused(lambda: E.ng_ranks(cb, ds, 257), who, "ranks")
    who = "somhip_debug_ng_sums"
    refused(lambda: E.ng_sums(cb, masked, [1.0]), who, "masked components")
    refused(lambda: E.ng_sums(shard, ds, [1.0]), who, "sharded")
    refused(lambda: E.ng_sums(cb, other, [1.0]), who, "dimension")
    refused(lambda: E.ng_sums(cb, ds, [1.0], 0, 0), who, "n 0")
    refused(lambda: E.ng_sums(cb, ds, np.ones(257)), who, "ranks")
    refused(lambda: E.ng_update(shard, np.ones(6, dtype=np.uint32), np.ones((6, 6)), np.ones(6)), "somhip_debug_ng_update", "sharded")
    for c, rows in ((cb, codes), (shard, codes[:6])):
        same(c.download(), rows)
    for o in (cb, shard, ds, masked, other):
        o.close()


# ---- what it is for
@pytest.mark.gpu
def test_neural_gas_beats_kmeans_from_a_bad_start(E, eng):
    """the clusters of test_replay_neural_gas_beats_kmeans_from_a_bad_start: the GPU shows the replay's bits for both runs,
    so no unit is dead after neural gas, some are after k-means, and neural gas ends with the lower quantization error"""
    x, start, gas, kmeans = replay_runs(E)
    ds = E.Dataset(eng, x)
    cb = E.Codebook(eng, start)
    E.ng_train(cb, ds, 20, qerror=False)
    same(cb.download(), gas)
    gq = E.ng_train(cb, ds, 1, 0.01, 0.01)[0]                           # (the q of the codebook the epoch starts from)
    cb.upload(start)
    E.ng_train(cb, ds, 20, 0.01, 0.01, qerror=False)
    same(cb.download(), kmeans)
    kq = E.ng_train(cb, ds, 1, 0.01, 0.01)[0]
    gh, wgq = final_state(gas, x)
    kh, wkq = final_state(kmeans, x)
    assert float(gq) == wgq and float(kq) == wkq
    assert (gh >= 1).all() and (kh == 0).any() and gq < kq
    cb.close(); ds.close()


# ---- the tool
def v_lines(E, units, T, q, n, **kw):
    out = []
    for t in range(T):
        lam, K, _ = E.ng_schedule(units, T, t, **kw)
        out.append("epoch %d lambda %.17g ranks %d qerror %f" % (t, lam, K, float(f32(q[t]) / f32(n))))
    return out


@pytest.mark.gpu
def test_bng_writes_the_engines_codebook(E, eng, tools, tmp_path):
    from som_lvq_pak_amd import textio
    rs = np.random.RandomState(71)
    x = (np.round(rs.standard_normal((700, 4)) * 16) / 16).astype(f32)              # values that "%g" keeps
    codes = (np.round(rs.standard_normal((30, 4)) * 16) / 16).astype(f32)
    dat, cod, out = tmp_path / "d.dat", tmp_path / "m.cod", tmp_path / "o.cod"
    d = textio.Entries()
    d.dim, d.points = 4, x
    textio.write_entries(str(dat), d)
    tab = textio.LabelTable()
    m = textio.Entries()
    m.dim, m.topol, m.neigh, m.xdim, m.ydim, m.points = 4, HEXA, GAUSSIAN, 6, 5, codes
    m.labels = [[tab.to_index("u%d" % (i % 4))] if i % 3 else [] for i in range(30)]
    textio.write_entries(str(cod), m, tab)

    p = run("bng", "-cin", cod, "-din", dat, "-cout", out, "-epochs", 4, "-v")
    assert p.returncode == 0, p.stderr
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, x)
    q = E.ng_train(cb, ds, 4)
    rows = cb.download()
    tab2 = textio.LabelTable()
    got = textio.read_entries(str(out), tab2)[0]
    assert (got.dim, got.topol, got.neigh, got.xdim, got.ydim) == (4, HEXA, GAUSSIAN, 6, 5)          # the header it read
    assert [[tab2.names[l] for l in ls] for ls in got.labels] == [[tab.names[l] for l in ls] for ls in m.labels]
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in rows], dtype=f32)
    same(got.points, printed)
    assert p.stdout.strip().split("\n") == v_lines(E, 30, 4, q, 700)
    # options reach the engine; without -v: no lines, the same file; a raw fp32 copy of the data: the same file
    out2 = tmp_path / "o2.cod"
    p = run("bng", "-cin", cod, "-din", dat, "-cout", out2, "-epochs", 3, "-lambda", 4, "-lambda_end", 0.5, "-ranks", 9, "-v")
    cb.upload(codes)
    q = E.ng_train(cb, ds, 3, 4.0, 0.5, 9)
    assert p.returncode == 0 and p.stdout.strip().split("\n") == v_lines(E, 30, 3, q, 700, lambda0=4.0, lambda_end=0.5, ranks=9)
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)
    same(textio.read_entries(str(out2))[0].points, printed)
    out3, raw, out4 = tmp_path / "o3.cod", tmp_path / "d.f32", tmp_path / "o4.cod"
    p = run("bng", "-cin", cod, "-din", dat, "-cout", out3, "-epochs", 4)
    assert p.returncode == 0 and p.stdout == "" and out3.read_bytes() == out.read_bytes()
    assert run("datconv", "-din", dat, "-dout", raw).returncode == 0
    p = run("bng", "-cin", cod, "-din", raw, "-cout", out4, "-epochs", 4)
    assert p.returncode == 0 and out4.read_bytes() == out.read_bytes()
    # T epochs, then the qerror tool on the result: the figure a further one-epoch run prints first
    p = run("qerror", "-cin", out, "-din", dat)
    assert p.returncode == 0, p.stderr
    nxt = run("bng", "-cin", out, "-din", dat, "-cout", tmp_path / "o5.cod", "-epochs", 1, "-v")
    figure = re.search(r" is (\d+\.\d{6}) per sample \(700 samples\)", p.stdout)
    assert figure and nxt.returncode == 0 and nxt.stdout.strip().split("\n")[0].split(" qerror ")[1] == figure.group(1)
    cb.close(); ds.close()
    # a gen: source
    gen = E.Dataset(eng, generate=(5, 3, 4, 0, 500))
    cb = E.Codebook(eng, codes)
    q = E.ng_train(cb, gen, 2)
    out6 = tmp_path / "o6.cod"
    p = run("bng", "-cin", cod, "-din", "gen:k=3,dim=4,n=500,seed=5", "-cout", out6, "-epochs", 2, "-v")
    assert p.returncode == 0 and p.stdout.strip().split("\n") == v_lines(E, 30, 2, q, 500)
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)
    same(textio.read_entries(str(out6))[0].points, printed)
    cb.close(); gen.close()
