"""Batch Robust Soft LVQ (K13: somhip_rslvq_train, somhip_rslvq_search and the stage entries, engine.rslvq_*, the rslvq
tool) against the numpy replay in rslvq_replay.py.

The correct flags are compared exactly.  The posteriors' coefficients, the cost and P(y | x) pass through exp and log,
which differ by an ulp between the device's library and the C library's, so they are held to the bounds DESIGN.md K13
derives from that (rslvq_replay.posterior_bounds), and to the invariants that follow from the definition.  The sums are
held to K8's combine bound against np.longdouble and must not depend on the chunk; the update, every operation of which
is one IEEE rounding, equals its float64 replay bit for bit and meets the np.longdouble allowance."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rslvq_replay as R
from conftest import ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
f32, f64 = np.float32, np.float64

# the overlapping classes of the whole-run tests, and the rates the replay itself needs on them (found on the CPU:
# test_replay_cost_falls_every_epoch)
GAUSS = dict(seed=5, n=1500, protos=12, dim=8, classes=3, sep=0.8)
GAUSS_ALPHA, GAUSS_SIGMA2, GAUSS_EPOCHS = 5.0, 1.0, 8


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("rslvq", "accuracy")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def clusters(seed, n, protos, dim, classes=3, sep=2.0):
    """Gaussian clusters of unit variance, one per class, and prototypes scattered near the shrunken centres"""
    rs = np.random.RandomState(seed)
    cen = (sep * rs.standard_normal((classes, dim))).astype(f32)
    dl = (np.arange(n) % classes).astype(np.int32)
    x = (cen[dl] + rs.standard_normal((n, dim))).astype(f32)
    cl = (np.arange(protos) % classes).astype(np.int32)
    c = (cen[cl] * 0.3 + rs.standard_normal((protos, dim))).astype(f32)
    return x, dl, c, cl


def bits32(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=f64).view(np.uint64)


def write_dat(path, x, labels, names):
    with open(path, "w") as fh:
        fh.write("%d\n" % x.shape[1])
        for row, l in zip(x, labels):
            fh.write(" ".join(repr(float(v)) for v in row) + " " + names[int(l)] + "\n")


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.RSLVQ_SIGNATURES
    for name in ("somhip_rslvq_train", "somhip_rslvq_search", "somhip_debug_rslvq_chunk", "somhip_debug_rslvq_posterior",
                 "somhip_debug_rslvq_sums", "somhip_debug_rslvq_update", "somhip_rslvq_timing"):
        assert hasattr(lib, name) and name in S, name
    assert S["somhip_rslvq_train"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.RslvqParams), _lib.c_double_p, _lib.c_i64_p])
    assert S["somhip_rslvq_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.RslvqParams._fields_] == ["epochs", "start_epoch", "count", "first", "n", "alpha", "sigma2"]
    assert C.sizeof(_lib.RslvqParams) == 48
    for name in ("rslvq_train", "rslvq_search", "rslvq_posterior", "rslvq_sums", "rslvq_update", "rslvq_chunk"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "rslvq_timing")


def test_header_declares_the_entry_points():
    assert re.search(r'^#include "somhip_rslvq.h"$', open(os.path.join(ROOT, "include", "somhip.h")).read(), flags=re.M)
    hdr = open(os.path.join(ROOT, "include", "somhip_rslvq.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int somhip_rslvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_rslvq_params *p, double *cost_out , "
            "int64_t *correct_out );") in hdr
    assert ("int somhip_rslvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, double *cost, "
            "int64_t *correct, double *pown );") in hdr
    assert "int somhip_rslvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]);" in hdr
    m = re.search(r"typedef struct somhip_rslvq_params \{(.*?)\} somhip_rslvq_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int64_t epochs; int64_t start_epoch, count; int64_t first, n; float alpha; "
                                                            "float sigma2;")


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 4)(), (C.c_double * 4)()
    assert lib.somhip_rslvq_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_rslvq_timing: null engine"


def test_chunk_rule_is_host_arithmetic(built):
    """min(4096, the largest multiple of 64 whose [chunk][ld] doubles fit 256 MiB), 64 at least; ld = 64 * row groups"""
    from som_lvq_pak_amd import engine as E
    assert E.rslvq_chunk(30) == (4096, 64) and E.rslvq_chunk(64) == (4096, 64) and E.rslvq_chunk(65) == (4096, 128)
    assert E.rslvq_chunk(1000) == (4096, 1024)
    assert E.rslvq_chunk(8192) == (4096, 8192) and E.rslvq_chunk(8193) == (4032, 8256)     # the first codebook that shortens it
    assert E.rslvq_chunk(10000) == ((256 << 20) // (8 * 10048) // 64 * 64, 10048) == (3328, 10048)
    assert E.rslvq_chunk(600000)[0] == 64 and E.rslvq_chunk(5000000)[0] == 64              # never below one sample tile
    with pytest.raises(Exception, match="somhip_debug_rslvq_chunk"):
        E.rslvq_chunk(0)


def test_replay_cost_falls_every_epoch():
    """the definition itself, on the CPU, on three overlapping Gaussian classes: the cost falls in every epoch and the
    accuracy ends above its start -- the alpha and sigma2 the GPU test takes"""
    x, dl, c, cl = clusters(**GAUSS)
    rows, cost, correct = R.train(c, cl, x, dl, GAUSS_EPOCHS, GAUSS_ALPHA, GAUSS_SIGMA2)
    after = R.epoch(rows, cl, x, dl, 0.0, GAUSS_SIGMA2)
    assert (np.diff(np.append(cost, after[1])) < 0).all(), (cost, after[1])
    assert after[2] > correct[0] and 0.5 < after[2] / GAUSS["n"] < 0.95                     # overlapping: far from separable


def test_replay_meets_its_own_invariants():
    x, dl, c, cl = clusters(3, 90, 7, 5, sep=1.0)
    p = R.posterior(c, cl, x, dl, 2.0)
    bq, bc, bp, bs = R.posterior_bounds(p)
    assert (np.abs([math.fsum(r) for r in p["q"]]) <= bs).all() and (p["q"][~p["own"]] <= 0).all() and (p["cost"] >= -bc).all()
    G, c64, bG, bcc = R.sums_longdouble(p["q"], x)
    Gm, cm = R.sums_mfma(p["q"], x)
    assert (np.abs(Gm - G) <= bG).all() and (np.abs(cm - c64) <= bcc).all()


def test_rslvq_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("rslvq", "-help")
    assert p.returncode == 0 and p.stdout.startswith("rslvq - ") and all(w in p.stdout for w in ("-epochs", "-alpha", "-sigma2", "-pout"))
    cod, dat, out = tmp_path / "c.cod", tmp_path / "d.dat", tmp_path / "o.cod"
    cod.write_text("2\n0 0 a\n1 1 b\n")
    dat.write_text("2\n0.25 0.5 a\n0.75 0.5 b\n")
    for args, word in ((("-epochs", -2, "-alpha", 1, "-sigma2", 1), "-epochs"), (("-epochs", 2, "-alpha", -1, "-sigma2", 1), "-alpha"),
                       (("-epochs", 2, "-alpha", "nan", "-sigma2", 1), "-alpha"), (("-epochs", 2, "-alpha", 1, "-sigma2", 0), "-sigma2"),
                       (("-epochs", 2, "-alpha", 1, "-sigma2", -1), "-sigma2"), (("-epochs", 2, "-alpha", 1, "-sigma2", "nan"), "-sigma2"),
                       (("-epochs", 2, "-alpha", 1, "-sigma2", "inf"), "-sigma2"), (("-epochs", 0, "-sigma2", 0), "-sigma2")):
        p = run("rslvq", "-cin", cod, "-din", dat, "-cout", out, *args)
        assert p.returncode == 1 and p.stderr.startswith("rslvq: " + word), (args, p.stderr)
    good = ("-epochs", 2, "-alpha", 1, "-sigma2", 1)
    for missing in ("-cin", "-din", "-cout", "-epochs", "-alpha", "-sigma2"):                 # a missing option
        args = {"-cin": cod, "-din": dat, "-cout": out, "-epochs": 2, "-alpha": 1, "-sigma2": 1}
        del args[missing]
        p = run("rslvq", *[v for kv in args.items() for v in kv])
        assert p.returncode != 0 and missing[1:] in (p.stderr + p.stdout), (missing, p.stderr)
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3 a\n4 5 6 b\n")
    p = run("rslvq", "-cin", cod, "-din", dim3, "-cout", out, *good)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    for name, text, word in (("x.cod", "2\nx 0 a\n1 1 b\n", "masked components"), ("x.dat", "2\nx 0.5 a\n0.75 0.5 b\n", "masked components"),
                             ("n.cod", "2\n0 0\n1 1\n", "no labels"), ("n.dat", "2\n0.25 0.5\n0.75 0.5\n", "no labels"),
                             ("one.cod", "2\n0 0 a\n1 1 a\n", "one label"), ("z.dat", "2\n0.25 0.5 a\n0.75 0.5 z\n", "no codebook row")):
        f = tmp_path / name
        f.write_text(text)
        p = run("rslvq", "-cin", f if name.endswith(".cod") else cod, "-din", f if name.endswith(".dat") else dat, "-cout", out, *good)
        assert p.returncode == 1 and p.stderr.startswith("rslvq: ") and word in p.stderr, (name, p.stderr)
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


def edge_case(seed, rows, dim, n_data, classes):
    """A labelled codebook and data set with the edges the posteriors have to get right: a class of a single row (q = 1 - P
    on it), a class that lies wholly behind the last full group of 64 rows, duplicated rows within a class and across two
    classes, and samples equal to a prototype"""
    rs = np.random.RandomState(seed)
    c = rs.standard_normal((rows, dim)).astype(f32)
    cl = rs.randint(0, max(classes - 2, 1), size=rows).astype(np.int32)
    tail = (rows - 1) // 64 * 64 if rows > 64 else rows - 1
    cl[tail:] = classes - 1                                        # the last class: only behind the last full group
    if classes > 2:
        cl[rows // 3] = classes - 2                                # a class with a single row
    x = (rs.standard_normal((n_data, dim)) * 1.5).astype(f32)
    dl = cl[rs.randint(0, rows, size=n_data)].astype(np.int32)
    if n_data > 1:
        dl[1] = classes - 2 if classes > 2 else classes - 1        # a sample of the single-row class
    if rows >= 8:
        a, b = 1, rows // 2
        if b != rows // 3 and a != rows // 3:
            c[b] = c[a]; cl[b] = cl[a]                              # duplicates within a class
        diff = np.flatnonzero(cl != cl[a])
        c[diff[-1]] = c[a]                                          # ... and across two classes
        if n_data > 3:
            x[0] = c[a]; dl[0] = cl[a]                              # a sample equal to prototypes of two classes
            x[2] = c[rows - 2]; dl[2] = cl[rows - 2]                # ... and to one prototype
    assert len(set(cl.tolist())) >= 2 and set(dl.tolist()) <= set(cl.tolist())
    return c, cl, x, dl


WORST = {}


def check_posterior(E, eng, c, cl, x, dl, sigma2, first, n, tag, cb=None):
    """cb: the caller's codebook of the rows c and labels cl (a map stored in patches, say), left open; else one without a
    lattice is made here"""
    mine = cb is None
    cb, ds = E.Codebook(eng, c, labels=cl) if mine else cb, E.Dataset(eng, x, labels=dl)
    rows = c.shape[0]
    got = E.rslvq_posterior(cb, ds, sigma2, first, n, chunk=64)
    again = E.rslvq_posterior(cb, ds, sigma2, first, n, chunk=64)
    whole = E.rslvq_posterior(cb, ds, sigma2, first, n)             # the rule's chunk: a sample's figures do not know the chunk
    for key in ("q", "cost", "pown"):
        assert (bits64(got[key]) == bits64(again[key])).all() and (bits64(got[key]) == bits64(whole[key])).all(), (tag, key)
    assert (got["correct"] == again["correct"]).all() and (got["correct"] == whole["correct"]).all()
    assert got["q"].shape == (n, (rows + 63) // 64 * 64) and (bits64(got["q"][:, rows:]) == 0).all(), tag     # the padding: +0.0
    p = R.posterior(c, cl, x, dl, sigma2, first, n)
    bq, bc, bp, bs = R.posterior_bounds(p)
    assert (got["correct"] == p["correct"]).all(), (tag, np.flatnonzero(got["correct"] != p["correct"])[:5])
    q = got["q"][:, :rows]
    worst = {}
    for name, err, tol in (("q", np.abs(q - p["q"]), bq), ("cost", np.abs(got["cost"] - p["cost"]), bc),
                           ("pown", np.abs(got["pown"] - p["pown"]), bp)):
        worst[name] = float((err / tol).max())
        assert (err <= tol).all(), (tag, name, worst)
    sums = np.array([math.fsum(r) for r in q])
    worst["sum_q"] = float((np.abs(sums) / bs).max())
    assert (np.abs(sums) <= bs).all(), (tag, worst)
    assert (q[~p["own"]] <= 0).all() and (got["cost"] >= -bc).all(), tag
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("rslvq posterior", tag, "largest difference / bound:", worst, "so far:", WORST)
    ds.close()
    if mine:
        cb.close()
    return got, p


# rows x dim x samples x classes: every row count, dimension and run length the issue names, run lengths 65 / 130 / 200
# crossing one, two and three edges of the 64-sample chunk; 321 and 1030 rows are 6 and 17 row groups without a lattice,
# the last of 1 and of 6 rows: k_knn_dist's last grid.y block (four groups a block) holds two live groups and one
POSTERIOR_SHAPES = [(2, 1, 1, 2), (3, 3, 3, 3), (63, 63, 4, 3), (64, 64, 5, 4), (65, 65, 63, 5), (130, 129, 64, 7), (130, 3, 65, 2),
                    (65, 64, 130, 6), (130, 16, 200, 7), (3, 129, 200, 2), (321, 5, 70, 6), (1030, 3, 65, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,classes", POSTERIOR_SHAPES)
def test_posterior_within_the_derived_bounds(E, eng, rows, dim, n, classes):
    """a width that leaves every posterior alive; a plain range, one that wraps once and (200 samples of 90 rows) twice"""
    n_data = 90 if n == 200 else max(n, 5)
    c, cl, x, dl = edge_case(2000 + rows + dim, rows, dim, n_data, classes)
    sigma2 = float(dim)
    check_posterior(E, eng, c, cl, x, dl, sigma2, 0, n, (rows, dim, n, "plain"))
    check_posterior(E, eng, c, cl, x, dl, sigma2, n_data - 2, n, (rows, dim, n, "wrapped"))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,classes", [(65, 5, 65, 5), (130, 64, 5, 7)])
def test_posterior_at_the_ends_of_sigma2(E, eng, rows, dim, n, classes):
    """sigma2 so small that every posterior but the nearest rows' underflows to zero, and so large that they are uniform"""
    c, cl, x, dl = edge_case(2100 + rows, rows, dim, max(n, 5), classes)
    check_the_ends_of_sigma2(E, eng, c, cl, x, dl, n, (rows, dim, n))


def check_the_ends_of_sigma2(E, eng, c, cl, x, dl, n, tag, cb=None):
    """(the posteriors at sigma2 = 1e-30, the replay's) after the assertions of both ends"""
    rows = c.shape[0]
    tiny = got, p = check_posterior(E, eng, c, cl, x, dl, 1e-30, 0, n, tag + ("tiny",), cb)
    d = p["d"]
    nearest = d == d.min(axis=1, keepdims=True)
    assert (got["q"][:, :rows][~nearest & ~p["own"]] == 0).all()                    # underflowed, not merely small
    lost = ~(nearest & p["own"]).any(axis=1)                                        # no own-label row among the nearest
    assert (got["pown"][lost] == 0).all() and (got["correct"][lost] == 0).all()
    got, p = check_posterior(E, eng, c, cl, x, dl, 1e30, 0, n, tag + ("huge",), cb)
    n_own = p["own"].sum(axis=1)
    assert np.allclose(got["pown"], n_own / rows, rtol=1e-12) and np.allclose(got["q"][:, :rows][~p["own"]], -1.0 / rows, rtol=1e-12)
    return tiny


@pytest.mark.gpu
def test_posterior_far_from_the_origin_and_equidistant(E, eng):
    """data and rows near 1000 in every component (the distances keep few bits of the differences); then rows that are all
    at one distance from every sample: the posteriors are the class sizes' shares, whatever the width"""
    c, cl, x, dl = edge_case(77, 65, 16, 70, 4)
    check_posterior(E, eng, c + f32(1000.0), cl, x + f32(1000.0), dl, 8.0, 3, 70, "far")
    rows, dim = 6, 6
    c = np.eye(rows, dim, dtype=f32)
    cl = np.array([0, 0, 0, 1, 1, 2], dtype=np.int32)
    x = np.zeros((7, dim), dtype=f32)
    dl = (np.arange(7) % 3).astype(np.int32)
    for sigma2 in (0.01, 1.0, 100.0):
        got, p = check_posterior(E, eng, c, cl, x, dl, sigma2, 0, 7, ("equidistant", sigma2))
        share = np.array([3, 2, 1], dtype=f64)[dl] / rows
        assert np.allclose(got["pown"], share, rtol=1e-14) and np.allclose(got["cost"], -np.log(share), rtol=1e-14)
        assert (got["correct"] == (dl == 0)).all()                                   # row 0 is the lowest of the equal keys


def random_q(seed, n, rows):
    rs = np.random.RandomState(seed)
    q = rs.standard_normal((n, rows)) * np.exp(rs.uniform(-6, 2, size=(n, rows)))    # mixed signs and magnitudes
    q[rs.rand(n, rows) < 0.1] = 0.0
    return q


SUMS_SHAPES = [(2, 1, 1), (3, 3, 5), (63, 63, 63), (64, 64, 64), (65, 65, 65), (130, 129, 200), (130, 64, 4), (65, 3, 3), (2, 130, 130),
               (321, 5, 130)]                                                         # six workgroups along grid.x, the last of one row


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n", SUMS_SHAPES)
def test_sums_meet_the_combine_bound_and_do_not_know_the_chunk(E, eng, rows, dim, n):
    """[G | c] on a caller's Q of mixed signs against np.longdouble within (2 n + 16) 2^-52 sum |q| |x|; the definition
    orders the additions by the sample's number in the run alone, so chunk 64 and chunk 4096 give the same bits; so
    does a second run; a plain range and a wrapped one"""
    rs = np.random.RandomState(rows * 131 + dim)
    n_data = 90 if n == 200 else max(n, 5)
    x = (rs.standard_normal((n_data, dim)) * 3).astype(f32)
    c = rs.standard_normal((rows, dim)).astype(f32)
    cl, dl = (np.arange(rows) % 2).astype(np.int32), (np.arange(n_data) % 2).astype(np.int32)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    q = random_q(rows + n, n, rows)
    for first in (0, n_data - 2):
        G, cc = E.rslvq_sums(cb, ds, q, first, n, chunk=64)
        G2, cc2 = E.rslvq_sums(cb, ds, q, first, n, chunk=64)
        G3, cc3 = E.rslvq_sums(cb, ds, q, first, n, chunk=4096)
        assert (bits64(G) == bits64(G2)).all() and (bits64(cc) == bits64(cc2)).all()
        assert (bits64(G) == bits64(G3)).all() and (bits64(cc) == bits64(cc3)).all()
        wG, wc, bG, bc = R.sums_longdouble(q, x, first)
        eG, ec = np.abs(G - wG).astype(f64), np.abs(cc - wc).astype(f64)
        print("rslvq sums", (rows, dim, n, first), "largest difference / bound:", float((eG / bG).max()), float((ec / bc).max()))
        assert (eG <= bG).all() and (ec <= bc).all(), (float((eG / bG).max()), float((ec / bc).max()))
    qp = np.full((n, (rows + 63) // 64 * 64), 1e300)                                  # the columns behind the last row reach no result
    qp[:, :rows] = q
    G4, cc4 = E.rslvq_sums(cb, ds, qp, n_data - 2, n, chunk=64)
    assert (bits64(G4) == bits64(G)).all() and (bits64(cc4) == bits64(cc)).all()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(2, 1), (63, 3), (64, 63), (65, 64), (130, 65), (3, 129)])
def test_update_equals_the_replay(E, eng, rows, dim):
    """every operation of step 5 is one IEEE rounding: the rows equal the float64 replay bit for bit, and lie within
    ulp32 / 2 plus the float64 roundings of the np.longdouble result; every row is stepped"""
    rs = np.random.RandomState(rows + 7 * dim)
    c = (rs.standard_normal((rows, dim)) * 2).astype(f32)
    cl = (np.arange(rows) % 2).astype(np.int32)
    G, cc = rs.standard_normal((rows, dim)) * 30, rs.standard_normal(rows) * 10
    alpha_t, sigma2, n = R.alpha_at(7.5, 9, 2), 0.7, 123
    cb = E.Codebook(eng, c, labels=cl)
    E.rslvq_update(cb, alpha_t, sigma2, n, G, cc)
    after = cb.download()
    assert (bits32(after) == bits32(R.update(c, G, cc, alpha_t, sigma2, n))).all()
    q, bound = R.update_longdouble(c, G, cc, alpha_t, sigma2, n)
    err = np.abs(after.astype(np.longdouble) - q)
    assert (err <= bound).all(), float((err / bound).max())
    assert (bits32(after) != bits32(c)).any(axis=1).all()
    cb.close()


def stage_epoch(E, cb, ds, alpha_t, sigma2, first, n, chunk=0):
    p = E.rslvq_posterior(cb, ds, sigma2, first, n, chunk)
    G, c = E.rslvq_sums(cb, ds, p["q"], first, n, chunk)
    chain = f64(0.0)
    for v in p["cost"]:
        chain = chain + v
    E.rslvq_update(cb, alpha_t, sigma2, n, G, c)
    return chain / f64(n), int(p["correct"].sum())


@pytest.mark.gpu
def test_runs(E, eng):
    """5 epochs in one call equal five calls and equal themselves run twice; an epoch equals its stages, at the rule's chunk
    and at chunk 64 (390 samples: six chunk edges); the figures follow the replay; rslvq_search after training gives the
    figures an epoch would report of those rows"""
    x, dl, c, cl = clusters(9, 400, 12, 16, sep=1.0)
    first, n, T, alpha, sigma2 = 7, 390, 5, 10.0, 4.0
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    cost, correct = E.rslvq_train(cb, ds, T, alpha, sigma2, first=first, n=n)
    one = cb.download()
    cb.upload(c)
    cost2, correct2 = E.rslvq_train(cb, ds, T, alpha, sigma2, first=first, n=n)
    assert (bits32(cb.download()) == bits32(one)).all() and (bits64(cost2) == bits64(cost)).all() and (correct2 == correct).all()
    cb.upload(c)
    for t in range(T):
        ct, rt = E.rslvq_train(cb, ds, T, alpha, sigma2, start_epoch=t, count=1, first=first, n=n)
        assert bits64(ct)[0] == bits64(cost)[t] and rt[0] == correct[t]
    assert (bits32(cb.download()) == bits32(one)).all()
    for chunk in (0, 64):
        cb.upload(c)
        for t in range(T):                                               # an epoch is its stages
            ct, rt = stage_epoch(E, cb, ds, E.glvq_alpha(alpha, T, t), sigma2, first, n, chunk)
            assert bits64(ct)[()] == bits64(cost)[t] and rt == correct[t], (chunk, t)
        assert (bits32(cb.download()) == bits32(one)).all(), chunk
    scost, scorrect, spown = E.rslvq_search(cb, ds, sigma2, first, n)
    p = E.rslvq_posterior(cb, ds, sigma2, first, n)
    assert (bits64(spown) == bits64(p["pown"])).all() and scorrect == int(p["correct"].sum())
    ct, rt = E.rslvq_train(cb, ds, T, 0.0, sigma2, start_epoch=0, count=1, first=first, n=n)   # alpha 0: the figures, no step
    assert bits64(scost) == bits64(ct)[0] and scorrect == rt[0] and (bits32(cb.download()) == bits32(one)).all()
    assert E.rslvq_search(cb, ds, sigma2, first, n, pown=False)[2] is None
    rows, rcost, rcorrect = R.train(c, cl, x, dl, T, alpha, sigma2, first, n)
    assert np.allclose(one, rows, rtol=0, atol=1e-5) and np.allclose(cost, rcost, rtol=1e-9, atol=0) and (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_cost_falls_every_epoch_on_overlapping_classes(E, eng):
    """three overlapping Gaussian classes, the alpha and sigma2 the replay needs (test_replay_cost_falls_every_epoch): the
    cost falls in every epoch, the accuracy ends above its start, and the search afterwards reports the state it left"""
    x, dl, c, cl = clusters(**GAUSS)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.rslvq_train(cb, ds, GAUSS_EPOCHS, GAUSS_ALPHA, GAUSS_SIGMA2)
    after, right, pown = E.rslvq_search(cb, ds, GAUSS_SIGMA2)
    assert (np.diff(np.append(cost, after)) < 0).all() and right > correct[0], (cost, after, correct, right)
    assert np.isclose(-np.log(pown).mean(), after, rtol=1e-12)
    rows, rcost, rcorrect = R.train(c, cl, x, dl, GAUSS_EPOCHS, GAUSS_ALPHA, GAUSS_SIGMA2)
    assert np.allclose(cost, rcost, rtol=1e-9, atol=0) and np.abs(correct - rcorrect).max() <= 2      # (a sample on a boundary may flip)
    assert np.allclose(cb.download(), rows, rtol=0, atol=1e-5)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_leave_the_rows(E, eng):
    x, dl, c, cl = clusters(3, 50, 6, 4)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    mask = np.zeros(x.shape, dtype=np.uint8); mask[3, 1] = 1
    cases = [
        (E.Codebook(eng, c), ds, {}, "no labels"),
        (cb, E.Dataset(eng, x), {}, "no labels"),
        (cb, E.Dataset(eng, x, mask=mask, labels=dl), {}, "masked components"),
        (E.Codebook(eng, c[:3], labels=cl[:3], row_offset=0, n_global=6), ds, {}, "sharded"),
        (cb, E.Dataset(eng, x[:, :3], labels=dl), {}, "dimension"),
        (cb, E.Dataset(eng, x, labels=dl + 1), {}, "no row of the codebook carries"),
        (E.Codebook(eng, c, labels=np.zeros(6, dtype=np.int32)), E.Dataset(eng, x, labels=np.zeros(50, dtype=np.int32)), {}, "every row of the codebook carries"),
        (cb, ds, dict(n=0), "n 0 <= 0"), (cb, ds, dict(n=1 << 32), "32-bit"), (cb, ds, dict(first=-1), "first row -1 < 0"),
        (cb, ds, dict(epochs=0), "epochs 0 < 1"), (cb, ds, dict(start_epoch=3, count=3), "outside [0, 5)"), (cb, ds, dict(start_epoch=-1, count=1), "outside"),
        (cb, ds, dict(alpha=-1.0), "alpha"), (cb, ds, dict(alpha=float("nan")), "alpha"),
        (cb, ds, dict(sigma2=0.0), "sigma2"), (cb, ds, dict(sigma2=-1.0), "sigma2"), (cb, ds, dict(sigma2=float("nan")), "sigma2"),
        (cb, ds, dict(sigma2=float("inf")), "sigma2"),
    ]
    for book, data, kw, word in cases:
        args = dict(epochs=5, alpha=1.0, sigma2=1.0)
        args.update(kw)
        with pytest.raises(Exception) as ei:
            E.rslvq_train(book, data, **args)
        assert str(ei.value).startswith("somhip_rslvq_train: ") and word in str(ei.value), (kw, str(ei.value))
        assert (bits32(book.download()) == bits32(c[:book.n])).all()
    z = np.zeros
    for fn, name in ((lambda: E.rslvq_search(E.Codebook(eng, c), ds, 1.0), "somhip_rslvq_search"), (lambda: E.rslvq_search(cb, ds, 0.0), "somhip_rslvq_search"),
                     (lambda: E.rslvq_search(cb, ds, 1.0, n=0), "somhip_rslvq_search"),
                     (lambda: E.rslvq_posterior(cb, ds, -1.0), "somhip_debug_rslvq_posterior"), (lambda: E.rslvq_posterior(cb, ds, 1.0, chunk=65), "somhip_debug_rslvq_posterior"),
                     (lambda: E.rslvq_posterior(cb, ds, 1.0, chunk=8192), "somhip_debug_rslvq_posterior"),
                     (lambda: E.rslvq_sums(cb, ds, z((50, 6)), chunk=32), "somhip_debug_rslvq_sums"), (lambda: E.rslvq_sums(cb, E.Dataset(eng, x), z((50, 6))), "somhip_debug_rslvq_sums"),
                     (lambda: E.rslvq_update(cb, 1.0, 1.0, 0, z((6, 4)), z(6)), "somhip_debug_rslvq_update"),
                     (lambda: E.rslvq_update(cb, 1.0, 0.0, 5, z((6, 4)), z(6)), "somhip_debug_rslvq_update"),
                     (lambda: E.rslvq_update(E.Codebook(eng, c), 1.0, 1.0, 5, z((6, 4)), z(6)), "somhip_debug_rslvq_update")):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(name + ": "), str(ei.value)
    assert (bits32(cb.download()) == bits32(c)).all()


@pytest.mark.gpu
def test_timing_counts_the_four_stages(E, eng):
    """130 samples at the rule's chunk: one chunk an epoch; the stages are timed whatever timing_select names"""
    x, dl, c, cl = clusters(4, 130, 6, 8)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    eng.timing(True); eng.timing_reset()
    E.rslvq_train(cb, ds, 3, 1.0, 2.0, stats=False)
    E.rslvq_posterior(cb, ds, 2.0, chunk=64)                            # three chunks
    t = eng.rslvq_timing()
    eng.timing(False)
    assert t["distances"][0] == 6 and t["k_rslvq_posterior"][0] == 6 and t["k_rslvq_sums"][0] == 3 and t["k_rslvq_update"][0] == 3
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


@pytest.mark.gpu
def test_rslvq_tool_writes_the_engines_rows_and_lines(E, eng, tools, tmp_path):
    """the tool on files: the written .cod holds the rows engine.rslvq_train leaves, the -v lines its alpha_t, cost and
    accuracy per epoch, the last line and -pout what rslvq_search says of those rows, and the accuracy is what `accuracy`
    says of the written codebook; -epochs 0 evaluates -cin and writes no codebook"""
    x, dl, c, cl = clusters(21, 120, 9, 5, sep=1.0)
    names = ["ape", "bee", "cat"]
    dat, cod, out, pout = tmp_path / "d.dat", tmp_path / "c.cod", tmp_path / "o.cod", tmp_path / "p.txt"
    write_dat(dat, x, dl, names)
    write_dat(cod, c, cl, names)
    from som_lvq_pak_amd import textio
    p = run("rslvq", "-din", dat, "-cin", cod, "-cout", out, "-epochs", 4, "-alpha", 2.5, "-sigma2", 1.5, "-pout", pout, "-v")
    assert p.returncode == 0, p.stderr
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.rslvq_train(cb, ds, 4, 2.5, 1.5)
    fcost, fcorrect, fpown = E.rslvq_search(cb, ds, 1.5)
    text = out.read_text().split("\n")
    rows = np.array([[float(v) for v in ln.split()[:5]] for ln in text[1:] if ln.strip() and not ln.startswith("#")], dtype=f32)
    printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)     # the file is "%g" text
    assert (bits32(rows) == bits32(printed)).all()
    assert [ln.split()[5] for ln in text[1:] if ln.strip() and not ln.startswith("#")] == [names[int(l)] for l in cl]
    lines = [ln for ln in p.stdout.split("\n") if ln.startswith("epoch ")]
    assert len(lines) == 4
    for t, ln in enumerate(lines):
        m = re.match(r"epoch (\d+) alpha ([-+.\deE]+) cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", ln)
        assert m and int(m.group(1)) == t, ln
        assert float(m.group(2)) == float(f32(E.glvq_alpha(2.5, 4, t)))                                       # "%.9g" carries a float
        assert float(m.group(3)) == cost[t] and float(m.group(4)) == pytest.approx(100.0 * correct[t] / 120, abs=0.006)
    m = re.search(r"^final cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", p.stdout, flags=re.M)
    assert m and float(m.group(1)) == fcost and float(m.group(2)) == pytest.approx(100.0 * fcorrect / 120, abs=0.006)
    plines = pout.read_text().split("\n")[:-1]
    assert [ln.split()[0] for ln in plines] == [names[int(l)] for l in dl]
    assert np.allclose([float(ln.split()[1]) for ln in plines], fpown, rtol=1e-8, atol=0)                     # "%.9g" of a double
    cb.close()
    # the written file, read back ("%g" text): -epochs 0 on it, and the accuracy tool
    p0 = run("rslvq", "-din", dat, "-cin", out, "-cout", tmp_path / "never.cod", "-epochs", 0, "-sigma2", 1.5, "-v")
    assert p0.returncode == 0 and not (tmp_path / "never.cod").exists() and "epoch " not in p0.stdout, p0.stderr
    cb = E.Codebook(eng, rows, labels=cl)
    wcost, wcorrect, _ = E.rslvq_search(cb, ds, 1.5)
    m0 = re.search(r"^final cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", p0.stdout, flags=re.M)
    assert m0 and float(m0.group(1)) == wcost and float(m0.group(2)) == pytest.approx(100.0 * wcorrect / 120, abs=0.006)
    a = run("accuracy", "-din", dat, "-cin", out)
    assert a.returncode == 0, a.stderr
    ma = re.search(r"Total accuracy:\s+(\d+) entries\s+([\d.]+) %", a.stdout)
    assert ma and int(ma.group(1)) == 120 and float(ma.group(2)) == pytest.approx(100.0 * wcorrect / 120, abs=0.006)
    cb.close(); ds.close()
