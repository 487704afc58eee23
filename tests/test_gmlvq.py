"""Batch GMLVQ (K12: somhip_gmlvq_train, somhip_gmlvq_search, somhip_gmlvq_project and the stages, engine.gmlvq_train /
gmlvq_search / gmlvq_project / gmlvq_sums / gmlvq_update, the gmlvq tool) against the numpy replay in gmlvq_replay.py.

The projection is compared by bit pattern, the search by bit pattern and index.  With the identity the sums, the gradient of
Omega, the update, Omega's step, the cost and whole runs are compared by bit pattern as well: every operation of the
definition is one IEEE rounding and every sum a chain in a fixed order.  With the sigmoid the device's exp and the C
library's may differ by an ulp each, so the gradient is compared against the bound DESIGN.md K12 derives from that
(gmlvq_replay.grad_bound).  The shapes, the edge cases and the helpers are test_glvq's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glvq_replay as G
import gmlvq_replay as M
import grlvq_replay as R
import test_glvq as TG
from conftest import ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
f32, f64 = np.float32, np.float64
bits32, bits64, run = TG.bits32, TG.bits64, TG.run


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("gmlvq", "accuracy")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


# ------------------------------------------------------------------------------------------------ without a GPU
NAMES = ("somhip_gmlvq_train", "somhip_gmlvq_search", "somhip_gmlvq_project", "somhip_debug_gmlvq_sums", "somhip_debug_gmlvq_update",
         "somhip_gmlvq_timing")


def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.SIGNATURES
    for name in NAMES:
        assert hasattr(lib, name) and name in S, name
    assert S["somhip_gmlvq_train"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.GmlvqParams), _lib.c_float_p, _lib.c_double_p,
                                                 _lib.c_i64_p])
    assert S["somhip_gmlvq_project"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _lib.c_float_p, C.c_int32, _lib.c_float_p])
    assert S["somhip_gmlvq_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.GmlvqParams._fields_] == ["epochs", "start_epoch", "count", "first", "n", "alpha", "sigmoid_beta", "eps", "rank"]
    assert [f[0] for f in _lib.GmlvqParams._fields_][:-1] == [f[0] for f in _lib.GrlvqParams._fields_]
    assert C.sizeof(_lib.GmlvqParams) == 56
    for name in ("gmlvq_train", "gmlvq_search", "gmlvq_project", "gmlvq_sums", "gmlvq_update", "gmlvq_omega"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "gmlvq_timing")
    om = engine.gmlvq_omega(5, 2)
    assert (bits32(om) == bits32(M.default_omega(5, 2))).all() and (om != 0).sum() == 5 and abs(float((om.astype(f64) ** 2).sum()) - 1.0) < 1e-6


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int somhip_gmlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_gmlvq_params *p, float *omega , "
            "double *cost_out , int64_t *correct_out );") in hdr
    assert ("int somhip_gmlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank, "
            "float *dplus, int32_t *iplus, float *dminus, int32_t *iminus);") in hdr
    assert ("int somhip_gmlvq_project(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank, "
            "float *out);") in hdr
    assert "int somhip_gmlvq_timing(somhip_engine *e, int64_t launches[6], double total_ms[6]);" in hdr
    assert "int somhip_debug_gmlvq_sums(" in hdr and "int somhip_debug_gmlvq_update(" in hdr
    m = re.search(r"typedef struct somhip_gmlvq_params \{(.*?)\} somhip_gmlvq_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int64_t epochs; int64_t start_epoch, count; int64_t first, n; float alpha; "
                                                            "float sigmoid_beta; float eps; int32_t rank;")


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 6)(), (C.c_double * 6)()
    assert lib.somhip_gmlvq_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_gmlvq_timing: null engine"


def test_replay_with_the_identity_is_the_glvq_replay():
    """omega the dim x dim identity and eps 0: the projection returns the rows, P = g and Dl = g, so rows, cost and count are
    glvq_replay's by bit pattern, and omega keeps its bits"""
    x, dl, c, cl = R.learning_case(4)
    eye = np.eye(8, dtype=f32)
    rows, om, cost, correct = M.train(c, cl, x, dl, eye, 3, 10.0, 0.0, first=5, n=500)
    grows, gcost, gcorrect = G.train(c, cl, x, dl, 3, 10.0, first=5, n=500)
    assert (bits32(rows) == bits32(grows)).all() and (bits64(cost) == bits64(gcost)).all() and (correct == gcorrect).all()
    assert (bits32(om) == bits32(eye)).all()
    assert (bits32(M.project(eye, x)) == bits32(x + f32(0.0))).all()


LEARNING = dict(epochs=50, alpha=20.0, eps=1.0)


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_replay_learning_run(seed):
    """the definition itself, on the CPU: K11's learning data rotated by a fixed orthogonal matrix, so no single axis separates
    the classes.  GMLVQ at rank 2 and rank 8 ends at 0.88 or more with 0.98 or more of trace(Omega^T Omega) in the two
    informative directions; glvq stays at 0.70 or less, grlvq at 0.82 or less.  (Seen: 0.910 - 0.932, >= 0.995, 0.55 - 0.62,
    0.75 - 0.76.)  The cost is not monotone under this schedule and is not asserted."""
    x, dl, c, cl, Q = M.learning_case(seed)
    for rank in (2, 8):
        rows, om, cost, _ = M.train(c, cl, x, dl, M.default_omega(8, rank), LEARNING["epochs"], LEARNING["alpha"], LEARNING["eps"])
        acc, share = M.evaluate(rows, cl, x, dl, om)[1], M.informative_share(om, Q)
        print("seed %d rank %d: accuracy %.3f, informative share %.4f" % (seed, rank, acc, share))
        assert acc >= 0.88 and share >= 0.98
        assert abs(float((om.astype(f64) ** 2).sum()) - 1.0) < 1e-6
    rows, _, _ = G.train(c, cl, x, dl, 50, 10.0)
    dp, ip, dm, im = G.search(rows, cl, x, dl)
    assert G.terms(dp, ip, dm, im)[3] / 600 <= 0.70
    rows, lam, _, _ = R.train(c, cl, x, dl, np.full(8, f32(1.0) / f32(8), dtype=f32), 50, 80.0, 0.5)
    assert R.evaluate(rows, cl, x, dl, lam)[1] <= 0.82


KERNELS = {"project": r"_ZN6somhip15k_gmlvq_project\w+", "grad": r"_ZN6somhip18k_gmlvq_omega_grad\w+", "reduce": r"_ZN6somhip20k_gmlvq_omega_reduce\w+",
           "update": r"_ZN6somhip14k_gmlvq_update\w+", "search": r"_ZN6somhip12k_scan_class\w+"}


def test_register_budget(built, tmp_path):
    """the four new kernels keep their chains in registers -- no scratch, no spills; the projection's chain is v_fma_f64;
    the search it shares with batch GLVQ has no contracted fp32 operation"""
    s = os.path.join(str(tmp_path), "k.s")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                          "--cuda-device-only", "-S", "-o", s, "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")], stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    txt = open(s).read()
    for key, pat in KERNELS.items():
        bodies = dict(re.findall(r"^(%s):.*?\n(.*?)s_endpgm" % pat, txt, flags=re.S | re.M))
        assert len(bodies) == (2 if key == "search" else 1), (key, sorted(bodies))
        for name, body in bodies.items():
            assert "scratch_" not in body, name
            m = re.search(r"Function Name: %s\b.*?LDS Size" % re.escape(name), res.stderr, flags=re.S)
            assert m, "no resource remark for " + name
            rem = m.group(0)
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem) and re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
            fma32 = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)(?:_mix|_legacy)?_f32.*", body)
            if key == "search":                                     # (elsewhere the 64-bit integer division's expansion has two)
                assert not fma32, (name, fma32[:3])
            fma64 = len(re.findall(r"\bv_(?:fma|fmac)_f64", body))       # (v_fmac_f64_e32: no word boundary behind f64)
            if key == "project":
                assert fma64 >= 8, (name, fma64)
            elif key in ("grad", "reduce", "update"):
                assert fma64 == 0, (name, fma64)                    # every product of these chains rounds before it is added


def omega_text(om):
    return "%d %d\n" % om.shape + "".join(" ".join("%.9g" % float(v) for v in row) + "\n" for row in om)


def test_gmlvq_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("gmlvq", "-help")
    assert p.returncode == 0 and p.stdout.startswith("gmlvq - ")
    assert all(w in p.stdout for w in ("-epochs", "-alpha", "-eps", "-rank", "-sigmoid", "-oin", "-oout", "-pout"))
    cod, dat, out, oout, pout = tmp_path / "c.cod", tmp_path / "d.dat", tmp_path / "o.cod", tmp_path / "o.om", tmp_path / "p.dat"
    cod.write_text("2\n0 0 a\n1 1 b\n")
    dat.write_text("2\n0.25 0.5 a\n0.75 0.5 b\n")
    for args, word in ((("-epochs", -2, "-alpha", 1, "-eps", 1), "-epochs"), (("-epochs", 0), "-epochs 0"),
                       (("-epochs", 2, "-alpha", -1, "-eps", 1), "-alpha"), (("-epochs", 2, "-alpha", "nan", "-eps", 1), "-alpha"),
                       (("-epochs", 2, "-alpha", 1, "-eps", -1), "-eps"), (("-epochs", 2, "-alpha", 1, "-eps", "nan"), "-eps"),
                       (("-epochs", 2, "-alpha", 1, "-eps", 1, "-sigmoid", -1), "-sigmoid"),
                       (("-epochs", 2, "-alpha", 1, "-eps", 1, "-sigmoid", "nan"), "-sigmoid"),
                       (("-epochs", 2, "-alpha", 1, "-eps", 1, "-rank", 0), "-rank"), (("-epochs", 2, "-alpha", 1, "-eps", 1, "-rank", -3), "-rank")):
        p = run("gmlvq", "-cin", cod, "-din", dat, "-cout", out, "-oout", oout, "-pout", pout, *args)
        assert p.returncode == 1 and p.stderr.startswith("gmlvq: " + word), (args, p.stderr)
    good = ("-epochs", 2, "-alpha", 1, "-eps", 0.5)
    p = run("gmlvq", "-cin", cod, "-din", dat, "-cout", out, "-rank", 3, *good)
    assert p.returncode == 1 and p.stderr.startswith("gmlvq: -rank 3 is larger than the dimension 2"), p.stderr
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3 a\n4 5 6 b\n")
    p = run("gmlvq", "-cin", cod, "-din", dim3, "-cout", out, *good)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    for name, text, word in (("x.cod", "2\nx 0 a\n1 1 b\n", "masked components"), ("x.dat", "2\nx 0.5 a\n0.75 0.5 b\n", "masked components"),
                             ("n.cod", "2\n0 0\n1 1\n", "no labels"), ("n.dat", "2\n0.25 0.5\n0.75 0.5\n", "no labels"),
                             ("one.cod", "2\n0 0 a\n1 1 a\n", "one label"), ("z.dat", "2\n0.25 0.5 a\n0.75 0.5 z\n", "no codebook row")):
        f = tmp_path / name
        f.write_text(text)
        p = run("gmlvq", "-cin", f if name.endswith(".cod") else cod, "-din", f if name.endswith(".dat") else dat, "-cout", out, *good)
        assert p.returncode == 1 and word in p.stderr, (name, p.stderr)
    for text, word in (("2 3\n1 0 0\n0 1 0\n", "has dimension 3, the codebook 2"), ("3 2\n1 0\n0 1\n1 1\n", "has 3 rows, outside 1 .. 2"),
                       ("0 2\n", "has 0 rows"), ("2 2\n1 0\n0 nan\n", "not a finite number"), ("2 2\n1 inf\n0 1\n", "not a finite number"),
                       ("2 2\n1 abc\n0 1\n", "can't read value 1"), ("2 2\n1 0\n0\n", "ends after 3 of 4 values"), ("two 2\n1 0\n", "M dim"),
                       ("", "is empty"), ("2 2\n0 0\n0 0\n", "all zero")):
        oin = tmp_path / "bad.om"
        oin.write_text(text)
        p = run("gmlvq", "-cin", cod, "-din", dat, "-cout", out, "-oout", oout, "-pout", pout, "-oin", oin, *good)
        assert p.returncode == 1 and p.stderr.startswith("gmlvq: ") and word in p.stderr, (text, p.stderr)
    oin = tmp_path / "one.om"
    oin.write_text("1 2\n1 1\n")
    p = run("gmlvq", "-cin", cod, "-din", dat, "-cout", out, "-oin", oin, "-rank", 2, *good)
    assert p.returncode == 1 and "has 1 rows, -rank asks for 2" in p.stderr
    p = run("gmlvq", "-cin", cod, "-din", dat, "-cout", out, "-oin", tmp_path / "none.om", *good)
    assert p.returncode == 1 and "can't open omega file" in p.stderr
    assert not out.exists() and not oout.exists() and not pout.exists()


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


def null_space_rows(c, cl):
    """rows of `c` made to differ only in the even components (which omegas()["null"] gives no weight): a pair within a
    class and a pair across two classes, so the lowest row must win"""
    if c.shape[0] >= 8:
        a = 2
        same = np.flatnonzero(cl == cl[a])
        diff = np.flatnonzero(cl != cl[a])
        if len(same) > 2:
            c[same[-1], 1::2] = c[a, 1::2]
        c[diff[len(diff) // 2], 1::2] = c[a, 1::2]


def omegas(seed, m, dim):
    """The matrices of a projection or search case, by name"""
    rs = np.random.RandomState(seed)
    rnd = (0.5 * rs.standard_normal((m, dim))).astype(f32)
    rnd[rs.uniform(size=(m, dim)) < 0.2] = 0.0
    out = {"random with zeros": rnd, "all zero": np.zeros((m, dim), dtype=f32)}
    null = (0.5 * rs.standard_normal((m, dim))).astype(f32)
    null[:, ::2] = 0.0
    out["null space"] = null
    big = (0.5 * rs.standard_normal((m, dim))).astype(f32)
    big[rs.randint(0, m), rs.randint(0, dim)] = f32(1e6)
    big[rs.randint(0, m), rs.randint(0, dim)] = f32(1e-30)
    if dim >= 3:
        big[0, 0], big[m - 1, dim - 1] = f32(1e6), f32(1e-30)
    out["1e6 and 1e-30"] = big
    if m == dim:
        out["identity"] = np.eye(dim, dtype=f32)
    return out


# rows, dim, samples, classes, ranks: rows at the lane, group and 4-groups-per-wave edges, dims around the 4- and 64-column
# edges, runs around the 32-sample tile and the 64-row workgroup of the projection, every rank of 1 .. 5, 63 .. 65 and dim
PROJECT_SHAPES = [(2, 1, 1, 2, (1,)), (2, 4, 33, 2, (1, 2, 3, 4)), (63, 3, 31, 3, (1, 2, 3)), (64, 5, 32, 4, (1, 4, 5)), (65, 63, 33, 5, (5, 63)),
                  (64, 64, 700, 7, (2, 63, 64)), (1030, 65, 700, 7, (3, 64, 65)), (65, 129, 31, 2, (1, 33, 65, 129)), (1030, 4, 32, 2, (2, 4)),
                  (1030, 1, 700, 4, (1,)), (63, 64, 1, 6, (64,)), (70, 128, 65, 3, (32, 128))]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,classes,ranks", PROJECT_SHAPES)
def test_projection_and_search_equal_the_replay(E, eng, rows, dim, n, classes, ranks):
    """the public projection of the samples (plain and wrapped ranges) and of the rows by bit pattern, and the search by bit
    pattern and index against glvq_replay.search on the replay's Y and V -- so the projections are the tiles the search saw;
    test_glvq.edge_case's single-row class, class behind the last full group, duplicates, d = 0 and D = 0; rows that differ
    only in omega's null space; omega with zeros, with 1e6 and 1e-30 entries, all zero; the identity, where the search is
    somhip_debug_glvq_search on the direct route bit for bit; every call twice"""
    n_data = max(n, 5) if n != 700 else 300                         # 700 samples of 300 rows: the run wraps twice
    c, cl, x, dl = TG.edge_case(3000 + rows + dim, rows, dim, n_data, classes)
    null_space_rows(c, cl)
    cb = E.Codebook(eng, c, labels=cl)
    ds = E.Dataset(eng, x, labels=dl)
    for m in ranks:
        for name, om in omegas(rows * 131 + dim + m, m, dim).items():
            V, Y = M.project(om, c), M.project(om, x)
            for first in (0, n_data - 2):                            # the second range wraps after two rows
                want = G.search(V, cl, Y, dl, first, n)
                for again in range(2):
                    got_v = E.gmlvq_project(cb, None, om)
                    got_y = E.gmlvq_project(cb, ds, om, first, n)
                    assert got_v.shape == (rows, m) and got_y.shape == (n, m)
                    assert (bits32(got_v) == bits32(V)).all(), (m, name)
                    assert (bits32(got_y) == bits32(Y[(first + np.arange(n)) % n_data])).all(), (m, name, first)
                    dp, ip, dm, im = E.gmlvq_search(cb, ds, om, first, n)
                    assert (ip == want[1]).all() and (im == want[3]).all(), (m, name, first, np.flatnonzero((ip != want[1]) | (im != want[3]))[:5])
                    assert (bits32(dp) == bits32(want[0])).all() and (bits32(dm) == bits32(want[2])).all(), (m, name, first)
                if name == "all zero":
                    assert not bits32(dp).any() and not bits32(dm).any() and not bits32(got_y).any()
                if name == "identity":
                    plain = E.glvq_search(cb, ds, first, n, E.GLVQ_DIRECT)
                    assert all((bits32(a) == bits32(b)).all() for a, b in zip((dp, ip, dm, im), plain[:4]))
    cb.close(); ds.close()


def sums_case(seed, rows, dim, n, one, m):
    """test_glvq.sums_case with duplicated samples and a sample equal to rows of two classes (D == 0 under any omega), and a
    matrix with a zero column, a large and a small entry"""
    c, cl, x, dl = TG.sums_case(seed, rows, dim, min(n, 500), one_winner=one)
    nd = x.shape[0]
    if nd > 8:
        x[5] = x[4]; dl[5] = dl[4]
        x[nd // 2] = x[4]; dl[nd // 2] = dl[4]
        other = int(np.flatnonzero(cl != cl[0])[0])
        c[other] = c[0]
        x[7] = c[0]
    om = (np.random.RandomState(seed + 1).standard_normal((m, dim)) / np.sqrt(dim)).astype(f32)
    om[:, dim // 2] = 0.0
    if dim > 2:
        om[0, 0], om[m - 1, dim - 1] = f32(3.0), f32(1e-3)
    return c, cl, x, dl, om


def replay_stages(c, cl, x, dl, om, first, n, beta=0.0):
    dp, ip, dm, im = M.search(c, cl, x, dl, om, first, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im, beta)
    S = G.sums(x, ip, im, xp, xm, f, c.shape[0], first)
    S["grad"], S["abs_grad"] = M.omega_grad(c, x, om, ip, im, xp, xm, first)
    return S, xp, xm, f, correct, (dp, dm)


# rows, dim, samples, every sample on one prototype, rank.  The first seven are test_glvq's shapes; the rest walk the edge
# of the gradient's 4096-sample block (over 500 data rows: the run wraps) with few rows and components.
SUMS_SHAPES = [(12, 16, 300, False, 16), (5, 63, 150, False, 2), (5, 64, 150, False, 64), (5, 65, 150, False, 9), (7, 3, 200, True, 3),
               (256, 5, 20, False, 4), (70, 129, 97, False, 65), (4, 8, 1, False, 3), (6, 8, 4095, False, 8), (6, 7, 4096, False, 2),
               (5, 8, 4097, False, 5), (6, 5, 8193, False, 1), (300, 260, 40, False, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,one,m", SUMS_SHAPES)
def test_identity_sums_gradient_update_and_omega_step_equal_the_replay_bit_for_bit(E, eng, rows, dim, n, one, m):
    """all samples on one prototype, most prototypes unchosen, duplicated samples, a sample with D == 0, runs of 1, 4095,
    4096, 4097 and 8193 samples: xi, f, Sp, Sm, sp, sm, cost, the counts and Gm; then, from those sums on the host, the rows
    and omega after an ordinary step, with eps_t == 0 (no step, no normalisation), and with a gradient that drives the
    matrix to zero (omega keeps its bits); the rows no sample chose keep theirs"""
    c, cl, x, dl, om = sums_case(rows * 7 + dim, rows, dim, n, one, m)
    first = 11
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.gmlvq_sums(cb, ds, om, first, n)
    S, xp, xm, f, correct, (dp, dm) = replay_stages(c, cl, x, dl, om, first, n)
    if n in (150, 200, 300):
        assert ((dp.astype(f64) + dm.astype(f64)) == 0).any() and (xp == 0).any()           # the D == 0 sample is there
    assert (bits64(got["xi_plus"]) == bits64(xp)).all() and (bits64(got["xi_minus"]) == bits64(xm)).all() and (bits64(got["f"]) == bits64(f)).all()
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    for key in ("sums_plus", "sums_minus", "cost", "grad"):
        assert (bits64(got[key]) == bits64(S[key])).all(), (key, np.flatnonzero(bits64(got[key]) != bits64(S[key]))[:5])
    assert got["grad"].shape == (m, dim) and np.abs(got["grad"]).max() > 0
    if one:
        assert got["n_plus"][rows // 2] == n and got["n_plus"].sum() == n
    if rows == 256:
        assert ((got["n_plus"] == 0) & (got["n_minus"] == 0)).sum() > 200
    again = E.gmlvq_sums(cb, ds, om, first, n)
    assert (bits64(again["grad"]) == bits64(got["grad"])).all()
    unchosen = (got["n_plus"] == 0) & (got["n_minus"] == 0)
    alpha_t, eps_t = R.rate_at(7.5, 9, 2), R.rate_at(0.5, 9, 2)
    for name, grad, e_t, nn in (("plain", got["grad"], eps_t, n), ("eps 0", got["grad"], f32(0.0), n),
                                ("to zero", om.astype(f64) * 128.0, f32(0.5), 64)):       # 0.5 / 64 * 128 omega = omega exactly
        cb.upload(c)
        after = E.gmlvq_update(cb, alpha_t, e_t, nn, om, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"], grad)
        assert (bits32(after) == bits32(M.omega_step(om, grad, e_t, nn))).all(), name
        if name == "plain":
            assert abs(float((after.astype(f64) ** 2).sum()) - 1.0) < 1e-6 and (bits32(after) != bits32(om)).any()
        else:
            assert (bits32(after) == bits32(om)).all(), name
        rows_after = cb.download()
        assert (bits32(rows_after) == bits32(M.update(c, got, om, alpha_t, nn))).all(), name
        assert (bits32(rows_after[unchosen]) == bits32(c[unchosen])).all()
        assert (bits32(rows_after) != bits32(c)).any()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,beta,m", [(12, 16, 300, 2.0, 16), (5, 65, 150, 0.5, 9), (256, 5, 20, 4.0, 2), (6, 8, 4097, 1.0, 3)])
def test_sigmoid_gradient_within_the_derived_bound(E, eng, rows, dim, n, beta, m):
    """xi within (20 + 8 exp(beta)) u of the replay's; Gm within 1.001 times gmlvq_replay.grad_bound, which is relative to
    the chain of |xi u t|.  Largest error / bound seen on the MI355X: xi 0.082, f 0.32, Gm 0.00021."""
    c, cl, x, dl, om = sums_case(rows + dim, rows, dim, n, False, m)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.gmlvq_sums(cb, ds, om, 0, n, beta)
    S, xp, xm, f, correct, _ = replay_stages(c, cl, x, dl, om, 0, n, beta)
    rel = G.xi_rel_bound(beta)
    worst = {}
    for name, ref, tol in (("xi_plus", xp, rel * xp), ("xi_minus", xm, rel * xm), ("f", f, G.F_REL_BOUND * f)):
        err = np.abs(got[name] - ref)
        worst[name] = float((err / np.maximum(tol, 1e-300)).max())
        assert (err <= tol).all(), (name, worst)
    bp, bm, bc = G.sums_bound(S, beta)
    for name, tol in (("sums_plus", bp), ("sums_minus", bm), ("cost", bc), ("grad", 1.001 * M.grad_bound(S["abs_grad"], beta, n))):
        err = np.abs(got[name] - S[name])
        worst[name] = float((err / tol).max())
        assert (err <= tol).all(), (name, worst)
    print("largest error / bound:", worst)
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    cb.close(); ds.close()


@pytest.mark.gpu
def test_the_identity_without_a_rate_is_batch_glvq(E, eng):
    """omega the identity with eps 0 over 3 epochs: codebook, cost and count are somhip_glvq_train's bit for bit, omega keeps
    its bits"""
    x, dl, c, cl = TG.clusters(9, 400, 12, 16)
    first, n = 7, 390
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    gcost, gcorrect = E.glvq_train(cb, ds, 3, 10.0, first=first, n=n)
    grows = cb.download()
    cb.upload(c)
    om, cost, correct = E.gmlvq_train(cb, ds, 3, 10.0, 0.0, np.eye(16, dtype=f32), first=first, n=n)
    assert (bits32(cb.download()) == bits32(grows)).all() and (bits64(cost) == bits64(gcost)).all() and (correct == gcorrect).all()
    assert (bits32(om) == bits32(np.eye(16, dtype=f32))).all() and (bits32(grows) != bits32(c)).any()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beta,m", [(0.0, 16), (0.0, 3), (2.0, 5)])
def test_runs(E, eng, beta, m):
    """5 epochs in one call equal five calls handing omega on and equal themselves run twice; an epoch equals its stages;
    rows, omega, cost and correct equal the replay's (by bit pattern with the identity)"""
    x, dl, c, cl = TG.clusters(9, 400, 12, 16)
    first, n, T, alpha, eps = 7, 390, 5, 10.0, 0.5
    om0 = np.random.RandomState(2).uniform(-0.3, 0.3, size=(m, 16)).astype(f32)             # not normalised: taken as it is
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    om, cost, correct = E.gmlvq_train(cb, ds, T, alpha, eps, om0, beta, first=first, n=n)
    one = cb.download()
    assert (bits32(om) != bits32(om0)).any() and abs(float((om.astype(f64) ** 2).sum()) - 1.0) < 1e-6
    cb.upload(c)
    om2, cost2, correct2 = E.gmlvq_train(cb, ds, T, alpha, eps, om0, beta, first=first, n=n)
    assert (bits32(cb.download()) == bits32(one)).all() and (bits64(cost2) == bits64(cost)).all() and (correct2 == correct).all()
    assert (bits32(om2) == bits32(om)).all()
    cb.upload(c)
    o = om0
    for t in range(T):
        o, ct, rt = E.gmlvq_train(cb, ds, T, alpha, eps, o, beta, start_epoch=t, count=1, first=first, n=n)
        assert bits64(ct)[0] == bits64(cost)[t] and rt[0] == correct[t]
    assert (bits32(cb.download()) == bits32(one)).all() and (bits32(o) == bits32(om)).all()
    cb.upload(c)
    o = om0
    for t in range(T):                                               # an epoch is its stages
        got = E.gmlvq_sums(cb, ds, o, first, n, beta)
        chain = f64(0.0)
        for v in got["cost"]:
            chain = chain + v
        assert bits64(chain / f64(n))[()] == bits64(cost)[t] and got["correct"] == correct[t]
        o = E.gmlvq_update(cb, E.glvq_alpha(alpha, T, t), E.glvq_alpha(eps, T, t), n, o, got["sums_plus"], got["n_plus"], got["sums_minus"],
                           got["n_minus"], got["grad"])
    assert (bits32(cb.download()) == bits32(one)).all() and (bits32(o) == bits32(om)).all()
    rows, rom, rcost, rcorrect = M.train(c, cl, x, dl, om0, T, alpha, eps, beta, first, n)
    if beta == 0.0:
        assert (bits32(one) == bits32(rows)).all() and (bits64(cost) == bits64(rcost)).all() and (bits32(om) == bits32(rom)).all()
    else:
        assert np.allclose(one, rows, rtol=0, atol=1e-5) and np.allclose(cost, rcost, rtol=1e-12, atol=0) and np.allclose(om, rom, rtol=0, atol=1e-6)
    assert (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [4, 5, 6])
def test_learning_finds_the_informative_directions(E, eng, seed):
    """K11's learning data rotated by a fixed orthogonal matrix, 600 samples, 6 prototypes, T = 50, alpha = 20, eps = 1 from
    engine.gmlvq_omega at rank 2 and rank 8: bit-equal with the replay, accuracy 0.88 or more, 0.98 or more of
    trace(Omega^T Omega) in the two informative directions; glvq at alpha 10 ends at 0.70 or less and grlvq at alpha 80,
    eps 0.5 at 0.82 or less.  (The replay gave 0.910 - 0.932, shares from 0.995, 0.55 - 0.62 and 0.75 - 0.76.)"""
    x, dl, c, cl, Q = M.learning_case(seed)
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    for rank in (2, 8):
        cb.upload(c)
        om, cost, correct = E.gmlvq_train(cb, ds, LEARNING["epochs"], LEARNING["alpha"], LEARNING["eps"], E.gmlvq_omega(8, rank))
        _, last, right = E.gmlvq_train(cb, ds, 1, 0.0, 0.0, om)                           # the state the run ended with
        share = M.informative_share(om, Q)
        print("seed %d rank %d: cost %.4f -> %.4f, accuracy %.3f, informative share %.4f" % (seed, rank, cost[0], last[0], right[0] / 600, share))
        assert right[0] / 600 >= 0.88 and share >= 0.98
        dp, ip, dm, im = E.gmlvq_search(cb, ds, om)
        assert int(((dp < dm) | ((dp == dm) & (ip < im))).sum()) == right[0]              # the public search evaluates the model
        rows, rom, rcost, _ = M.train(c, cl, x, dl, M.default_omega(8, rank), LEARNING["epochs"], LEARNING["alpha"], LEARNING["eps"])
        assert (bits32(cb.download()) == bits32(rows)).all() and (bits32(om) == bits32(rom)).all() and (bits64(cost) == bits64(rcost)).all()
    cb.upload(c)
    E.glvq_train(cb, ds, 50, 10.0)
    _, right0 = E.glvq_train(cb, ds, 1, 0.0)
    assert right0[0] / 600 <= 0.70
    cb.upload(c)
    lam, _, _ = E.grlvq_train(cb, ds, 50, 80.0, 0.5)
    _, _, right1 = E.grlvq_train(cb, ds, 1, 0.0, 0.0, lam)
    assert right1[0] / 600 <= 0.82
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_leave_rows_and_omega(E, eng):
    from som_lvq_pak_amd import _lib
    x, dl, c, cl = TG.clusters(3, 50, 6, 4)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    mask = np.zeros(x.shape, dtype=np.uint8); mask[3, 1] = 1
    nan, inf = float("nan"), float("inf")
    bad = lambda r, k, v: np.array([[0.5 if (i, j) != (r, k) else v for j in range(4)] for i in range(2)], dtype=f32)
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
        (cb, ds, dict(alpha=-1.0), "alpha"), (cb, ds, dict(alpha=nan), "alpha"),
        (cb, ds, dict(sigmoid_beta=-0.5), "sigmoid_beta"), (cb, ds, dict(sigmoid_beta=nan), "sigmoid_beta"),
        (cb, ds, dict(eps=-0.5), "eps"), (cb, ds, dict(eps=nan), "eps"),
        (cb, ds, dict(omega=bad(1, 2, nan)), "omega[1][2]"), (cb, ds, dict(omega=bad(0, 3, inf)), "omega[0][3]"),
        (cb, ds, dict(omega=bad(1, 0, -inf)), "omega[1][0]"), (cb, ds, dict(omega=np.zeros((3, 4), dtype=f32)), "omega is all zero"),
    ]
    for book, data, kw, word in cases:
        args = dict(epochs=5, alpha=1.0, eps=0.5)
        args.update(kw)
        with pytest.raises(Exception) as ei:
            E.gmlvq_train(book, data, **args)
        assert str(ei.value).startswith("somhip_gmlvq_train: ") and word in str(ei.value), (kw, str(ei.value))
        assert (bits32(book.download()) == bits32(c[:book.n])).all()
    lib = cb.e.lib
    p = _lib.GmlvqParams(5, 0, 5, 0, 50, 1.0, 0.0, 0.5, 2)
    assert lib.somhip_gmlvq_train(cb.h, ds.h, C.byref(p), None, None, None) != 0                           # a NULL omega
    assert lib.somhip_last_error().decode() == "somhip_gmlvq_train: null omega"
    for rank in (0, -1, 5):                                                                                 # the rank, through the ABI
        p.rank = rank
        om = np.full((5, 4), 0.5, dtype=f32)
        assert lib.somhip_gmlvq_train(cb.h, ds.h, C.byref(p), om.ctypes.data_as(_lib.c_float_p), None, None) != 0
        assert lib.somhip_last_error().decode() == "somhip_gmlvq_train: rank %d outside [1, 4]" % rank
        assert (om == 0.5).all()
    p.rank = 2
    om = bad(1, 2, nan)                                                                                     # the caller's array
    keep = om.copy()
    assert lib.somhip_gmlvq_train(cb.h, ds.h, C.byref(p), om.ctypes.data_as(_lib.c_float_p), None, None) != 0
    assert (bits32(om) == bits32(keep)).all()
    p.eps = -1.0
    om = M.default_omega(4, 2)
    assert lib.somhip_gmlvq_train(cb.h, ds.h, C.byref(p), om.ctypes.data_as(_lib.c_float_p), None, None) != 0
    assert (bits32(om) == bits32(M.default_omega(4, 2))).all()
    z6, z4 = np.zeros(6), np.zeros((4, 4))
    for fn, name in ((lambda: E.gmlvq_search(E.Codebook(eng, c), ds), "somhip_gmlvq_search"), (lambda: E.gmlvq_search(cb, ds, bad(0, 0, nan)), "somhip_gmlvq_search"),
                     (lambda: E.gmlvq_search(cb, ds, n=0), "somhip_gmlvq_search"),
                     (lambda: E.gmlvq_project(cb, ds, bad(1, 1, inf)), "somhip_gmlvq_project"), (lambda: E.gmlvq_project(cb, ds, n=0), "somhip_gmlvq_project"),
                     (lambda: E.gmlvq_project(cb, E.Dataset(eng, x[:, :3])), "somhip_gmlvq_project"),
                     (lambda: E.gmlvq_sums(cb, ds, sigmoid_beta=-1.0), "somhip_debug_gmlvq_sums"), (lambda: E.gmlvq_sums(cb, ds, n=0), "somhip_debug_gmlvq_sums"),
                     (lambda: E.gmlvq_sums(cb, ds, bad(0, 1, nan)), "somhip_debug_gmlvq_sums"),
                     (lambda: E.gmlvq_update(cb, 1.0, 0.5, 0, None, np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, z4), "somhip_debug_gmlvq_update"),
                     (lambda: E.gmlvq_update(cb, 1.0, -0.5, 50, None, np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, z4), "somhip_debug_gmlvq_update"),
                     (lambda: E.gmlvq_update(cb, 1.0, 0.5, 50, bad(1, 3, inf), np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, np.zeros((2, 4))), "somhip_debug_gmlvq_update")):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(name + ": "), str(ei.value)
    dp, _, dm, _ = E.gmlvq_search(cb, ds, np.zeros((2, 4), dtype=f32))                                      # the search takes a matrix of zeros
    assert not bits32(dp).any() and not bits32(dm).any()
    assert (bits32(cb.download()) == bits32(c)).all()


@pytest.mark.gpu
def test_timing_counts_the_six_stages(E, eng):
    x, dl, c, cl = TG.clusters(4, 100, 6, 8)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    eng.timing(True); eng.timing_reset()
    E.gmlvq_train(cb, ds, 3, 1.0, 0.5, E.gmlvq_omega(8, 3), stats=False)
    t = eng.gmlvq_timing()
    eng.timing(False)
    assert t["k_gmlvq_project"][0] == 3 * 2 and t["search"][0] == 3 and t["terms"][0] == 3 * 5 and t["sums"][0] == 3
    assert t["k_gmlvq_omega_grad"][0] == 3 and t["k_gmlvq_update"][0] == 3
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


def read_omega(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    m, dim = (int(v) for v in lines[0].split())
    om = np.array([[f32(v) for v in ln.split()] for ln in lines[1:-1]], dtype=f32)
    assert om.shape == (m, dim)
    return om


def read_rows(path, dim):
    text = open(path).read().split("\n")
    assert int(text[0]) == dim
    body = [ln for ln in text[1:] if ln.strip() and not ln.startswith("#")]
    return np.array([[f32(v) for v in ln.split()[:dim]] for ln in body], dtype=f32), [ln.split()[dim] for ln in body]


FINAL = r"final cost ([-+.\deE]+) accuracy ([-+.\deE]+) %"


@pytest.mark.gpu
def test_gmlvq_tool_writes_the_engines_rows_matrix_projection_and_lines(E, eng, tools, tmp_path):
    """the tool on files: the written .cod holds the rows engine.gmlvq_train leaves, -oout its omega float for float, -pout
    engine.gmlvq_project of the data under it, the -v lines alpha_t, eps_t, cost and accuracy per epoch, the final line the
    state it ends with; -oout read back by -oin with -epochs 0 evaluates the written model; the `accuracy` tool on the
    -pout file with the projected codebook gives the printed accuracy"""
    x, dl, c, cl = TG.clusters(21, 120, 9, 5)
    names = ["ape", "bee", "cat"]
    dat, cod, out, oout, pout = tmp_path / "d.dat", tmp_path / "c.cod", tmp_path / "o.cod", tmp_path / "o.om", tmp_path / "p.dat"
    TG.write_dat(dat, x, dl, names)
    TG.write_dat(cod, c, cl, names)
    from som_lvq_pak_amd import textio
    ds = E.Dataset(eng, x, labels=dl)
    start = tmp_path / "start.om"
    om_in = np.random.RandomState(5).uniform(-0.5, 0.5, size=(3, 5)).astype(f32)
    start.write_text(omega_text(om_in))
    for beta, oin, rank in ((0.0, None, None), (0.0, None, 2), (1.5, start, None)):
        opt = (("-sigmoid", beta) if beta else ()) + (("-oin", oin) if oin else ()) + (("-rank", rank) if rank else ())
        p = run("gmlvq", "-din", dat, "-cin", cod, "-cout", out, "-oout", oout, "-pout", pout, "-epochs", 4, "-alpha", 2.5, "-eps", 0.5, "-v", *opt)
        assert p.returncode == 0, p.stderr
        cb = E.Codebook(eng, c, labels=cl)
        om, cost, correct = E.gmlvq_train(cb, ds, 4, 2.5, 0.5, om_in if oin else E.gmlvq_omega(5, rank), beta)
        m = om.shape[0]
        assert m == (3 if oin else rank or 5)
        rows, labels = read_rows(out, 5)
        printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)     # the file is "%g" text
        assert (bits32(rows) == bits32(printed)).all() and labels == [names[int(l)] for l in cl]
        assert (bits32(read_omega(oout)) == bits32(om)).all()
        proj, plabels = read_rows(pout, m)
        assert (bits32(proj) == bits32(E.gmlvq_project(cb, ds, om))).all() and plabels == [names[int(l)] for l in dl]
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("epoch ")]
        assert len(lines) == 4
        for t, ln in enumerate(lines):
            mt = re.match(r"epoch (\d+) alpha ([-+.\deE]+) eps ([-+.\deE]+) cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", ln)
            assert mt and int(mt.group(1)) == t, ln
            assert float(mt.group(2)) == pytest.approx(float(E.glvq_alpha(2.5, 4, t)), rel=1e-7)
            assert float(mt.group(3)) == pytest.approx(float(E.glvq_alpha(0.5, 4, t)), rel=1e-7)
            assert float(mt.group(4)) == pytest.approx(cost[t], rel=1e-9) and float(mt.group(5)) == pytest.approx(100.0 * correct[t] / 120, abs=0.006)
        _, last, right = E.gmlvq_train(cb, ds, 1, 0.0, 0.0, om, beta)
        mf = re.search(FINAL, p.stdout)
        assert mf and float(mf.group(1)) == pytest.approx(last[0], rel=1e-9) and float(mf.group(2)) == pytest.approx(100.0 * right[0] / 120, abs=0.006)
        # the picture: the nearest projected row classifies the projected data as the printed accuracy says
        pcod = tmp_path / "p.cod"
        TG.write_dat(pcod, E.gmlvq_project(cb, None, om), cl, names)
        a = run("accuracy", "-din", pout, "-cin", pcod)
        ma = re.search(r"Total accuracy:\s+(\d+) entries\s+([\d.]+) %", a.stdout)
        assert a.returncode == 0 and ma and int(ma.group(1)) == 120 and float(ma.group(2)) == pytest.approx(float(mf.group(2)), abs=0.006), (a.stdout, a.stderr)
        cb.close()
        # the written model, evaluated: -oout into -oin, no training, no codebook written, -pout still written
        none, pout2 = tmp_path / "none.cod", tmp_path / "p2.dat"
        q = run("gmlvq", "-din", dat, "-cin", out, "-cout", none, "-epochs", 0, "-oin", oout, "-pout", pout2, *(("-sigmoid", beta) if beta else ()))
        assert q.returncode == 0 and not none.exists(), q.stderr
        cb = E.Codebook(eng, rows, labels=cl)
        _, last, right = E.gmlvq_train(cb, ds, 1, 0.0, 0.0, om, beta)
        mq = re.search(FINAL, q.stdout)
        assert mq and float(mq.group(1)) == pytest.approx(last[0], rel=1e-9) and float(mq.group(2)) == pytest.approx(100.0 * right[0] / 120, abs=0.006)
        assert (bits32(read_rows(pout2, m)[0]) == bits32(E.gmlvq_project(cb, ds, om))).all()
        cb.close()
    ds.close()
