"""Batch GRLVQ (K11: somhip_grlvq_train, somhip_grlvq_search and the stages, engine.grlvq_train / grlvq_search / grlvq_sums /
grlvq_update, the grlvq tool) against the numpy replay in grlvq_replay.py.

The weighted search is compared by bit pattern and index.  With the identity the sums, the relevance sums, the relevance
gradient, the update, the relevance step, the cost and whole runs are compared by bit pattern as well: every operation of
the definition is one IEEE rounding and every sum a chain in a fixed order.  With the sigmoid the device's exp and the C
library's may differ by an ulp each, so the sums are compared against the bounds DESIGN.md K9 and K11 derive from that
(glvq_replay.sums_bound, grlvq_replay.rel_bound).  The shapes, the edge cases and the helpers are test_glvq's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glvq_replay as G
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
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("grlvq", "accuracy")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def uniform(dim):
    return np.full(dim, f32(1.0) / f32(dim), dtype=f32)


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.SIGNATURES
    for name in ("somhip_grlvq_train", "somhip_grlvq_search", "somhip_debug_grlvq_sums", "somhip_debug_grlvq_update", "somhip_grlvq_timing"):
        assert hasattr(lib, name) and name in S, name
    assert S["somhip_grlvq_train"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.GrlvqParams), _lib.c_float_p, _lib.c_double_p,
                                                 _lib.c_i64_p])
    assert S["somhip_grlvq_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.GrlvqParams._fields_] == ["epochs", "start_epoch", "count", "first", "n", "alpha", "sigmoid_beta", "eps"]
    assert C.sizeof(_lib.GrlvqParams) == 56
    for name in ("grlvq_train", "grlvq_search", "grlvq_sums", "grlvq_update"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "grlvq_timing")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int somhip_grlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_grlvq_params *p, float *lambda , "
            "double *cost_out , int64_t *correct_out );") in hdr
    assert ("int somhip_grlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *lambda, float *dplus, "
            "int32_t *iplus, float *dminus, int32_t *iminus);") in hdr
    assert "int somhip_grlvq_timing(somhip_engine *e, int64_t launches[5], double total_ms[5]);" in hdr
    m = re.search(r"typedef struct somhip_grlvq_params \{(.*?)\} somhip_grlvq_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int64_t epochs; int64_t start_epoch, count; int64_t first, n; float alpha; "
                                                            "float sigmoid_beta; float eps;")


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 5)(), (C.c_double * 5)()
    assert lib.somhip_grlvq_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_grlvq_timing: null engine"


def test_replay_with_unit_relevances_is_the_glvq_replay():
    """lambda all 1.0f and eps 0: the weighted chain is the unweighted one and the step has the factor 1.0, so rows, cost
    and count are glvq_replay's by bit pattern, and lambda keeps its bits"""
    x, dl, c, cl = R.learning_case(4)
    one = np.ones(8, dtype=f32)
    rows, lam, cost, correct = R.train(c, cl, x, dl, one, 3, 10.0, 0.0, first=5, n=500)
    grows, gcost, gcorrect = G.train(c, cl, x, dl, 3, 10.0, first=5, n=500)
    assert (bits32(rows) == bits32(grows)).all() and (bits64(cost) == bits64(gcost)).all() and (correct == gcorrect).all()
    assert (bits32(lam) == bits32(one)).all()
    assert (bits32(R.dist_weighted(c, x, one)) == bits32(G.dist_sq(c, x))).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replay_learns_the_relevances(seed):
    """the definition itself, on the CPU: two informative components of eight, the others noise of standard deviation 3.
    With eps 0.5 the cost falls by more than 0.3, the two informative components end with more than 0.9 of the relevance
    and the accuracy above 0.8; with eps 0 (batch GLVQ under lambda = 1/8) the accuracy stays below 0.7"""
    x, dl, c, cl = R.learning_case(seed)
    rows, lam, cost, _ = R.train(c, cl, x, dl, uniform(8), 40, 10.0, 0.5)
    last, acc = R.evaluate(rows, cl, x, dl, lam)
    print("seed %d: cost %.4f -> %.4f, lambda %s, accuracy %.3f" % (seed, cost[0], last, lam, acc))
    assert cost[0] - last > 0.3 and lam[0] + lam[1] > 0.9 and acc > 0.8
    assert abs(float(lam.astype(f64).sum()) - 1.0) < 1e-6 and (lam >= 0).all()
    rows0, lam0, _, _ = R.train(c, cl, x, dl, uniform(8), 40, 10.0, 0.0)
    assert (bits32(lam0) == bits32(uniform(8))).all()
    assert R.evaluate(rows0, cl, x, dl, lam0)[1] < 0.7


def test_weighted_scan_is_exact_and_spill_free(built, tmp_path):
    """k_scan_class_weighted forms its distances by sub, mul, mul, add with four roundings: no contracted v_fma / v_fmac /
    v_mac / v_mad in its gfx950 ISA, twice as many multiplications as subtractions, and its register tiles stay in
    registers: no scratch, no spills, in both instantiations"""
    s = os.path.join(str(tmp_path), "k.s")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                          "--cuda-device-only", "-S", "-o", s, "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")], stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    txt = open(s).read()
    bodies = dict(re.findall(r"^(_ZN6somhip21k_scan_class_weighted\w+):.*?\n(.*?)s_endpgm", txt, flags=re.S | re.M))
    assert len(bodies) == 2, sorted(bodies)
    for name, body in bodies.items():
        bad = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)_f32\b.*", body)
        assert not bad, (name, bad[:3])
        subs, muls, adds = (len(re.findall(r"\bv_%s_f32" % op, body)) for op in ("sub(?:rev)?", "mul", "add"))
        assert subs >= 128 and adds >= subs and muls >= 2 * subs, (name, subs, muls, adds)
        assert "scratch_" not in body, name
        m = re.search(r"Function Name: %s\b.*?LDS Size" % re.escape(name), res.stderr, flags=re.S)
        assert m, "no resource remark for " + name
        rem = m.group(0)
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem) and re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem


def test_grlvq_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("grlvq", "-help")
    assert p.returncode == 0 and p.stdout.startswith("grlvq - ") and all(w in p.stdout for w in ("-epochs", "-alpha", "-eps", "-sigmoid", "-rin", "-rout"))
    cod, dat, out, rout = tmp_path / "c.cod", tmp_path / "d.dat", tmp_path / "o.cod", tmp_path / "o.rel"
    cod.write_text("2\n0 0 a\n1 1 b\n")
    dat.write_text("2\n0.25 0.5 a\n0.75 0.5 b\n")
    for args, word in ((("-epochs", -2, "-alpha", 1, "-eps", 1), "-epochs"), (("-epochs", 0), "-epochs 0"),
                       (("-epochs", 2, "-alpha", -1, "-eps", 1), "-alpha"), (("-epochs", 2, "-alpha", "nan", "-eps", 1), "-alpha"),
                       (("-epochs", 2, "-alpha", 1, "-eps", -1), "-eps"), (("-epochs", 2, "-alpha", 1, "-eps", "nan"), "-eps"),
                       (("-epochs", 2, "-alpha", 1, "-eps", 1, "-sigmoid", -1), "-sigmoid"),
                       (("-epochs", 2, "-alpha", 1, "-eps", 1, "-sigmoid", "nan"), "-sigmoid")):
        p = run("grlvq", "-cin", cod, "-din", dat, "-cout", out, "-rout", rout, *args)
        assert p.returncode == 1 and p.stderr.startswith("grlvq: " + word), (args, p.stderr)
    good = ("-epochs", 2, "-alpha", 1, "-eps", 0.5)
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3 a\n4 5 6 b\n")
    p = run("grlvq", "-cin", cod, "-din", dim3, "-cout", out, *good)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    for name, text, word in (("x.cod", "2\nx 0 a\n1 1 b\n", "masked components"), ("x.dat", "2\nx 0.5 a\n0.75 0.5 b\n", "masked components"),
                             ("n.cod", "2\n0 0\n1 1\n", "no labels"), ("n.dat", "2\n0.25 0.5\n0.75 0.5\n", "no labels"),
                             ("one.cod", "2\n0 0 a\n1 1 a\n", "one label"), ("z.dat", "2\n0.25 0.5 a\n0.75 0.5 z\n", "no codebook row")):
        f = tmp_path / name
        f.write_text(text)
        p = run("grlvq", "-cin", f if name.endswith(".cod") else cod, "-din", f if name.endswith(".dat") else dat, "-cout", out, *good)
        assert p.returncode == 1 and word in p.stderr, (name, p.stderr)
    for text, word in (("3\n1\n1\n1\n", "has dimension 3, the codebook 2"), ("2\n1\n-0.5\n", "negative or not a finite number"),
                       ("2\n1\nnan\n", "negative or not a finite number"), ("2\n1\ninf\n", "negative or not a finite number"),
                       ("2\n1\nabc\n", "can't read value 1"), ("2\n1\n", "ends after 1 of 2 values"), ("two\n1\n1\n", "dimension"),
                       ("", "is empty"), ("2\n0\n0\n", "sum to zero")):
        rin = tmp_path / "bad.rel"
        rin.write_text(text)
        p = run("grlvq", "-cin", cod, "-din", dat, "-cout", out, "-rout", rout, "-rin", rin, *good)
        assert p.returncode == 1 and p.stderr.startswith("grlvq: ") and word in p.stderr, (text, p.stderr)
    p = run("grlvq", "-cin", cod, "-din", dat, "-cout", out, "-rin", tmp_path / "none.rel", *good)
    assert p.returncode == 1 and "can't open relevance file" in p.stderr
    assert not out.exists() and not rout.exists()


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


def lambdas(seed, c, cl):
    """The relevance vectors of a search case, by name; `c` gets rows that coincide under the vector with zeros: a pair
    within a class and a pair across two classes that differ only where lambda is 0, so the lowest row must win"""
    dim = c.shape[1]
    rs = np.random.RandomState(seed)
    out = {"random": rs.uniform(0.05, 2.0, size=dim).astype(f32), "ones": np.ones(dim, dtype=f32), "all zero": np.zeros(dim, dtype=f32)}
    z = rs.uniform(0.5, 1.5, size=dim).astype(f32)
    z[::2] = 0.0
    out["zeros"] = z
    if c.shape[0] >= 8:
        a = 2
        same = np.flatnonzero(cl == cl[a])
        diff = np.flatnonzero(cl != cl[a])
        if len(same) > 2:
            c[same[-1], 1::2] = c[a, 1::2]
        c[diff[len(diff) // 2], 1::2] = c[a, 1::2]
    big = rs.uniform(0.5, 1.5, size=dim).astype(f32)
    big[rs.randint(0, dim)] = f32(1e6)
    big[rs.randint(0, dim)] = f32(1e-30)
    if dim >= 3:
        big[0], big[dim - 1] = f32(1e6), f32(1e-30)
    out["1e6 and 1e-30"] = big
    return out


SEARCH_SHAPES = [(2, 1, 1, 2), (2, 4, 33, 2), (63, 3, 31, 3), (64, 4, 32, 4), (65, 5, 33, 5), (64, 64, 700, 7), (1030, 129, 700, 7),
                 (1030, 4, 32, 2), (65, 129, 31, 2), (1030, 1, 700, 4), (63, 64, 1, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,classes", SEARCH_SHAPES)
def test_weighted_search_equals_the_replay(E, eng, rows, dim, n, classes):
    """rows at the lane, group and 4-groups-per-wave edges, dims around the float4 and 128 edges, runs around the 32-sample
    tile, 2 to 7 classes with test_glvq.edge_case's single-row class and class behind the last full group; plain and
    wrapped ranges; lambda random, with zeros, with 1e6 and 1e-30 entries, all zero, and all 1.0f, where the search is
    somhip_debug_glvq_search on the direct route bit for bit; every call twice"""
    n_data = max(n, 5) if n != 700 else 300                         # 700 samples of 300 rows: the run wraps twice
    c, cl, x, dl = TG.edge_case(2000 + rows + dim, rows, dim, n_data, classes)
    lams = lambdas(rows * 131 + dim, c, cl)
    cb = E.Codebook(eng, c, labels=cl)
    ds = E.Dataset(eng, x, labels=dl)
    for first in (0, n_data - 2):                                    # the second range wraps after two rows
        for name, lam in lams.items():
            want = R.search(c, cl, x, dl, lam, first, n)
            for again in range(2):
                dp, ip, dm, im = E.grlvq_search(cb, ds, lam, first, n)
                assert (ip == want[1]).all() and (im == want[3]).all(), (name, first, np.flatnonzero((ip != want[1]) | (im != want[3]))[:5])
                assert (bits32(dp) == bits32(want[0])).all() and (bits32(dm) == bits32(want[2])).all(), (name, first)
            if name == "all zero":
                assert not bits32(dp).any() and not bits32(dm).any()
            if name == "ones":
                plain = E.glvq_search(cb, ds, first, n, E.GLVQ_DIRECT)
                assert all((bits32(a) == bits32(b)).all() for a, b in zip((dp, ip, dm, im), plain[:4]))
    cb.close(); ds.close()


def sums_case(seed, rows, dim, n, one):
    """test_glvq.sums_case with duplicated samples and a sample equal to rows of two classes (D == 0 under any lambda),
    and a relevance vector with a zero, a large and a small entry"""
    c, cl, x, dl = TG.sums_case(seed, rows, dim, n, one_winner=one)
    x[5] = x[4]; dl[5] = dl[4]
    x[n // 2] = x[4]; dl[n // 2] = dl[4]
    other = int(np.flatnonzero(cl != cl[0])[0])
    c[other] = c[0]
    x[7] = c[0]
    lam = np.random.RandomState(seed + 1).uniform(0.1, 1.5, size=dim).astype(f32)
    lam[dim // 2] = 0.0
    if dim > 2:
        lam[0], lam[dim - 1] = f32(40.0), f32(1e-3)
    return c, cl, x, dl, lam


SUMS_SHAPES = [(12, 16, 300, False), (5, 63, 150, False), (5, 64, 150, False), (5, 65, 150, False), (7, 3, 200, True), (256, 5, 20, False),
               (70, 129, 97, False)]


def replay_sums(c, cl, x, dl, lam, first, n, beta=0.0):
    dp, ip, dm, im = R.search(c, cl, x, dl, lam, first, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im, beta)
    return R.sums(c, x, ip, im, xp, xm, f, first), xp, xm, f, correct, (dp, dm)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,one", SUMS_SHAPES)
def test_identity_sums_and_relevance_gradient_equal_the_replay_bit_for_bit(E, eng, rows, dim, n, one):
    """all samples on one prototype, most prototypes unchosen, duplicated samples, a sample with D == 0, lists crossing 64
    columns at dims 63 / 64 / 65: xi, f, Sp, Sm, sp, sm, cost, the counts, Rp, Rm and G"""
    c, cl, x, dl, lam = sums_case(rows * 7 + dim, rows, dim, n, one)
    first = 11
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.grlvq_sums(cb, ds, lam, first, n)
    S, xp, xm, f, correct, (dp, dm) = replay_sums(c, cl, x, dl, lam, first, n)
    assert ((dp.astype(f64) + dm.astype(f64)) == 0).any() and (xp == 0).any()               # the D == 0 sample is there
    assert (bits64(got["xi_plus"]) == bits64(xp)).all() and (bits64(got["xi_minus"]) == bits64(xm)).all() and (bits64(got["f"]) == bits64(f)).all()
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    for key in ("sums_plus", "sums_minus", "cost", "rel_plus", "rel_minus", "grad"):
        assert (bits64(got[key]) == bits64(S[key])).all(), key
    if one:
        assert got["n_plus"][rows // 2] == n and got["n_plus"].sum() == n
    if rows == 256:
        assert ((got["n_plus"] == 0) & (got["n_minus"] == 0)).sum() > 200
    again = E.grlvq_sums(cb, ds, lam, first, n)
    assert (bits64(again["rel_minus"]) == bits64(got["rel_minus"])).all() and (bits64(again["grad"]) == bits64(got["grad"])).all()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,beta", [(12, 16, 300, 2.0), (5, 65, 150, 0.5), (256, 5, 20, 4.0)])
def test_sigmoid_sums_within_the_derived_bounds(E, eng, rows, dim, n, beta):
    c, cl, x, dl, lam = sums_case(rows + dim, rows, dim, n, False)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.grlvq_sums(cb, ds, lam, 0, n, beta)
    S, xp, xm, f, correct, _ = replay_sums(c, cl, x, dl, lam, 0, n, beta)
    rel = G.xi_rel_bound(beta)
    worst = {}
    for name, ref, tol in (("xi_plus", xp, rel * xp), ("xi_minus", xm, rel * xm), ("f", f, G.F_REL_BOUND * f)):
        err = np.abs(got[name] - ref)
        worst[name] = float((err / np.maximum(tol, 1e-300)).max())
        assert (err <= tol).all(), (name, worst)
    bp, bm, bc = G.sums_bound(S, beta)
    rp, rm, rg = R.rel_bound(S, beta)
    for name, tol in (("sums_plus", bp), ("sums_minus", bm), ("cost", bc), ("rel_plus", rp), ("rel_minus", rm), ("grad", rg)):
        err = np.abs(got[name] - S[name])
        worst[name] = float((err / tol).max())
        assert (err <= tol).all(), (name, worst)
    print("largest error / bound:", worst)
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n", [(12, 16, 300), (70, 129, 97), (256, 5, 20)])
def test_update_and_relevance_step_from_host_sums_equal_the_replay(E, eng, rows, dim, n):
    """the rows and lambda by bit pattern from host-supplied sums and gradients: an ordinary step; a component clamped to 0;
    every component clamped (lambda keeps its bits); eps_t == 0 (no step, no normalisation of a lambda that sums to
    something else); a lambda[k] == 0 column and the rows no sample chose keep their bits"""
    c, cl, x, dl, lam = sums_case(rows + 3 * dim, rows, dim, n, False)
    assert lam[dim // 2] == 0 and abs(float(lam.sum()) - 1.0) > 0.1
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.grlvq_sums(cb, ds, lam, 0, n)
    unchosen = (got["n_plus"] == 0) & (got["n_minus"] == 0)
    alpha_t, eps_t = R.rate_at(7.5, 9, 2), R.rate_at(0.5, 9, 2)
    scale = 2.0 * n / float(eps_t)
    one_clamped = got["grad"].copy()
    one_clamped[1 % dim] = 3.0 * scale
    cases = (("plain", got["grad"], eps_t, None), ("one clamped", one_clamped, eps_t, 1 % dim), ("all clamped", np.full(dim, 100.0 * scale), eps_t, None),
             ("eps 0", got["grad"], f32(0.0), None))
    for name, grad, e_t, zeroed in cases:
        cb.upload(c)
        after = E.grlvq_update(cb, alpha_t, e_t, n, lam, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"], grad)
        want = R.relevance_step(lam, grad, e_t, n)
        assert (bits32(after) == bits32(want)).all(), name
        if name in ("all clamped", "eps 0"):
            assert (bits32(after) == bits32(lam)).all(), name
        else:
            assert abs(float(after.astype(f64).sum()) - 1.0) < 1e-6 and (after >= 0).all() and (bits32(after) != bits32(lam)).any(), name
        if zeroed is not None:
            assert after[zeroed] == 0 and lam[zeroed] > 0
        rows_after = cb.download()
        assert (bits32(rows_after) == bits32(R.update(c, got, lam, alpha_t, n))).all(), name
        assert (bits32(rows_after[:, dim // 2]) == bits32(c[:, dim // 2])).all()           # the column lambda gives no weight
        assert (bits32(rows_after[unchosen]) == bits32(c[unchosen])).all()
        assert (bits32(rows_after) != bits32(c)).any()
    if rows == 256:
        assert unchosen.sum() > 200
    cb.close(); ds.close()


@pytest.mark.gpu
def test_unit_relevances_without_a_rate_are_batch_glvq(E, eng):
    """lambda all 1.0f with eps 0 over 3 epochs: codebook, cost and count are somhip_glvq_train's bit for bit, lambda keeps
    its bits"""
    x, dl, c, cl = TG.clusters(9, 400, 12, 16)
    first, n = 7, 390
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    gcost, gcorrect = E.glvq_train(cb, ds, 3, 10.0, first=first, n=n)
    grows = cb.download()
    cb.upload(c)
    lam, cost, correct = E.grlvq_train(cb, ds, 3, 10.0, 0.0, np.ones(16, dtype=f32), first=first, n=n)
    assert (bits32(cb.download()) == bits32(grows)).all() and (bits64(cost) == bits64(gcost)).all() and (correct == gcorrect).all()
    assert (bits32(lam) == bits32(np.ones(16, dtype=f32))).all() and (bits32(grows) != bits32(c)).any()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 2.0])
def test_runs(E, eng, beta):
    """5 epochs in one call equal five calls handing lambda on and equal themselves run twice; an epoch equals its stages;
    rows, lambda, cost and correct equal the replay's (by bit pattern with the identity)"""
    x, dl, c, cl = TG.clusters(9, 400, 12, 16)
    first, n, T, alpha, eps = 7, 390, 5, 10.0, 0.5
    lam0 = np.random.RandomState(2).uniform(0.02, 0.1, size=16).astype(f32)              # not normalised: taken as it is
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    lam, cost, correct = E.grlvq_train(cb, ds, T, alpha, eps, lam0, beta, first=first, n=n)
    one = cb.download()
    assert (bits32(lam) != bits32(lam0)).any() and abs(float(lam.astype(f64).sum()) - 1.0) < 1e-6
    cb.upload(c)
    lam2, cost2, correct2 = E.grlvq_train(cb, ds, T, alpha, eps, lam0, beta, first=first, n=n)
    assert (bits32(cb.download()) == bits32(one)).all() and (bits64(cost2) == bits64(cost)).all() and (correct2 == correct).all()
    assert (bits32(lam2) == bits32(lam)).all()
    cb.upload(c)
    l = lam0
    for t in range(T):
        l, ct, rt = E.grlvq_train(cb, ds, T, alpha, eps, l, beta, start_epoch=t, count=1, first=first, n=n)
        assert bits64(ct)[0] == bits64(cost)[t] and rt[0] == correct[t]
    assert (bits32(cb.download()) == bits32(one)).all() and (bits32(l) == bits32(lam)).all()
    cb.upload(c)
    l = lam0
    for t in range(T):                                               # an epoch is its stages
        got = E.grlvq_sums(cb, ds, l, first, n, beta)
        chain = f64(0.0)
        for v in got["cost"]:
            chain = chain + v
        assert bits64(chain / f64(n))[()] == bits64(cost)[t] and got["correct"] == correct[t]
        l = E.grlvq_update(cb, E.glvq_alpha(alpha, T, t), E.glvq_alpha(eps, T, t), n, l, got["sums_plus"], got["n_plus"], got["sums_minus"],
                           got["n_minus"], got["grad"])
    assert (bits32(cb.download()) == bits32(one)).all() and (bits32(l) == bits32(lam)).all()
    rows, rlam, rcost, rcorrect = R.train(c, cl, x, dl, lam0, T, alpha, eps, beta, first, n)
    if beta == 0.0:
        assert (bits32(one) == bits32(rows)).all() and (bits64(cost) == bits64(rcost)).all() and (bits32(lam) == bits32(rlam)).all()
    else:
        assert np.allclose(one, rows, rtol=0, atol=1e-5) and np.allclose(cost, rcost, rtol=1e-12, atol=0) and np.allclose(lam, rlam, rtol=0, atol=1e-6)
    assert (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_learning_finds_the_informative_components(E, eng, seed):
    """three classes separated in 2 of 8 components, six noise components of standard deviation 3, 600 samples, 6
    prototypes, T = 40, alpha = 10, eps = 0.5 from lambda = 1/8: the cost falls by more than 0.3, components 0 and 1 end
    with more than 0.9 of the relevance, the accuracy ends above 0.8 -- and the eps = 0 run on the same data below 0.7.
    (The replay gave falls of 0.68 to 0.70, a share of 1.000 and accuracies from 0.89 on these seeds.)"""
    x, dl, c, cl = R.learning_case(seed)
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    lam, cost, correct = E.grlvq_train(cb, ds, 40, 10.0, 0.5)
    _, last, right = E.grlvq_train(cb, ds, 1, 0.0, 0.0, lam)                             # the state the run ended with
    print("seed %d: cost %.4f -> %.4f, lambda %s, accuracy %.3f" % (seed, cost[0], last[0], lam, right[0] / 600))
    assert cost[0] - last[0] > 0.3
    assert float(lam[0]) + float(lam[1]) > 0.9
    assert right[0] / 600 > 0.8
    dp, ip, dm, im = E.grlvq_search(cb, ds, lam)
    assert int(((dp < dm) | ((dp == dm) & (ip < im))).sum()) == right[0]                  # the public search evaluates the model
    rows, rlam, rcost, _ = R.train(c, cl, x, dl, uniform(8), 40, 10.0, 0.5)
    assert (bits32(cb.download()) == bits32(rows)).all() and (bits32(lam) == bits32(rlam)).all() and (bits64(cost) == bits64(rcost)).all()
    cb.upload(c)
    lam0, _, _ = E.grlvq_train(cb, ds, 40, 10.0, 0.0)
    assert (bits32(lam0) == bits32(uniform(8))).all()
    _, _, right0 = E.grlvq_train(cb, ds, 1, 0.0, 0.0, lam0)
    assert right0[0] / 600 < 0.7
    cb.close(); ds.close()


@pytest.mark.gpu
def test_refusals_name_the_entry_point_and_leave_rows_and_lambda(E, eng):
    x, dl, c, cl = TG.clusters(3, 50, 6, 4)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    mask = np.zeros(x.shape, dtype=np.uint8); mask[3, 1] = 1
    nan, inf = float("nan"), float("inf")
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
        (cb, ds, dict(lam=[0.25, -0.25, 0.5, 0.5]), "lambda[1]"), (cb, ds, dict(lam=[0.25, 0.25, nan, 0.5]), "lambda[2]"),
        (cb, ds, dict(lam=[0.25, 0.25, 0.5, inf]), "lambda[3]"), (cb, ds, dict(lam=[0.0, 0.0, 0.0, 0.0]), "lambda sums to zero"),
    ]
    for book, data, kw, word in cases:
        args = dict(epochs=5, alpha=1.0, eps=0.5)
        args.update(kw)
        with pytest.raises(Exception) as ei:
            E.grlvq_train(book, data, **args)
        assert str(ei.value).startswith("somhip_grlvq_train: ") and word in str(ei.value), (kw, str(ei.value))
        assert (bits32(book.download()) == bits32(c[:book.n])).all()
    from som_lvq_pak_amd import _lib
    p = _lib.GrlvqParams(5, 0, 5, 0, 50, 1.0, 0.0, 0.5)
    assert cb.e.lib.somhip_grlvq_train(cb.h, ds.h, C.byref(p), None, None, None) != 0                      # a NULL lambda
    assert cb.e.lib.somhip_last_error().decode() == "somhip_grlvq_train: null lambda"
    lam = np.array([0.25, 0.25, nan, 0.5], dtype=f32)                                                   # the caller's array, through the ABI
    keep = lam.copy()
    assert cb.e.lib.somhip_grlvq_train(cb.h, ds.h, C.byref(p), lam.ctypes.data_as(_lib.c_float_p), None, None) != 0
    assert (bits32(lam) == bits32(keep)).all()
    p.eps = -1.0
    lam = uniform(4)
    assert cb.e.lib.somhip_grlvq_train(cb.h, ds.h, C.byref(p), lam.ctypes.data_as(_lib.c_float_p), None, None) != 0
    assert (bits32(lam) == bits32(uniform(4))).all()
    z6, z4 = np.zeros(6), np.zeros(4)
    for fn, name in ((lambda: E.grlvq_search(E.Codebook(eng, c), ds), "somhip_grlvq_search"), (lambda: E.grlvq_search(cb, ds, [1, 1, -1, 1]), "somhip_grlvq_search"),
                     (lambda: E.grlvq_search(cb, ds, n=0), "somhip_grlvq_search"),
                     (lambda: E.grlvq_sums(cb, ds, sigmoid_beta=-1.0), "somhip_debug_grlvq_sums"), (lambda: E.grlvq_sums(cb, ds, n=0), "somhip_debug_grlvq_sums"),
                     (lambda: E.grlvq_sums(cb, ds, [1, nan, 1, 1]), "somhip_debug_grlvq_sums"),
                     (lambda: E.grlvq_update(cb, 1.0, 0.5, 0, None, np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, z4), "somhip_debug_grlvq_update"),
                     (lambda: E.grlvq_update(cb, 1.0, -0.5, 50, None, np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, z4), "somhip_debug_grlvq_update"),
                     (lambda: E.grlvq_update(cb, 1.0, 0.5, 50, [1, 1, inf, 1], np.zeros((6, 5)), z6, np.zeros((6, 5)), z6, z4), "somhip_debug_grlvq_update")):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(name + ": "), str(ei.value)
    assert (bits32(cb.download()) == bits32(c)).all()


@pytest.mark.gpu
def test_timing_counts_the_five_stages(E, eng):
    x, dl, c, cl = TG.clusters(4, 100, 6, 8)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    eng.timing(True); eng.timing_reset()
    E.grlvq_train(cb, ds, 3, 1.0, 0.5, stats=False)
    t = eng.grlvq_timing()
    eng.timing(False)
    assert t["search"][0] == 3 and t["terms"][0] == 3 * 5 and t["k_grlvq_sums"][0] == 3 and t["k_grlvq_relevance"][0] == 3 and t["k_grlvq_update"][0] == 3
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


def read_relevances(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    vals = np.array([f32(v) for v in lines[1:-1]], dtype=f32)
    assert int(lines[0]) == len(vals)
    return vals


def read_rows(path, dim):
    text = open(path).read().split("\n")
    body = [ln for ln in text[1:] if ln.strip() and not ln.startswith("#")]
    return np.array([[float(v) for v in ln.split()[:dim]] for ln in body], dtype=f32), [ln.split()[dim] for ln in body]


FINAL = r"final cost ([-+.\deE]+) accuracy ([-+.\deE]+) %"


@pytest.mark.gpu
def test_grlvq_tool_writes_the_engines_rows_relevances_and_lines(E, eng, tools, tmp_path):
    """the tool on files: the written .cod holds the rows engine.grlvq_train leaves, -rout its lambda float for float, the
    -v lines its alpha_t, eps_t, cost and accuracy per epoch, the final line the state it ends with; -rout read back by
    -rin with -epochs 0 evaluates the written model; with a file of ones -epochs 0 gives the `accuracy` tool's figure"""
    x, dl, c, cl = TG.clusters(21, 120, 9, 5)
    names = ["ape", "bee", "cat"]
    dat, cod, out, rel = tmp_path / "d.dat", tmp_path / "c.cod", tmp_path / "o.cod", tmp_path / "o.rel"
    TG.write_dat(dat, x, dl, names)
    TG.write_dat(cod, c, cl, names)
    from som_lvq_pak_amd import textio
    ds = E.Dataset(eng, x, labels=dl)
    start = tmp_path / "start.rel"
    lam_in = np.array([0.3, 0.1, 0.25, 0.05, 0.7], dtype=f32)
    start.write_text("5\n" + "".join("%.9g\n" % float(v) for v in lam_in))
    for beta, rin in ((0.0, None), (1.5, start)):
        opt = (("-sigmoid", beta) if beta else ()) + (("-rin", rin) if rin else ())
        p = run("grlvq", "-din", dat, "-cin", cod, "-cout", out, "-rout", rel, "-epochs", 4, "-alpha", 2.5, "-eps", 0.5, "-v", *opt)
        assert p.returncode == 0, p.stderr
        cb = E.Codebook(eng, c, labels=cl)
        lam, cost, correct = E.grlvq_train(cb, ds, 4, 2.5, 0.5, lam_in if rin else None, beta)
        rows, labels = read_rows(out, 5)
        printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)     # the file is "%g" text
        assert (bits32(rows) == bits32(printed)).all() and labels == [names[int(l)] for l in cl]
        assert (bits32(read_relevances(rel)) == bits32(lam)).all()
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("epoch ")]
        assert len(lines) == 4
        for t, ln in enumerate(lines):
            m = re.match(r"epoch (\d+) alpha ([-+.\deE]+) eps ([-+.\deE]+) cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", ln)
            assert m and int(m.group(1)) == t, ln
            assert float(m.group(2)) == pytest.approx(float(E.glvq_alpha(2.5, 4, t)), rel=1e-7)
            assert float(m.group(3)) == pytest.approx(float(E.glvq_alpha(0.5, 4, t)), rel=1e-7)
            assert float(m.group(4)) == pytest.approx(cost[t], rel=1e-9) and float(m.group(5)) == pytest.approx(100.0 * correct[t] / 120, abs=0.006)
        _, last, right = E.grlvq_train(cb, ds, 1, 0.0, 0.0, lam, beta)
        m = re.search(FINAL, p.stdout)
        assert m and float(m.group(1)) == pytest.approx(last[0], rel=1e-9) and float(m.group(2)) == pytest.approx(100.0 * right[0] / 120, abs=0.006)
        cb.close()
        # the written model, evaluated: -rout into -rin, no training, no codebook written
        none = tmp_path / "none.cod"
        q = run("grlvq", "-din", dat, "-cin", out, "-cout", none, "-epochs", 0, "-rin", rel, *(("-sigmoid", beta) if beta else ()))
        assert q.returncode == 0 and not none.exists(), q.stderr
        cb = E.Codebook(eng, rows, labels=cl)
        _, last, right = E.grlvq_train(cb, ds, 1, 0.0, 0.0, lam, beta)
        m = re.search(FINAL, q.stdout)
        assert m and float(m.group(1)) == pytest.approx(last[0], rel=1e-9) and float(m.group(2)) == pytest.approx(100.0 * right[0] / 120, abs=0.006)
        cb.close()
    ones = tmp_path / "ones.rel"
    ones.write_text("5\n1\n1\n1\n1\n1\n")
    q = run("grlvq", "-din", dat, "-cin", cod, "-epochs", 0, "-rin", ones)
    a = run("accuracy", "-din", dat, "-cin", cod)
    assert q.returncode == 0 and a.returncode == 0, (q.stderr, a.stderr)
    m, ma = re.search(FINAL, q.stdout), re.search(r"Total accuracy:\s+(\d+) entries\s+([\d.]+) %", a.stdout)
    assert m and ma and int(ma.group(1)) == 120 and float(m.group(2)) == pytest.approx(float(ma.group(2)), abs=0.006), (q.stdout, a.stdout)
    ds.close()
