"""Batch GLVQ (K9: somhip_glvq_train and its stages, engine.glvq_train / glvq_search / glvq_sums / glvq_update, the glvq
tool) against the numpy replay in glvq_replay.py.

The search is compared by bit pattern and index on both routes.  With the identity the terms, the sums, the update, the
cost and whole runs are compared by bit pattern as well: every operation of the definition is one IEEE rounding, and the
sums are chains in data order.  With the sigmoid the device's exp and the C library's may differ by an ulp each, so xi, f
and the sums are compared against the bounds DESIGN.md K9 derives from that (glvq_replay.xi_rel_bound, sums_bound), and
the update against a np.longdouble replay with ulp32 / 2 plus those bounds carried through."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glvq_replay as R
from conftest import ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("glvq", "accuracy")):
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


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    S = _lib.SIGNATURES
    for name in ("somhip_glvq_train", "somhip_debug_glvq_plan", "somhip_debug_glvq_search", "somhip_debug_glvq_sums",
                 "somhip_debug_glvq_update", "somhip_glvq_timing"):
        assert hasattr(lib, name) and name in S, name
    assert S["somhip_glvq_train"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.GlvqParams), _lib.c_double_p, _lib.c_i64_p])
    assert S["somhip_glvq_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert [f[0] for f in _lib.GlvqParams._fields_] == ["epochs", "start_epoch", "count", "first", "n", "alpha", "sigmoid_beta"]
    assert C.sizeof(_lib.GlvqParams) == 48
    for name in ("glvq_train", "glvq_search", "glvq_sums", "glvq_update", "glvq_plan", "glvq_alpha"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Engine, "glvq_timing")
    assert lib.somhip_version() == 1


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int somhip_glvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_glvq_params *p, double *cost_out , "
            "int64_t *correct_out );") in hdr
    assert "int somhip_glvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]);" in hdr
    m = re.search(r"typedef struct somhip_glvq_params \{(.*?)\} somhip_glvq_params;", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int64_t epochs; int64_t start_epoch, count; int64_t first, n; float alpha; "
                                                            "float sigmoid_beta;")


def test_null_engine_timing_is_an_error(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    n, ms = (C.c_int64 * 4)(), (C.c_double * 4)()
    assert lib.somhip_glvq_timing(None, n, ms) != 0
    assert lib.somhip_last_error().decode() == "somhip_glvq_timing: null engine"


def test_plan_is_host_arithmetic(built):
    """one function of (rows, dim, n): the list route where its worst case is cheap -- the top-8 search's two-level
    pre-filter (512 row groups), rows of 512 components and more, runs of at least one sample tile -- and the class-wise
    scan alone everywhere else, the two bench shapes among them; it answers without a GPU and refuses nonsense"""
    from som_lvq_pak_amd import engine as E
    assert E.glvq_plan(10000, 256, 100000) == E.GLVQ_DIRECT and E.glvq_plan(100000, 1024, 100000) == E.GLVQ_LIST
    for rows, dim, n, want in ((32767, 512, 100, E.GLVQ_DIRECT), (32768, 512, 100, E.GLVQ_LIST), (32768, 511, 100, E.GLVQ_DIRECT),
                               (100000, 1024, 31, E.GLVQ_DIRECT), (100000, 1024, 32, E.GLVQ_LIST), (12, 16, 2000, E.GLVQ_DIRECT)):
        assert E.glvq_plan(rows, dim, n) == want, (rows, dim, n)
    for bad in ((0, 4, 10), (10, 0, 10), (10, 4, 0)):
        with pytest.raises(Exception, match="somhip_debug_glvq_plan"):
            E.glvq_plan(*bad)


def test_replay_cost_falls_every_epoch():
    """the definition itself, on the CPU: three Gaussian classes, 2000 samples, 12 prototypes, dim 16, alpha 10 -- the cost
    falls every epoch of 20 and ends below where it started, identity and sigmoid"""
    x, dl, c, cl = clusters(5, 2000, 12, 16)
    for beta in (0.0, 2.0):
        rows, cost, correct = R.train(c, cl, x, dl, 20, 10.0, beta)
        after = R.epoch(rows, cl, x, dl, 0.0, beta)[1]
        assert (np.diff(np.append(cost, after)) < 0).all(), (beta, cost, after)
        assert correct[-1] > correct[0]


def test_scan_class_is_exact_and_spill_free(built, tmp_path):
    """k_scan_class forms its distances by sub, mul, add with three roundings: no contracted v_fma / v_fmac / v_mac / v_mad
    in its gfx950 ISA (as test_exact_kernels_have_no_fma asks of K1), and its register tiles stay in registers: no
    scratch, no spills, in both instantiations"""
    s = os.path.join(str(tmp_path), "k.s")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                          "--cuda-device-only", "-S", "-o", s, "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")], stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    txt = open(s).read()
    bodies = dict(re.findall(r"^(_ZN6somhip12k_scan_class\w+):.*?\n(.*?)s_endpgm", txt, flags=re.S | re.M))
    assert len(bodies) == 2, sorted(bodies)
    for name, body in bodies.items():
        bad = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)_f32\b.*", body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_(pk_)?mul_f32", body) and re.search(r"v_(pk_)?add_f32", body) and re.search(r"v_(pk_)?sub(rev)?_f32", body)
        assert "scratch_" not in body, name
        m = re.search(r"Function Name: %s\b.*?LDS Size" % re.escape(name), res.stderr, flags=re.S)
        assert m, "no resource remark for " + name
        rem = m.group(0)
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem) and re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem


def write_dat(path, x, labels, names):
    with open(path, "w") as fh:
        fh.write("%d\n" % x.shape[1])
        for row, l in zip(x, labels):
            fh.write(" ".join(repr(float(v)) for v in row) + " " + names[int(l)] + "\n")


def test_glvq_help_and_bad_arguments(tools, tmp_path):
    """-help, and the refusals that need no engine: they come before one is asked for, so they hold without a GPU"""
    p = run("glvq", "-help")
    assert p.returncode == 0 and p.stdout.startswith("glvq - ") and "-epochs" in p.stdout and "-alpha" in p.stdout and "-sigmoid" in p.stdout
    cod, dat, out = tmp_path / "c.cod", tmp_path / "d.dat", tmp_path / "o.cod"
    cod.write_text("2\n0 0 a\n1 1 b\n")
    dat.write_text("2\n0.25 0.5 a\n0.75 0.5 b\n")
    for args, word in ((("-epochs", 0, "-alpha", 1), "-epochs"), (("-epochs", -2, "-alpha", 1), "-epochs"),
                       (("-epochs", 2, "-alpha", -1), "-alpha"), (("-epochs", 2, "-alpha", "nan"), "-alpha"),
                       (("-epochs", 2, "-alpha", 1, "-sigmoid", -1), "-sigmoid"), (("-epochs", 2, "-alpha", 1, "-sigmoid", "nan"), "-sigmoid")):
        p = run("glvq", "-cin", cod, "-din", dat, "-cout", out, *args)
        assert p.returncode == 1 and p.stderr.startswith("glvq: " + word), (args, p.stderr)
        assert not out.exists()
    good = ("-epochs", 2, "-alpha", 1)
    dim3 = tmp_path / "d3.dat"
    dim3.write_text("3\n1 2 3 a\n4 5 6 b\n")
    p = run("glvq", "-cin", cod, "-din", dim3, "-cout", out, *good)
    assert p.returncode == 1 and "different dimensions" in p.stderr
    for name, text, other, word in (("x.cod", "2\nx 0 a\n1 1 b\n", None, "masked components"), ("x.dat", "2\nx 0.5 a\n0.75 0.5 b\n", None, "masked components"),
                                    ("n.cod", "2\n0 0\n1 1\n", None, "no labels"), ("n.dat", "2\n0.25 0.5\n0.75 0.5\n", None, "no labels"),
                                    ("one.cod", "2\n0 0 a\n1 1 a\n", None, "one label"), ("z.dat", "2\n0.25 0.5 a\n0.75 0.5 z\n", None, "no codebook row")):
        f = tmp_path / name
        f.write_text(text)
        p = run("glvq", "-cin", f if name.endswith(".cod") else cod, "-din", f if name.endswith(".dat") else dat, "-cout", out, *good)
        assert p.returncode == 1 and word in p.stderr, (name, p.stderr)
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
    """A labelled codebook and data set with the edges the search has to get right: a class with a single row, a class
    whose rows all lie behind the last full group of 64 (and of 1024) rows, duplicated rows within a class and across
    two classes, a sample equal to a prototype and a sample equal to prototypes of two classes"""
    rs = np.random.RandomState(seed)
    c = rs.standard_normal((rows, dim)).astype(f32)
    cl = rs.randint(0, max(classes - 2, 1), size=rows).astype(np.int32) if classes > 2 else np.zeros(rows, dtype=np.int32)
    tail = (rows - 1) // 64 * 64 if rows > 64 else rows - 1       # first row of the last group (partial or not)
    if rows > 1024:
        tail = 1024
    cl[cl == classes - 1] = 0
    cl[tail:] = classes - 1                                        # the last class: only behind the last full group
    if classes > 2:
        cl[cl == classes - 2] = 0
        cl[rows // 3] = classes - 2                                # a class with a single row
    x = (rs.standard_normal((n_data, dim)) * 1.5).astype(f32)
    dl = cl[rs.randint(0, rows, size=n_data)].astype(np.int32)
    if rows >= 8:
        a, b = 1, rows // 2
        c[b] = c[a]; cl[b] = cl[a]                                  # duplicates within a class: the lower row must win
        if cl[a] == cl[rows // 3] and classes > 2:
            cl[a] = cl[b] = 0
        same = np.flatnonzero(cl == cl[a])
        diff = np.flatnonzero(cl != cl[a])
        c[diff[-1]] = c[a]                                          # ... and across two classes
        if len(diff) > 1 and n_data > 2:
            c[diff[0]] = c[diff[-1]]                                # ... twice in the other class: its lower row must win too
        if n_data > 3:
            x[0] = c[a]; dl[0] = cl[a]                              # a sample equal to prototypes of two classes: D = 0
            x[1] = c[a]; dl[1] = cl[diff[-1]]
            lone = same[same != a][0] if len(same) > 2 else a
            x[2] = c[lone + 1 if lone + 1 < rows and lone + 1 not in (a, b, diff[0], diff[-1]) else lone]
            dl[2] = cl[lone + 1 if lone + 1 < rows and lone + 1 not in (a, b, diff[0], diff[-1]) else lone]   # d+ = 0 alone
    assert len(set(cl.tolist())) >= 2 and set(dl.tolist()) <= set(cl.tolist())
    return c, cl, x, dl


def check_search(E, eng, c, cl, x, dl, first, n, routes=None):
    cb = E.Codebook(eng, c, labels=cl)
    ds = E.Dataset(eng, x, labels=dl)
    want = R.search(c, cl, x, dl, first, n)
    rems = {}
    for route in routes or (E.GLVQ_DIRECT, E.GLVQ_LIST):
        for again in range(2):                                       # the same call twice
            dp, ip, dm, im, rem = E.glvq_search(cb, ds, first, n, route)
            assert (ip == want[1]).all() and (im == want[3]).all(), (route, np.flatnonzero((ip != want[1]) | (im != want[3]))[:5])
            assert (bits32(dp) == bits32(want[0])).all() and (bits32(dm) == bits32(want[2])).all(), route
            rems[route] = rem
    assert rems.get(E.GLVQ_DIRECT, n) == n
    cb.close(); ds.close()
    return rems.get(E.GLVQ_LIST)


SEARCH_SHAPES = [(2, 1, 1, 2), (2, 4, 33, 2), (63, 3, 31, 3), (64, 4, 32, 4), (65, 5, 33, 5), (256, 127, 700, 7), (257, 128, 33, 6),
                 (1030, 129, 700, 7), (1030, 4, 32, 2), (256, 5, 1, 3), (65, 129, 31, 2), (1030, 1, 700, 4), (257, 3, 700, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,classes", SEARCH_SHAPES)
def test_search_both_routes_equal_the_replay(E, eng, rows, dim, n, classes):
    """rows at the lane, group and 4R-group edges, dims around the float4 and 128 edges, runs around the 32-sample tile,
    2 to 7 classes with the edge cases of edge_case; plain and wrapped ranges; both routes; every call twice"""
    n_data = max(n, 5) if n != 700 else 300                         # 700 samples of 300 rows: the run wraps twice
    c, cl, x, dl = edge_case(1000 + rows + dim, rows, dim, n_data, classes)
    check_search(E, eng, c, cl, x, dl, 0, n)
    check_search(E, eng, c, cl, x, dl, n_data - 2, n)               # wraps after two rows


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(256, 5), (1030, 16)])
def test_list_route_without_the_other_role_goes_through_the_remainder(E, eng, rows, dim):
    """40 rows of one class in front, next to every sample, and every other row far away: no top-8 list holds a row of
    another class, so the list route has every sample in its remainder and must equal the direct route"""
    rs = np.random.RandomState(rows)
    c = (50.0 + rs.standard_normal((rows, dim))).astype(f32)
    c[:40] = (0.01 * rs.standard_normal((40, dim))).astype(f32)
    cl = (1 + np.arange(rows) % 3).astype(np.int32)
    cl[:40] = 0
    x = (0.01 * rs.standard_normal((70, dim))).astype(f32)
    dl = (np.arange(70) % 4).astype(np.int32)                        # class 0: no other role in the list; 1..3: no own role
    assert check_search(E, eng, c, cl, x, dl, 3, 70) == 70
    x[::2] += 50.0                                                   # half the samples next to the mixed rows: lists with both roles
    rem = check_search(E, eng, c, cl, x, dl, 3, 70)
    assert 35 <= rem < 70


def sums_case(seed, rows, dim, n, classes=3, one_winner=False):
    x, dl, c, cl = clusters(seed, n, rows, dim, classes)
    if one_winner:                                                   # one class with one row, every sample of that class
        cl[:] = 1
        cl[rows // 2] = 0
        dl[:] = 0
    return c, cl, x, dl


SUMS_SHAPES = [(12, 16, 300, False), (5, 63, 150, False), (5, 64, 150, False), (5, 65, 150, False), (7, 3, 200, True), (256, 5, 20, False),
               (70, 129, 97, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,one", SUMS_SHAPES)
def test_identity_terms_and_sums_equal_the_replay_bit_for_bit(E, eng, rows, dim, n, one):
    """all samples on one prototype, most prototypes unchosen, lists crossing 64 columns at dims 63 / 64 / 65: xi, f, every
    sum, the counts and the correct count"""
    c, cl, x, dl = sums_case(rows * 7 + dim, rows, dim, n, one_winner=one)
    first = 11
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.glvq_sums(cb, ds, first, n)
    dp, ip, dm, im = R.search(c, cl, x, dl, first, n)
    xp, xm, f, correct = R.terms(dp, ip, dm, im)
    S = R.sums(x, ip, im, xp, xm, f, rows, first)
    assert (bits64(got["xi_plus"]) == bits64(xp)).all() and (bits64(got["xi_minus"]) == bits64(xm)).all() and (bits64(got["f"]) == bits64(f)).all()
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    for key in ("sums_plus", "sums_minus", "cost"):
        assert (bits64(got[key]) == bits64(S[key])).all(), key
    if one:
        assert got["n_plus"][rows // 2] == n and got["n_plus"].sum() == n
    assert (bits64(E.glvq_sums(cb, ds, first, n)["sums_minus"]) == bits64(got["sums_minus"])).all()     # twice the same bits
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,beta", [(12, 16, 300, 2.0), (5, 65, 150, 0.5), (256, 5, 20, 4.0)])
def test_sigmoid_terms_and_sums_within_the_derived_bounds(E, eng, rows, dim, n, beta):
    c, cl, x, dl = sums_case(rows + dim, rows, dim, n)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.glvq_sums(cb, ds, 0, n, beta)
    dp, ip, dm, im = R.search(c, cl, x, dl, 0, n)
    xp, xm, f, correct = R.terms(dp, ip, dm, im, beta)
    S = R.sums(x, ip, im, xp, xm, f, rows)
    rel = R.xi_rel_bound(beta)
    worst = {}
    for name, ref, tol in (("xi_plus", xp, rel * xp), ("xi_minus", xm, rel * xm), ("f", f, R.F_REL_BOUND * f)):
        err = np.abs(got[name] - ref)
        worst[name] = float((err / np.maximum(tol, 1e-300)).max())
        assert (err <= tol).all(), (name, worst)
    bp, bm, bc = R.sums_bound(S, beta)
    for name, tol in (("sums_plus", bp), ("sums_minus", bm), ("cost", bc)):
        err = np.abs(got[name] - S[name])
        worst[name] = float((err / tol).max())
        assert (err <= tol).all(), (name, worst)
    print("largest error / bound:", worst)
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["correct"] == correct
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,n,beta", [(12, 16, 300, 0.0), (70, 129, 97, 0.0), (256, 5, 20, 0.0), (12, 16, 300, 2.0), (256, 5, 20, 4.0)])
def test_update_equals_the_replay(E, eng, rows, dim, n, beta):
    """identity: the rows bit-equal with the float64 replay from the same sums; sigmoid: within ulp32 / 2 plus the carried
    bounds of the np.longdouble replay from the replay's sums.  Rows no sample chose keep their bits, -0.0 included."""
    c, cl, x, dl = sums_case(rows + 3 * dim, rows, dim, n)
    dp, ip, dm, im = R.search(c, cl, x, dl, 0, n)
    unchosen = np.setdiff1d(np.arange(rows), np.concatenate([ip, im]))
    if len(unchosen):                                                # a row of -0.0s that stays unchosen: its other half is far away
        c[unchosen[0], ::2] = -0.0
        c[unchosen[0], 1::2] = 1000.0
        dp, ip, dm, im = R.search(c, cl, x, dl, 0, n)
        assert unchosen[0] not in ip and unchosen[0] not in im
        unchosen = np.setdiff1d(np.arange(rows), np.concatenate([ip, im]))
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    got = E.glvq_sums(cb, ds, 0, n, beta)
    alpha_t = R.alpha_at(7.5, 9, 2)
    E.glvq_update(cb, alpha_t, n, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"])
    rows_after = cb.download()
    want = R.update(c, got, alpha_t, n)
    assert (bits32(rows_after) == bits32(want)).all()
    assert (bits32(rows_after[unchosen]) == bits32(c[unchosen])).all()
    if rows == 256:
        assert len(unchosen) > 200
    xp, xm, f, _ = R.terms(dp, ip, dm, im, beta)
    S = R.sums(x, ip, im, xp, xm, f, rows)
    q, bound = R.update_longdouble(c, S, alpha_t, n, beta)
    live = (S["n_plus"] > 0) | (S["n_minus"] > 0)
    err = np.abs(rows_after.astype(np.longdouble) - q)
    assert (err[live] <= bound[live]).all(), float((err[live] / bound[live]).max())
    cb.close(); ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 2.0])
def test_runs(E, eng, beta):
    """5 epochs in one call equal five calls and equal themselves run twice; an epoch equals its stages; cost and correct
    equal the replay's (by bit pattern with the identity)"""
    x, dl, c, cl = clusters(9, 400, 12, 16)
    first, n, T, alpha = 7, 390, 5, 10.0
    ds = E.Dataset(eng, x, labels=dl)
    cb = E.Codebook(eng, c, labels=cl)
    cost, correct = E.glvq_train(cb, ds, T, alpha, beta, first=first, n=n)
    one = cb.download()
    cb.upload(c)
    cost2, correct2 = E.glvq_train(cb, ds, T, alpha, beta, first=first, n=n)
    assert (bits32(cb.download()) == bits32(one)).all() and (bits64(cost2) == bits64(cost)).all() and (correct2 == correct).all()
    cb.upload(c)
    for t in range(T):
        ct, rt = E.glvq_train(cb, ds, T, alpha, beta, start_epoch=t, count=1, first=first, n=n)
        assert bits64(ct)[0] == bits64(cost)[t] and rt[0] == correct[t]
    assert (bits32(cb.download()) == bits32(one)).all()
    cb.upload(c)
    for t in range(T):                                               # an epoch is its stages
        got = E.glvq_sums(cb, ds, first, n, beta)
        chain = f64(0.0)
        for v in got["cost"]:
            chain = chain + v
        assert bits64(chain / f64(n))[()] == bits64(cost)[t] and got["correct"] == correct[t]
        E.glvq_update(cb, E.glvq_alpha(alpha, T, t), n, got["sums_plus"], got["n_plus"], got["sums_minus"], got["n_minus"])
    assert (bits32(cb.download()) == bits32(one)).all()
    rows, rcost, rcorrect = R.train(c, cl, x, dl, T, alpha, beta, first, n)
    assert E.glvq_alpha(alpha, T, 3) == R.alpha_at(alpha, T, 3)
    if beta == 0.0:
        assert (bits32(one) == bits32(rows)).all() and (bits64(cost) == bits64(rcost)).all()
    else:
        assert np.allclose(one, rows, rtol=0, atol=1e-5) and np.allclose(cost, rcost, rtol=1e-12, atol=0)
    assert (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_training_on_the_planned_list_route_equals_the_replay(E, eng):
    """the smallest shape at which the plan takes the list route (32768 rows of 512 components, 33 samples): an epoch by
    bit pattern against the replay, and the search on both routes"""
    rows, dim, n = 32768, 512, 33
    assert E.glvq_plan(rows, dim, n) == E.GLVQ_LIST and E.glvq_plan(rows - 1, dim, n) == E.GLVQ_DIRECT
    x, dl, c, cl = clusters(77, n, rows, dim, classes=3, sep=0.5)
    c[:3] = x[:3]; cl[:3] = dl[:3]                                    # d+ = 0 for three samples
    rem = check_search(E, eng, c, cl, x, dl, 5, n)
    assert 0 <= rem <= n
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.glvq_train(cb, ds, 2, 50.0, first=5, count=1)
    want, rcost, rcorrect = R.train(c, cl, x, dl, 2, 50.0, first=5, count=1)
    assert (bits32(cb.download()) == bits32(want)).all() and (bits64(cost) == bits64(rcost)).all() and (correct == rcorrect).all()
    cb.close(); ds.close()


@pytest.mark.gpu
def test_cost_falls_every_epoch_on_clusters(E, eng):
    """three Gaussian classes, 2000 samples, 12 prototypes, dim 16, alpha 10: the cost falls every epoch of 20 and ends
    below the cost before the first; the device's costs are the replay's"""
    x, dl, c, cl = clusters(5, 2000, 12, 16)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.glvq_train(cb, ds, 20, 10.0)
    got = E.glvq_sums(cb, ds)
    after = float(got["cost"].sum()) / 2000
    assert (np.diff(np.append(cost, after)) < 0).all() and after < cost[0], (cost, after)
    rows, rcost, rcorrect = R.train(c, cl, x, dl, 20, 10.0)
    assert (bits64(cost) == bits64(rcost)).all() and (correct == rcorrect).all() and (bits32(cb.download()) == bits32(rows)).all()
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
        (cb, ds, dict(sigmoid_beta=-0.5), "sigmoid_beta"), (cb, ds, dict(sigmoid_beta=float("nan")), "sigmoid_beta"),
    ]
    for book, data, kw, word in cases:
        args = dict(epochs=5, alpha=1.0)
        args.update(kw)
        with pytest.raises(Exception) as ei:
            E.glvq_train(book, data, **args)
        assert str(ei.value).startswith("somhip_glvq_train: ") and word in str(ei.value), (kw, str(ei.value))
        assert (bits32(book.download()) == bits32(c[:book.n])).all()
    for fn, name in ((lambda: E.glvq_search(E.Codebook(eng, c), ds), "somhip_debug_glvq_search"), (lambda: E.glvq_search(cb, ds, route=7), "somhip_debug_glvq_search"),
                     (lambda: E.glvq_sums(cb, ds, sigmoid_beta=-1.0), "somhip_debug_glvq_sums"), (lambda: E.glvq_sums(cb, ds, n=0), "somhip_debug_glvq_sums"),
                     (lambda: E.glvq_update(cb, 1.0, 0, np.zeros((6, 5)), np.zeros(6), np.zeros((6, 5)), np.zeros(6)), "somhip_debug_glvq_update")):
        with pytest.raises(Exception) as ei:
            fn()
        assert str(ei.value).startswith(name + ": "), str(ei.value)
    assert (bits32(cb.download()) == bits32(c)).all()


@pytest.mark.gpu
def test_timing_counts_the_four_stages(E, eng):
    x, dl, c, cl = clusters(4, 100, 6, 8)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    eng.timing(True); eng.timing_reset()
    E.glvq_train(cb, ds, 3, 1.0, stats=False)
    t = eng.glvq_timing()
    eng.timing(False)
    assert t["search"][0] == 3 and t["terms"][0] == 3 * 5 and t["k_glvq_sums"][0] == 3 and t["k_glvq_update"][0] == 3
    assert all(ms > 0 for _, ms in t.values())
    cb.close(); ds.close()


@pytest.mark.gpu
def test_glvq_tool_writes_the_engines_rows_and_lines(E, eng, tools, tmp_path):
    """the tool on files: the written .cod holds the rows engine.glvq_train leaves, the -v lines its alpha_t, cost and
    accuracy per epoch, and the correct count is what `accuracy` says of the same files"""
    x, dl, c, cl = clusters(21, 120, 9, 5)
    names = ["ape", "bee", "cat"]
    dat, cod, out = tmp_path / "d.dat", tmp_path / "c.cod", tmp_path / "o.cod"
    write_dat(dat, x, dl, names)
    write_dat(cod, c, cl, names)
    from som_lvq_pak_amd import textio
    for beta in (0.0, 1.5):
        p = run("glvq", "-din", dat, "-cin", cod, "-cout", out, "-epochs", 4, "-alpha", 2.5, "-v", *(("-sigmoid", beta) if beta else ()))
        assert p.returncode == 0, p.stderr
        cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
        cost, correct = E.glvq_train(cb, ds, 4, 2.5, beta)
        text = out.read_text().split("\n")
        rows = np.array([[float(v) for v in ln.split()[:5]] for ln in text[1:] if ln.strip() and not ln.startswith("#")], dtype=f32)
        printed = np.array([[f32(float(textio.fmt_g(v))) for v in row] for row in cb.download()], dtype=f32)     # the file is "%g" text
        assert (bits32(rows) == bits32(printed)).all()
        assert [ln.split()[5] for ln in text[1:] if ln.strip() and not ln.startswith("#")] == [names[int(l)] for l in cl]
        lines = [ln for ln in (p.stdout + p.stderr).split("\n") if ln.startswith("epoch ")]
        assert len(lines) == 4
        for t, ln in enumerate(lines):
            m = re.match(r"epoch (\d+) alpha ([-+.\deE]+) cost ([-+.\deE]+) accuracy ([-+.\deE]+) %", ln)
            assert m and int(m.group(1)) == t, ln
            assert float(m.group(2)) == pytest.approx(float(E.glvq_alpha(2.5, 4, t)), rel=1e-5)
            assert float(m.group(3)) == pytest.approx(cost[t], rel=1e-9) and float(m.group(4)) == pytest.approx(100.0 * correct[t] / 120, abs=0.006)
        cb.close(); ds.close()
    a = run("accuracy", "-din", dat, "-cin", cod)
    assert a.returncode == 0, a.stderr
    m = re.search(r"Total accuracy:\s+(\d+) entries\s+([\d.]+) %", a.stdout)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    cost, correct = E.glvq_train(cb, ds, 1, 0.0)
    assert m and int(m.group(1)) == 120 and float(m.group(2)) == pytest.approx(100.0 * correct[0] / 120, abs=0.006), a.stdout
