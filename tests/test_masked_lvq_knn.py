"""LVQ training and k-NN searches on data with missing (`x`) components.

Only the sample's mask counts (lvq_pak.c:65-69, 179-186, 343-347): a masked component is left out of every distance
and every update, and a code row's own `x` components take part with the value the reader stored for them (0.0).
The tool runs are replayed against what the REAL reference wrote for the same inputs (tests/golden/masked, made by
tests/golden/make_golden_masked.py) and compared byte for byte.  The masked data files are not stored: the fixture
script's seeded write_masked_data() makes them again, and their md5 is checked against the recorded one."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, synth
from som_lvq_pak_amd import textio

MASKED = os.path.join(GOLDEN, "masked")
EXPECTED = json.load(open(os.path.join(MASKED, "expected.json")))
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
REF = os.path.join(ROOT, "oracle", "_ref")


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """ex1_masked.dat / ex2_masked.dat, made again by the fixture script's seeded masking"""
    spec = importlib.util.spec_from_file_location("make_golden_masked", os.path.join(GOLDEN, "make_golden_masked.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path_factory.mktemp("masked_data")
    mod.write_masked_data(str(out))
    return str(out)


# ------------------------------------------------------------------ CPU: the fixtures
def test_masked_fixtures_exist_and_parse(data_dir):
    for f, want in EXPECTED["data"].items():
        assert md5(os.path.join(data_dir, f)) == want, f            # the same bytes the reference was run on
        e, _ = textio.read_entries(os.path.join(data_dir, f), skip_empty=False)
        assert e.mask is not None and e.points.shape[0] > 1900
        share = e.mask.mean()
        assert 0.07 < share < 0.13, (f, share)                      # about 10 % of the components are `x`
        assert not e.mask.all(axis=1).any(), f                      # no fully masked row
        assert sum(1 for ln in open(os.path.join(data_dir, f)) if ln.startswith("#")) == \
            sum(1 for ln in open(os.path.join(GOLDEN, "data", f.replace("_masked", ""))) if ln.startswith("#"))
    for tag in ("eveninit_knn5", "olvq1"):                            # the two stored codebooks later runs start from
        p = os.path.join(MASKED, tag + ".cod")
        assert md5(p) == EXPECTED["runs"][tag]["md5"], tag
        e, _ = textio.read_entries(p)
        assert e.points.shape == (200, 20)
    # the LVQ runs start from a codebook whose rows carry `x` of their own
    ini, _ = textio.read_entries(os.path.join(MASKED, "eveninit_knn5.cod"))
    assert ini.mask is not None and ini.mask.any(axis=1).sum() > 100


# ------------------------------------------------------------------ GPU: the engine
@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


def _masked_case(seed, n, d, m, frac=0.15):
    """codes with exact duplicates (ties), samples with ~frac masked components, three of them fully masked; masked
    components hold NaN / inf (a select, not a multiply by the mask, keeps them out)"""
    x, _ = synth(seed, m, d, k=5, spread=2.0)
    rs = np.random.RandomState(seed)
    codes = (x[rs.randint(0, m, n)] + 0.05 * rs.standard_normal((n, d))).astype(np.float32)
    codes[n // 2:n // 2 + 16] = codes[:16]
    mask = (rs.random_sample((m, d)) < frac).astype(np.uint8)
    mask[[1, m // 2, m - 1]] = 1
    xs = x.copy()
    xs[mask != 0] = np.where(rs.random_sample(int(mask.sum())) < 0.5, np.nan, np.inf).astype(np.float32)
    xo = x.copy()
    xo[mask != 0] = 0.0                 # what the oracle reads (never used: its mask skips them)
    return codes, xs, xo, mask


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m", [(300, 20, 257), (4096, 64, 300), (5000, 13, 70)])
@pytest.mark.parametrize("knn", [2, 3, 5, 8])
def test_masked_find_winners_knn(eng, E, oracle, n, d, m, knn):
    codes, xs, xo, mask = _masked_case(n + d + knn, n, d, m)
    want_i, want_d, want_r = oracle.winners(codes, xo, knn, True, mask=mask)
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, xs, mask=mask)
    gi, gd, gr = E.find_winners(cb, ds, knn=knn, tie=E.TIE_KNN)
    assert np.array_equal(gr, want_r)
    assert (gr == 0).sum() == 3 and np.all(gi[gr == 0] == -2)
    assert np.array_equal(gi, want_i)
    assert np.array_equal(bits(gd), bits(want_d))
    # a run that wraps round the end of the data
    gi2, gd2, _ = E.find_winners(cb, ds, first=m - 5, count=12, knn=knn, tie=E.TIE_KNN)
    order = [(m - 5 + j) % m for j in range(12)]
    assert np.array_equal(gi2, want_i[order]) and np.array_equal(bits(gd2), bits(want_d[order]))
    ds.close()
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knn", [2, 4, 8])
def test_masked_batch_topk_keys(eng, E, oracle, knn):
    from som_lvq_pak_amd import sharded
    n, d, m = 4096, 40, 200
    codes, xs, xo, mask = _masked_case(31 + knn, n, d, m)
    want_i, want_d, want_r = oracle.winners(codes, xo, knn, True, mask=mask)
    cb = E.Codebook(eng, codes)
    ds = E.Dataset(eng, xs, mask=mask)
    kb = eng.device_alloc(8 * m * knn)
    assert eng.lib.somhip_batch_topk_keys(cb.h, ds.h, 0, m, knn, E.TIE_KNN, kb) == 0
    hk = np.empty((m, knn), dtype=np.uint64)
    assert eng.lib.somhip_copy_to_host(eng.h, hk.ctypes.data_as(C.c_void_p), kb, 8 * m * knn) == 0
    eng.device_free(kb)
    gd, gi = sharded.unpack_knn_keys(hk)
    live = want_r != 0                                       # fully masked samples: the caller's to skip
    assert np.array_equal(gi[live], want_i[live])
    assert np.array_equal(bits(gd[live]), bits(want_d[live]))
    ds.close()
    cb.close()


@pytest.mark.gpu
def test_lvq_refuses_a_fully_masked_sample_and_the_engine_goes_on(eng, E, tmp_path, data_dir):
    tab = textio.LabelTable()
    x1, _ = textio.read_entries(os.path.join(data_dir, "ex1_masked.dat"), tab)
    ini, _ = textio.read_entries(os.path.join(MASKED, "eveninit_knn5.cod"), tab)
    lab = x1.first_label.astype(np.int32)
    bad = x1.mask.copy()
    bad[7] = 1
    cb = E.Codebook(eng, ini.points, labels=ini.first_label.astype(np.int32))
    ds = E.Dataset(eng, x1.points, mask=bad, labels=lab)
    with pytest.raises(Exception, match="row 7 has every component masked"):
        E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, trace=False)
    assert np.array_equal(bits(cb.download()), bits(ini.points))        # nothing was trained
    # iterations that never reach row 7 run
    E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, start_iter=0, count=5, data_first=0, trace=False)
    ds.close()
    # the same engine, the same codebook object: the reference's lvq1 on the masked data, byte for byte
    cb.upload(ini.points)
    ds = E.Dataset(eng, x1.points, mask=x1.mask, labels=lab)
    E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, trace=False)
    ini.points = cb.download()
    out = str(tmp_path / "lvq1.cod")
    textio.write_entries(out, ini, tab)
    assert md5(out) == EXPECTED["runs"]["lvq1"]["md5"]
    ds.close()
    cb.close()


# ------------------------------------------------------------------ GPU: the tools, byte for byte
@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("lvqtrain", "knntest", "eveninit", "balance", "elimin")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


def run(exe, *args, env=None):
    p = subprocess.run([exe] + [str(a) for a in args] + ["-v", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, (exe, args, p.stderr)
    return p.stdout


@pytest.fixture(scope="module")
def d(data_dir):
    return lambda f: os.path.join(data_dir, f)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["eveninit_knn5", "eveninit_knn3", "propinit_knn5", "propinit_knn3", "elimin_knn5"])
def test_masked_init_tools(tools, tmp_path, d, tag):
    r = EXPECTED["runs"][tag]
    out = tmp_path / "out.cod"
    run(os.path.join(BIN, r["tool"]), "-din", d(r["din"]), "-cout", out, *r["args"])
    assert md5(out) == r["md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["lvq1", "olvq1", "lvq2", "lvq3"])
def test_masked_lvq_tools(tools, tmp_path, d, tag):
    r = EXPECTED["runs"][tag]
    cin = os.path.join(MASKED, r["cin"])
    out = tmp_path / "out.cod"
    run(os.path.join(BIN, r["tool"]), "-din", d(r["din"]), "-cin", cin, "-cout", out, *r["args"])
    assert md5(out) == r["md5"]
    assert not os.path.exists(tmp_path / "out.lra")                  # lvqtrain.c:249 removes it
    assert run(os.path.join(BIN, "accuracy"), "-din", d("ex2_masked.dat"), "-cin", out) == r["accuracy_stdout"]
    out2 = tmp_path / "out2.cod"
    run(os.path.join(BIN, "lvqtrain"), "-type", r["tool"], "-din", d(r["din"]), "-cin", cin, "-cout", out2, *r["args"])
    assert md5(out2) == r["md5"]


@pytest.mark.gpu
def test_masked_scanners(tools, tmp_path, d):
    t = EXPECTED["scan"]
    cod = os.path.join(MASKED, "olvq1.cod")
    ex2 = d("ex2_masked.dat")
    assert run(os.path.join(BIN, "accuracy"), "-din", ex2, "-cin", cod) == t["accuracy"]
    for knn in (1, 3, 5, 8):
        assert run(os.path.join(BIN, "knntest"), "-din", ex2, "-cin", cod, "-knn", knn) == t["knntest_%d" % knn], knn
    run(os.path.join(BIN, "classify"), "-din", ex2, "-cin", cod, "-dout", tmp_path / "cls.dat", "-cfout", tmp_path / "cls.cfo")
    assert md5(tmp_path / "cls.dat") == t["classify_dout_md5"]
    assert md5(tmp_path / "cls.cfo") == t["classify_cfout_md5"]
    assert run(os.path.join(BIN, "cmatr"), "-din", ex2, "-cin", cod, "-cfout", tmp_path / "cm.cfo") == t["cmatr"]
    assert md5(tmp_path / "cm.cfo") == t["cmatr_cfout_md5"]
    for knn in (3, 5):
        run(os.path.join(BIN, "setlabel"), "-din", ex2, "-cin", cod, "-cout", tmp_path / "sl.cod", "-knn", knn)
        assert md5(tmp_path / "sl.cod") == t["setlabel_%d_md5" % knn], knn


def _glued(tool):
    exe = os.path.join(REF, tool)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs the reference sources at build time)" % tool)
    return exe


@pytest.mark.gpu
def test_masked_runs_through_the_glue(tmp_path, d):
    """the reference's own lvqtrain.o / knntest.o linked with host/glue/somhip_glue.c: masked LVQ training goes to the
    engine (no CPU fall-back any more) and gives the reference's bytes; knntest_hip with the "hip" row gives them too
    (knntest.c:206 puts find_winner_knn in the winner slot itself, so its k-NN stays the reference's)"""
    r = EXPECTED["runs"]["lvq3"]
    out = tmp_path / "lvq3.cod"
    run(_glued("lvqtrain_hip"), "-type", "lvq3", "-din", d(r["din"]), "-cin", os.path.join(MASKED, r["cin"]), "-cout", out,
        *r["args"], env={"SOMHIP_SELFUNCS": "hip"})
    assert md5(out) == r["md5"]
    cod = os.path.join(MASKED, "olvq1.cod")
    assert run(_glued("knntest_hip"), "-din", d("ex2_masked.dat"), "-cin", cod, "-knn", 5, "-selfuncs", "hip") == \
        EXPECTED["scan"]["knntest_5"]
