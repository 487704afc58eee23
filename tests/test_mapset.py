"""Map sets (include/somhip.h: somhip_mapset_*; kernels/mapset.hpp): many maps of one shape trained at once, each in one
workgroup's LDS.  Without a GPU: the symbols, the plan's arithmetic, the refusals, the ISA of the exact instantiations.
On the GPU: every map of every set against the oracle's som_train(batch=1), the compiled reference (plain cases) and
the one-map engine, rows and traces bit for bit, at the wave and workgroup edges of the kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, synth

HEXA, RECT, BUBBLE, GAUSSIAN, LINEAR, INVERSE_T = 3, 4, 1, 2, 1, 2
BUDGET = 128 * 1024
NEW_SYMBOLS = ("somhip_mapset_create", "somhip_mapset_download", "somhip_mapset_upload", "somhip_mapset_destroy",
               "somhip_mapset_train", "somhip_mapset_winners", "somhip_debug_mapset_plan", "somhip_mapset_timing")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    from som_lvq_pak_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ without a GPU
def test_mapset_symbols_exported_and_declared(lib):
    from som_lvq_pak_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(somhip_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct somhip_mapset somhip_mapset;" in hdr
    assert hasattr(engine, "MapSet") and hasattr(engine, "mapset_plan") and hasattr(engine.Engine, "mapset_timing")


def test_mapset_plan_is_host_arithmetic(lib):
    from som_lvq_pak_amd import engine as E
    p = E.mapset_plan(96, 5)
    assert p["fits"] and p["threads"] == 128 and p["units_per_thread"] == 1 and p["chunk"] >= 1 and not p["masked"]
    assert p["lds_bytes"] >= 5 * 128 * 4
    assert E.mapset_plan(96, 5, masked=True)["masked"]
    # an image of exactly the budget fits (dim x units-rounded-to-64 x 4 bytes); one unit or one component more does not
    for n, d in ((128, 256), (64, 512), (1024, 32), (32768, 1)):
        assert n * d * 4 == BUDGET
        assert E.mapset_plan(n, d)["fits"], (n, d)
        assert not E.mapset_plan(n + 1, d)["fits"], (n, d)
        assert not E.mapset_plan(n, d + 1)["fits"], (n, d)
    for n in (1, 63, 64, 65, 96, 1000, 1024, 1025, 1050, 2048, 2049, 5000):
        for d in (1, 3, 6):
            p = E.mapset_plan(n, d)
            assert p["fits"], (n, d)
            assert p["threads"] % 64 == 0 and 64 <= p["threads"] <= 1024
            assert p["units_per_thread"] * p["threads"] >= n
            assert (p["units_per_thread"] - 1) * p["threads"] < n
            assert d * ((n + 63) // 64 * 64) * 4 <= p["lds_bytes"] <= 160 * 1024
    out = (C.c_int32 * 8)()
    assert lib.somhip_debug_mapset_plan(0, 5, 0, out) != 0 and lib.somhip_debug_mapset_plan(96, 0, 0, out) != 0
    assert lib.somhip_debug_mapset_plan(96, 5, 0, None) != 0


def test_mapset_entry_points_refuse_null_arguments(lib, tmp_path):
    from som_lvq_pak_amd import _lib
    rows = np.zeros((2, 6, 3), np.float32)
    h = C.c_void_p()
    p = _lib.SomParams(10, 0.05, 2.0, 1, 0, 0, 1, 0, 10, 0)
    fp, ip = _lib.c_float_p, _lib.c_i32_p
    buf_f, buf_i = np.zeros(64, np.float32), np.zeros(64, np.int32)
    assert lib.somhip_mapset_create(None, rows.ctypes.data_as(fp), 2, 6, 3, HEXA, BUBBLE, 3, 2, C.byref(h)) != 0
    assert b"null" in lib.somhip_last_error()
    assert lib.somhip_mapset_train(None, None, C.byref(p), None, None) != 0 and b"null" in lib.somhip_last_error()
    assert lib.somhip_mapset_winners(None, None, 0, 1, buf_i.ctypes.data_as(ip), buf_f.ctypes.data_as(fp), None) != 0
    assert lib.somhip_mapset_download(None, 0, 1, buf_f.ctypes.data_as(fp)) != 0
    assert lib.somhip_mapset_upload(None, 0, 1, buf_f.ctypes.data_as(fp)) != 0
    lib.somhip_mapset_destroy(None)                     # a null handle is nothing to destroy
    import torch
    if not torch.cuda.is_available():
        # ... and nothing runs without a GPU: no engine to make a set on, and vfind's set route ends with the engine's message
        from som_lvq_pak_amd import engine as E
        with pytest.raises(Exception, match="no HIP device|no CPU path|hip"):
            E.MapSet(E.Engine(0), rows, HEXA, BUBBLE, 3, 2)
        ans = "\n".join(["3", os.path.join(GOLDEN, "data", "ex.dat"), os.path.join(GOLDEN, "data", "ex.dat"), "o.cod", "hexa", "bubble",
                         "6", "5", "50", "0.05", "5", "50", "0.02", "2"]) + "\n"
        if len(os.path.join(GOLDEN, "data", "ex.dat")) < 99:
            r = subprocess.run([os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "vfind")], input=ans, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, cwd=tmp_path)
            assert r.returncode == 1 and "no CPU path" in r.stderr and not os.path.exists(tmp_path / "o.cod")


def test_vfind_help_names_together(lib):
    exe = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "vfind")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    r = subprocess.run([exe, "-help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "-together" in r.stdout and "MI355X" in r.stdout


def test_exact_mapset_kernels_have_no_fma(lib, tmp_path):
    """as test_exact_kernels_have_no_fma: distance = sub, mul, add and update = sub, mul, add with a rounding each, so
    the bubble instantiations of k_mapset_train and both of k_mapset_winners hold no fp32 fma / mac / mad.  (The
    gaussian ones legitimately hold the rate's division and exp; they are checked for parity on the GPU.)"""
    s = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "--cuda-device-only", "-S", "-o", s, os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")])
    txt = open(s).read()
    bodies = dict(re.findall(r"^(_ZN6somhip\w+):.*?\n(.*?)s_endpgm", txt, flags=re.S | re.M))
    checked = []
    for name, body in bodies.items():
        if not ("k_mapset_trainILb0E" in name or "k_mapset_winnersILb" in name):
            continue
        checked.append(name)
        bad = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)_f32\b.*", body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_(pk_)?mul_f32", body) and re.search(r"v_(pk_)?add_f32", body) and re.search(r"v_(pk_)?sub_f32", body)
    assert len(checked) == 4, checked
    assert sum("k_mapset_trainILb1E" in name for name in bodies) == 2       # the gaussian pair is built too


# ------------------------------------------------------------------------------------------------ on the GPU
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


def make_maps(x, T, n, seed):
    """T initial maps of n units: data rows plus noise, different for every map"""
    rs = np.random.RandomState(seed)
    return (x[rs.randint(0, x.shape[0], (T, n))] + 0.5 * rs.standard_normal((T, n, x.shape[1]))).astype(np.float32)


def roll(a, k):
    return None if a is None else np.roll(a, -k, axis=0)


def check_set(eng, E, oracle, ini, xdim, ydim, topol, neigh, x, length, alpha, radius, alpha_type=LINEAR, mask=None, weight=None,
              fixed=None, use_fixed=0, use_weights=0, ref=None, data_first=0, one_map=True):
    """train the set ini[T, n, d]; every map against the oracle (and ref, and the one-map engine): rows and traces"""
    T = ini.shape[0]
    ds = E.Dataset(eng, x, mask=mask, weight=weight, fixed_xy=fixed)
    ms = E.MapSet(eng, ini, topol, neigh, xdim, ydim)
    ti, td = ms.train(ds, length, alpha, radius, alpha_type=alpha_type, use_fixed=use_fixed, use_weights=use_weights,
                      data_first=data_first, trace=True)
    got = ms.download()
    ms.close()
    assert ti.shape == (T, length) and got.shape == ini.shape
    k = data_first % x.shape[0]
    for m in range(T):
        for who in (oracle, ref):
            if who is None:
                continue
            oc, oi, od = who.som_train(ini[m], xdim, ydim, topol, neigh, roll(x, k), length, alpha, radius, alpha_type=alpha_type,
                                       weight=roll(weight, k), fixed_xy=roll(fixed, k), mask=roll(mask, k), fixed_on=use_fixed,
                                       weights_on=use_weights)
            assert np.array_equal(ti[m], oi), (m, who)
            assert np.array_equal(bits(td[m]), bits(od)), (m, who)
            assert np.array_equal(bits(got[m]), bits(oc)), (m, who)
        if one_map:
            cb = E.Codebook(eng, ini[m], topol, neigh, xdim, ydim)
            ci, cd = E.som_train(cb, ds, length, alpha, radius, alpha_type=alpha_type, use_fixed=use_fixed, use_weights=use_weights,
                                 data_first=data_first)
            assert np.array_equal(ti[m], ci) and np.array_equal(bits(td[m]), bits(cd)), m
            assert np.array_equal(bits(got[m]), bits(cb.download())), m
            cb.close()
    ds.close()
    return got, ti, td


# unit counts at the wave and workgroup edges (1, 63, 64, 65, 96, 1024, 1050: two units per thread, the last trip partly
# empty; a side above 1024: lattice_sq's general form), dims 1, 3, 4, 5, 7, 16
@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,d,topol,neigh", [
    (1, 1, 1, HEXA, BUBBLE), (9, 7, 3, HEXA, BUBBLE), (8, 8, 4, RECT, GAUSSIAN), (13, 5, 5, HEXA, GAUSSIAN), (12, 8, 7, RECT, BUBBLE),
    (12, 8, 16, HEXA, BUBBLE), (32, 32, 4, HEXA, BUBBLE), (32, 32, 3, RECT, GAUSSIAN), (35, 30, 5, HEXA, BUBBLE),
    (35, 30, 3, HEXA, GAUSSIAN), (1, 1100, 3, HEXA, BUBBLE), (1100, 1, 4, RECT, GAUSSIAN), (1, 1030, 1, HEXA, GAUSSIAN)])
def test_every_map_of_a_set_equals_the_oracle_the_reference_and_the_one_map_engine(eng, E, oracle, ref, xdim, ydim, d, topol, neigh):
    x, _ = synth(xdim * 31 + ydim + d, 211, d)
    ini = make_maps(x, 3, xdim * ydim, xdim + ydim)
    check_set(eng, E, oracle, ini, xdim, ydim, topol, neigh, x, 300, 0.07, min(max(xdim, ydim) / 2.0 + 1.0, 12.0), ref=ref)


@pytest.mark.gpu
def test_the_largest_dim_of_a_96_unit_map_and_one_more(eng, E, oracle):
    d = BUDGET // (128 * 4)
    assert E.mapset_plan(96, d)["fits"] and not E.mapset_plan(96, d + 1)["fits"]
    x, _ = synth(5, 90, d)
    check_set(eng, E, oracle, make_maps(x, 2, 96, 1), 12, 8, HEXA, BUBBLE, x, 150, 0.06, 4.0)
    x1, _ = synth(5, 20, d + 1)
    with pytest.raises(Exception, match=r"%d bytes.*%d" % (128 * (d + 1) * 4, BUDGET)):
        E.MapSet(eng, make_maps(x1, 2, 96, 1), HEXA, BUBBLE, 12, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 300])
def test_set_sizes_one_map_and_more_workgroups_than_cus(eng, E, oracle, T):
    x, _ = synth(8, 150, 5)
    check_set(eng, E, oracle, make_maps(x, T, 96, T), 12, 8, HEXA, BUBBLE, x, 200, 0.05, 5.0)


@pytest.mark.gpu
@pytest.mark.parametrize("topol", [HEXA, RECT])
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN])
@pytest.mark.parametrize("alpha_type", [LINEAR, INVERSE_T])
def test_schedules(eng, E, oracle, ref, topol, neigh, alpha_type):
    x, _ = synth(21, 180, 5)
    check_set(eng, E, oracle, make_maps(x, 3, 96, 4), 12, 8, topol, neigh, x, 400, 0.05, 6.0, alpha_type=alpha_type, ref=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN])
def test_a_run_that_crosses_a_chunk(eng, E, oracle, neigh):
    length = E.mapset_plan(96, 5)["chunk"] + 1
    x, _ = synth(22, 333, 5)
    check_set(eng, E, oracle, make_maps(x, 3, 96, 5), 12, 8, HEXA, neigh, x, length, 0.05, 6.0, one_map=False)


@pytest.mark.gpu
def test_continued_runs_data_first_and_short_data(eng, E, oracle):
    # more iterations than data rows (the rows come round), a run that starts at another data row
    x, _ = synth(23, 47, 4)
    ini = make_maps(x, 3, 65, 6)
    want, wi, wd = check_set(eng, E, oracle, ini, 13, 5, HEXA, BUBBLE, x, 300, 0.06, 4.0, data_first=0)
    check_set(eng, E, oracle, ini, 13, 5, HEXA, GAUSSIAN, x, 200, 0.06, 4.0, data_first=29)
    # a run in two calls equals one call
    ds = E.Dataset(eng, x)
    ms = E.MapSet(eng, ini, HEXA, BUBBLE, 13, 5)
    i1, d1 = ms.train(ds, 300, 0.06, 4.0, start_iter=0, count=111, data_first=0, trace=True)
    i2, d2 = ms.train(ds, 300, 0.06, 4.0, start_iter=111, count=189, data_first=111 % 47, trace=True)
    assert np.array_equal(np.concatenate([i1, i2], axis=1), wi)
    assert np.array_equal(bits(np.concatenate([d1, d2], axis=1)), bits(wd))
    assert np.array_equal(bits(ms.download()), bits(want))
    # upload / download of a part of the set
    ms.upload(ini[1:3], first_map=1)
    back = ms.download()
    assert np.array_equal(bits(back[0]), bits(want[0])) and np.array_equal(bits(back[1:]), bits(ini[1:]))
    assert np.array_equal(bits(ms.download(2, 1)[0]), bits(ini[2]))
    ms.close()
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN])
def test_masks_weights_fixed_points_and_ties(eng, E, oracle, ref, neigh):
    rs = np.random.RandomState(31)
    n, d, xdim, ydim = 170, 7, 9, 7
    x, _ = synth(24, n, d)
    mask = (rs.rand(n, d) < 0.25).astype(np.uint8)
    mask[5] = 1                                         # every component masked: the iteration is skipped, trace -2
    mask[9] = 1                                         # ... but a fixed point still teaches (nothing: all components masked), trace -3
    weight = rs.randint(0, 4, n).astype(np.int16)
    fixed = np.full((n, 2), -1, np.int16)
    fixed[3] = (2, 4)
    fixed[9] = (1, 1)
    fixed[17] = (xdim + 2, 3)                           # beyond the map's edge: the units within the radius of it learn
    fixed[40] = (4, ydim + 30)                          # out of everybody's reach
    ini = make_maps(x, 3, xdim * ydim, 7)
    ini[:, 20] = ini[:, 11]                             # duplicate rows: ties go to the lowest index
    ini[:, 50] = ini[:, 11]
    got, ti, td = check_set(eng, E, oracle, ini, xdim, ydim, HEXA, neigh, x, 400, 0.08, 4.0, mask=mask, weight=weight, fixed=fixed,
                            use_fixed=1, use_weights=1, ref=ref)
    assert (ti[:, 5] == -2).all() and (ti[:, 9] == -3).all() and (ti[:, 17] == -3).all() and (ti[:, 3] == -3).all()
    # the same data without using fixed points or weights, masks only
    check_set(eng, E, oracle, ini, xdim, ydim, RECT, neigh, x, 250, 0.08, 4.0, mask=mask, weight=weight, fixed=fixed)
    # exact duplicates that stay duplicates while the bubble covers the whole map (every unit then gets every update): the
    # radius falls from 40 to 1 over 60 iterations and is above the map's diagonal, sqrt(8^2 + 6^2) = 10, before iteration 46
    same = np.repeat(ini[:, :1], xdim * ydim, axis=1).copy()
    _, si, _ = check_set(eng, E, oracle, same, xdim, ydim, RECT, BUBBLE, x, 60, 0.05, 40.0)
    assert (si[:, :40] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 200])
def test_winners_of_every_map(eng, E, oracle, count):
    rs = np.random.RandomState(count)
    x, _ = synth(25, 200, 6)
    mask = (rs.rand(200, 6) < 0.3).astype(np.uint8)
    mask[0] = 1
    for (xdim, ydim), T in (((12, 8), 4), ((35, 30), 2), ((1, 1), 3)):
        ini = make_maps(x, T, xdim * ydim, count)
        ini[:, -1] = ini[:, 0]                         # a tie: the lower index wins
        ms = E.MapSet(eng, ini, HEXA, BUBBLE, xdim, ydim)
        for mk in (None, mask):
            ds = E.Dataset(eng, x, mask=mk)
            for first in (0, 190):                      # (the second run wraps round the end of the data)
                gi, gd, gr = ms.winners(ds, first=first, count=count)
                rows = (first + np.arange(count)) % 200
                for m in range(T):
                    oi, od, orr = oracle.winners(ini[m], x[rows], mask=None if mk is None else mk[rows])
                    assert np.array_equal(gi[m], oi[:, 0]) and np.array_equal(bits(gd[m]), bits(od[:, 0])), (xdim, m, first)
                    assert np.array_equal(gr[m], orr)
                if mk is not None and first == 0:
                    assert (gr[:, 0] == 0).all() and (gi[:, 0] == -2).all()
            ds.close()
        ms.close()


@pytest.mark.gpu
def test_refusals_leave_the_engine_working(eng, E, oracle):
    from som_lvq_pak_amd import _lib
    x, _ = synth(26, 120, 5)
    ini = make_maps(x, 3, 96, 9)
    ds = E.Dataset(eng, x)
    other = E.Dataset(eng, np.zeros((10, 6), np.float32))
    good = E.MapSet(eng, ini, HEXA, BUBBLE, 12, 8)
    lib = eng.lib
    fp = _lib.c_float_p

    def train(ms_h, ds_h, batch=1, count=50, start=0, length=50):
        p = _lib.SomParams(length, 0.05, 3.0, 1, 0, 0, batch, start, count, 0)
        return lib.somhip_mapset_train(ms_h, ds_h, C.byref(p), None, None)

    def refused(rc, *words):
        msg = lib.somhip_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg

    h = C.c_void_p()
    mk = lambda *a: lib.somhip_mapset_create(*a, C.byref(h))          # noqa: E731
    rows = ini.ctypes.data_as(fp)
    refused(mk(None, rows, 3, 96, 5, HEXA, BUBBLE, 12, 8), "null")
    refused(mk(eng.h, None, 3, 96, 5, HEXA, BUBBLE, 12, 8), "null")
    refused(lib.somhip_mapset_create(eng.h, rows, 3, 96, 5, HEXA, BUBBLE, 12, 8, None), "null")
    refused(mk(eng.h, rows, 0, 96, 5, HEXA, BUBBLE, 12, 8), "0 maps")
    refused(mk(eng.h, rows, 3, 96, 5, HEXA, BUBBLE, 12, 9), "12x9", "96")
    refused(mk(eng.h, rows, 3, 96, 5, 2, 0, 12, 8), "topology")
    refused(mk(eng.h, rows, 3, 96, 5, HEXA, 0, 12, 8), "SOM parameters")
    big = np.zeros((1, 33 * 32, 32), np.float32)
    refused(mk(eng.h, big.ctypes.data_as(fp), 1, 33 * 32, 32, HEXA, BUBBLE, 33, 32), str(1088 * 32 * 4), str(BUDGET))
    refused(train(None, ds.h), "null")
    refused(train(good.h, None), "null")
    refused(lib.somhip_mapset_train(good.h, ds.h, None, None, None), "null")
    refused(train(good.h, ds.h, batch=2), "batch 2")
    refused(train(good.h, ds.h, batch=-1), "batch")
    refused(train(good.h, other.h), "dimension")
    refused(train(good.h, ds.h, count=60), "outside schedule")
    refused(lib.somhip_mapset_winners(good.h, other.h, 0, 5, None, None, None), "dimension")
    refused(lib.somhip_mapset_winners(good.h, ds.h, 0, 5, None, None, None), "null")
    refused(lib.somhip_mapset_download(good.h, 2, 2, rows), "outside")
    refused(lib.somhip_mapset_upload(good.h, 0, 1, None), "null")
    # a set whose engine was destroyed: every call refuses, its own destroy is still fine
    e2 = E.Engine(0)
    orphan, ds2 = C.c_void_p(), E.Dataset(e2, x)
    assert lib.somhip_mapset_create(e2.h, rows, 3, 96, 5, HEXA, BUBBLE, 12, 8, C.byref(orphan)) == 0
    ds2_h = ds2.h
    lib.somhip_engine_destroy(e2.h)
    e2.h = None
    refused(train(orphan, ds.h), "destroyed")
    refused(lib.somhip_mapset_download(orphan, 0, 1, rows), "destroyed")
    refused(train(good.h, ds2_h), "destroyed")
    lib.somhip_mapset_destroy(orphan)
    lib.somhip_dataset_destroy(ds2_h)
    ds2.h = None
    # after all of it the good set is untouched and trains correctly on the same engine
    assert np.array_equal(bits(good.download()), bits(ini))
    good.close()
    other.close()
    ds.close()
    check_set(eng, E, oracle, ini, 12, 8, HEXA, BUBBLE, x, 120, 0.05, 3.0)
