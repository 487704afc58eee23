"""The lazy search of somhip_som_train's mini-batch loop (host_som.inc, som_lazy_run): in update mode gemm with the
lists' tails only, a run's last M samples are searched, K4b runs over exactly those trips, and the rest of the run is
searched only if some row group's tail did not fill.  Either way the codebook must be, bit for bit, what the same
batches give when every winner is known: somhip_batch_winner_keys + somhip_som_batch_update (the step API never takes
the lazy path), and the lists the statistics describe must be the same lists.

M is whole K4b trips (members_nt x members_rr) and at most half the run.  A map below 512 row groups takes trips of
1024 x 4 from 1025 samples on (som_update_plan, `wide`), so the 32 x 32 map at batch 4096 has ONE trip per run and is
never lazy: that shape is kept here as the non-lazy control (samples grow by every vector trained), and the lazy cases
run on a 256 x 128 map (512 row groups: trips of 256 x 4) at radius 180, where the rule gives M = 3072 for a first batch:
quarter = 0.25 x 3.6276 x 174^2 / 32768 = 0.84, tail_need = 342 .. 345, 7 x 345 / 0.84 = 2880 -> three trips.
Trips of 1024 x 8: on maps of 512 row groups and more the plan takes them only where tail_need > 3072 x full, where the
rule wants M > 86016 samples -- no such run is lazy.  A map BELOW 512 row groups takes them from 16384 samples on whatever
the radius: 32 x 32 at batch 16384 or 32768 and radius 36 (quarter = 0.25 x 3.6276 x 30^2 / 1024 = 0.80, M = one trip of
8192) is lazy through k_som_members<false, 1024, 8, true>: satisfied, second path and statistics at that shape below.
Needs an MI355X:  pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEXA, BUBBLE = 3, 1
L, ALPHA, DIM = 1000000, 0.05, 128
RADIUS = 180.0
STATS = ("row_updates", "group_updates", "gemm_entries")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    e.set_update_mode("gemm")
    yield e
    e.close()


@pytest.fixture(scope="module")
def spread():
    """6000 rows of dim 128 without clusters (winners all over a map) and a 256 x 128 map of rows near data rows"""
    rs = np.random.RandomState(41)
    x = rs.standard_normal((6000, DIM)).astype(np.float32)
    ini = (x[rs.randint(0, 6000, 256 * 128)] + 0.3 * rs.standard_normal((256 * 128, DIM))).astype(np.float32)
    return x, ini


def cuts(batch, start, count):
    """the runs somhip_som_train makes of iterations [start, start + count): cut at the schedule's batch boundaries"""
    it = start
    while it < start + count:
        c = min(batch - it % batch, start + count - it)
        yield it, c
        it += c


def step_driver(eng, E, cb, ds, radius, batch, start, count, data_first):
    """the non-lazy driver: every key of every run, then the update; returns the keys of the whole call"""
    from som_lvq_pak_amd._lib import SomParams
    p = SomParams(L, ALPHA, radius, 0, 0, 0, batch, start, count, data_first)
    dk = eng.device_alloc(8 * batch)
    keys = np.empty(count, dtype=np.uint64)
    try:
        for it0, c in cuts(batch, start, count):
            first = (data_first + it0 - start) % ds.n
            E.check(eng.lib.somhip_batch_winner_keys(cb.h, ds.h, first, c, dk))
            E.check(eng.lib.somhip_som_batch_update(cb.h, ds.h, C.byref(p), it0, c, first, dk))
            hk = np.empty(c, dtype=np.uint64)
            E.check(eng.lib.somhip_copy_to_host(eng.h, hk.ctypes.data_as(C.c_void_p), dk, 8 * c))
            keys[it0 - start:it0 - start + c] = hk
    finally:
        eng.device_free(dk)
    return keys


def both(eng, E, x, ini, xd, yd, radius, batch, start=0, count=None, data_first=0, trace=False):
    """somhip_som_train and the step driver on the same call: codebooks, statistics deltas, trace and keys"""
    count = batch if count is None else count
    ds = E.Dataset(eng, x)
    out = {}
    try:
        for tag in ("train", "steps"):
            cb = E.Codebook(eng, ini, HEXA, BUBBLE, xd, yd)
            try:
                s0 = eng.scan_stats()
                if tag == "train":
                    out["trace"] = E.som_train(cb, ds, L, ALPHA, radius, batch=batch, start_iter=start, count=count,
                                               data_first=data_first, trace=trace)
                else:
                    out["keys"] = step_driver(eng, E, cb, ds, radius, batch, start, count, data_first)
                s1 = eng.scan_stats()
                out[tag] = cb.download()
                out[tag + "_stats"] = {k: s1[k] - s0[k] for k in STATS + ("samples",)}
            finally:
                cb.close()
        cb = E.Codebook(eng, ini, HEXA, BUBBLE, xd, yd)
        try:
            out["plan"] = E.update_plan(cb, ds, L, ALPHA, radius, min(batch, count), start_iter=start, data_first=data_first)
        finally:
            cb.close()
    finally:
        ds.close()
    print("LAZY %dx%d radius %g batch %d start %d count %d first %d: searched %d of %d, stats %s" % (
        xd, yd, radius, batch, start, count, data_first, out["train_stats"]["samples"], count,
        {k: out["train_stats"][k] for k in STATS}))
    assert out["steps_stats"]["samples"] == count
    assert np.array_equal(bits(out["train"]), bits(out["steps"]))
    for k in STATS:
        assert out["train_stats"][k] == out["steps_stats"][k], k
    return out


def gemm_tail(plan, trip):
    return plan["apply"] == "gemm" and plan["tail"] and plan["tail_need"] > 0 and plan["members_nt"] * plan["members_rr"] == trip


def test_lazy_satisfied(eng, E, spread):
    """three batches of 8192 at radius 180 on the 256 x 128 map: M = 3072 or 4096, the tails fill (winners all over the map)"""
    x, ini = spread
    out = both(eng, E, x, ini, 256, 128, RADIUS, 8192, count=3 * 8192)
    assert gemm_tail(out["plan"], 1024) and out["plan"]["decode"], out["plan"]
    assert out["train_stats"]["samples"] < 3 * 8192


def test_lazy_falls_back(eng, E, spread):
    """the same plan, every winner in one corner (copies of one code row plus tiny noise): the patches further than the
    radius from that corner (x > 180 of 256) never fill, the rest of every run is searched after all"""
    _, ini = spread
    rs = np.random.RandomState(42)
    x = (ini[0][None, :] + 1e-4 * rs.standard_normal((6000, DIM))).astype(np.float32)
    out = both(eng, E, x, ini, 256, 128, RADIUS, 8192, count=2 * 8192)
    assert gemm_tail(out["plan"], 1024), out["plan"]
    assert out["train_stats"]["samples"] == 2 * 8192


@pytest.mark.parametrize("corner", [False, True])
def test_one_trip_runs_are_never_lazy(eng, E, corner):
    """32 x 32 (16 row groups), batch 4096, radius 24: the plan's trips are 1024 x 4 = the run, so the search is whole"""
    rs = np.random.RandomState(43)
    x = rs.standard_normal((6000, DIM)).astype(np.float32)
    ini = (x[rs.randint(0, 6000, 1024)] + 0.3 * rs.standard_normal((1024, DIM))).astype(np.float32)
    if corner:
        x = (ini[0][None, :] + 1e-4 * rs.standard_normal((6000, DIM))).astype(np.float32)
    out = both(eng, E, x, ini, 32, 32, 24.0, 4096, count=3 * 4096)
    assert gemm_tail(out["plan"], 4096), out["plan"]
    assert out["train_stats"]["samples"] == 3 * 4096


@pytest.mark.parametrize("name,batch,start,count,first", [
    ("not_whole_trips", 7003, 0, 7003, 0),            # 6.8 trips, keys decoded in K4b; the key array is shifted by one (7003 % 4 = 3)
    ("shorter_than_a_trip", 1000, 0, 1000, 0),        # one trip: never lazy
    ("starts_mid_batch", 8192, 1001, 7191, 17),       # iterations 1001 .. 8191 of the first batch (shifted by one)
    ("mid_batch_then_whole", 8192, 1001, 7191 + 8192, 17),
    ("tail_wraps_the_data", 8192, 0, 8192, 500),      # the searched end is rows 5620 .. 5999, 0 .. 2691
    ("run_wraps_before_the_tail", 8192, 0, 8192, 2000),          # ... rows 1120 .. 4191, the run wraps in front of it
])
def test_edges(eng, E, spread, name, batch, start, count, first):
    x, ini = spread
    out = both(eng, E, x, ini, 256, 128, RADIUS, batch, start=start, count=count, data_first=first)
    if name == "shorter_than_a_trip":
        assert out["train_stats"]["samples"] == count
    else:
        assert gemm_tail(out["plan"], 1024), out["plan"]
        assert out["train_stats"]["samples"] < count, name


@pytest.fixture(scope="module")
def small():
    """6000 rows without clusters and a 32 x 32 map of rows near data rows"""
    rs = np.random.RandomState(44)
    x = rs.standard_normal((6000, DIM)).astype(np.float32)
    ini = (x[rs.randint(0, 6000, 1024)] + 0.3 * rs.standard_normal((1024, DIM))).astype(np.float32)
    return x, ini


WIDE = 8192


@pytest.mark.parametrize("batch,count", [(16384, 2 * 16384), (32768, 32768), (16384 + 5, 16384 + 5)])
def test_wide_trips_satisfied(eng, E, small, batch, count):
    """trips of 1024 x 8 on 16 row groups: one trip of two (of four, of 2.0006: the key array shifted) is searched; the
    first run starts from a map of scattered rows (winners everywhere), so it at least keeps its first pass"""
    x, ini = small
    out = both(eng, E, x, ini, 32, 32, 36.0, batch, count=count)
    assert gemm_tail(out["plan"], WIDE) and out["plan"]["decode"], out["plan"]
    assert out["train_stats"]["samples"] < count
    if count == batch:
        assert out["train_stats"]["samples"] == WIDE


@pytest.mark.parametrize("batch", [16384, 32768])
def test_wide_trips_fall_back(eng, E, small, batch):
    """every winner at unit (0, 0): the far corner patch has units further than the radius (41.4 > 36), never fills.  One
    run: after it every unit near that corner equals the data to 1e-4 and the next run's winners may lie anywhere."""
    _, ini = small
    rs = np.random.RandomState(45)
    x = (ini[0][None, :] + 1e-4 * rs.standard_normal((6000, DIM))).astype(np.float32)
    out = both(eng, E, x, ini, 32, 32, 36.0, batch, count=batch)
    assert gemm_tail(out["plan"], WIDE) and out["plan"]["decode"], out["plan"]
    assert out["train_stats"]["samples"] == batch


def test_trace_wanted_searches_everything(eng, E, spread):
    """with a trace every winner and distance comes back: the step API's keys"""
    x, ini = spread
    out = both(eng, E, x, ini, 256, 128, RADIUS, 8192, count=2 * 8192, trace=True)
    ti, td = out["trace"]
    assert out["train_stats"]["samples"] == 2 * 8192
    assert np.array_equal(ti.astype(np.uint32), (out["keys"] & 0xFFFFFFFF).astype(np.uint32))
    assert np.array_equal(td.view(np.uint32), (out["keys"] >> 32).astype(np.uint32))
