"""Update mode gemm (kernels/som_update_gemm.hpp) against a float64 replay of the run, at the edges where it can go wrong.

The yardstick is tests/helpers/som_replay.py: the reference's mini-batch semantics written out once in NumPy, winners
given.  Its float32 form is checked first, on the CPU, against the batch oracle BIT FOR BIT -- hexa and rect, bubble and
gaussian, linear and inverse_t, weights, fixed points inside and far beyond the map, runs that start mid-schedule and
wrap the data, rates above 1 -- and only then is its float64 form trusted to judge the matrix-pipe kernel.

On the GPU every case runs one batch (batch = count = B) in exact mode and in gemm mode from the same codebook: the
winner traces must be equal, exact mode must equal the oracle's bits (or, where the oracle cannot replay the schedule,
the float32 replay's, which equal them), and gemm mode must lie within ALLOW of the float64 replay, element by element:

    allow[u, i] = max(2 err_exact[u], 12 sqrt(hits[u]) 2^-24, 3e-6) * scale

err_exact[u] is the exact kernels' own largest error on unit u against the same replay (relative to scale = the largest
|c| of the exact result), hits[u] the unit's hits in the run.  That is the bound tools/fuzz_gemm.py measured over
~56 000 random cases (profiles/r02_fuzz_gemm.txt), with the unit's hits in place of the run length: never looser.  No
element-wise term in S (P0 |c| + sum |w_j| |x_j|) was needed: the measured worst of gemm error / allow over this table
is printed by each case (ALLOW_RATIO): measured on MI355X, at most 0.15 (fix_gauss_rect_kept; run_max 0.085 with 14 495
hits on one unit).  The faults of test_allowance_sees_seeded_faults are all
outside it.

Where gemm mode must not apply (a gaussian fixed point beyond lattice coordinate 1023, a rate outside [0, 1], a run of
more than GEMM_MAX_RUN samples, a map side above 1024 in gaussian) the matrix-pipe kernel must not run
(scan_stats()["gemm_entries"] unchanged) and the result must equal exact mode bit for bit.  Where it ran,
SOMHIP_GEMM_FULL_LISTS=1 (whole member lists instead of the tail the backward walk can reach) must give the same bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth
from helpers.som_replay import replay

GEMM_MAX_RUN = 65504          # kernels/som_update_gemm.hpp
EPS = 2.0 ** -24
HEXA, RECT, BUBBLE, GAUSS = 3, 4, 1, 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def make_inputs(seed, n, d, xd, yd, weights=False, fixed=None, every=5, same=False):
    """seeded data, weights 0..5, every `every`-th sample fixed at one of `fixed` in turn, an initial codebook"""
    x, _ = synth(seed, n, d)
    if same:
        x[:] = x[0]
    rs = np.random.RandomState(seed + 1)
    wt = rs.randint(0, 6, n).astype(np.int16) if weights else None
    fx = None
    if fixed:
        fx = np.full((n, 2), -1, dtype=np.int16)
        for k, r in enumerate(range(1, n, every)):
            fx[r] = fixed[k % len(fixed)]
    lo, hi = x.min(axis=0), x.max(axis=0)
    ini = (lo + (hi - lo) * rs.rand(xd * yd, d)).astype(np.float32)
    return x, wt, fx, ini


def allowance(exact, r64, hits, scale):
    err_exact = np.abs(exact.astype(np.float64) - r64).max(axis=1) / scale
    per_unit = np.maximum(np.maximum(2.0 * err_exact, 12.0 * np.sqrt(hits) * EPS), 3e-6) * scale
    return per_unit[:, None]


# ------------------------------------------------------------------ CPU: the replay is the oracle, bit for bit
FAR = [(3, 4), (12, 2), (13, 0), (0, 9), (1030, 5), (32767, 32767), (5, 2000), (40, 3), (1023, 7)]


@pytest.mark.parametrize("topol,neigh,alpha_type,alpha,radius,B,length,n,weights,fixed", [
    (HEXA, BUBBLE, 1, 0.05, 4.0, 17, 500, 200, False, None),
    (RECT, BUBBLE, 1, 0.3, 6.0, 1, 150, 60, True, FAR),
    (HEXA, GAUSS, 2, 0.5, 6.0, 1, 120, 50, False, FAR),
    (RECT, GAUSS, 1, 0.05, 3.0, 100, 500, 200, True, None),
    (HEXA, BUBBLE, 2, 0.2, 12.0, 300, 900, 250, True, FAR),         # runs start mid-schedule and wrap the data
    (HEXA, GAUSS, 1, 0.6, 3000.0, 300, 700, 200, True, FAR),        # radius reaching every fixed point
    (HEXA, BUBBLE, 1, 1.5, 30.0, 300, 700, 200, True, FAR),         # rates above 1
    (RECT, GAUSS, 1, 1.5, 8.0, 17, 300, 200, True, FAR),
    (HEXA, BUBBLE, 1, 0.05, 2500.0, 64, 256, 100, False, FAR),      # a bubble that reaches (1030, 5) and (5, 2000)
])
def test_float32_replay_equals_batch_oracle_bits(oracle, topol, neigh, alpha_type, alpha, radius, B, length, n, weights, fixed):
    """tests/helpers/som_replay.py in float32 == orc_som_training(batch=B), bit for bit, run by run over the whole
    schedule, winners from the oracle's own trace (fixed samples traced as -3)"""
    xd, yd, d = 12, 9, 16
    x, wt, fx, ini = make_inputs(31, n, d, xd, yd, weights, fixed)
    use = 1 if fixed else 0
    want, ti, _ = oracle.som_train(ini, xd, yd, topol, neigh, x, length, alpha, radius, alpha_type=alpha_type,
                                   weight=wt, fixed_xy=fx, fixed_on=use, weights_on=int(weights), batch=B)
    if fixed:
        assert (ti == -3).sum() == sum(1 for le in range(length) if fx[le % n][0] >= 0)
    c = ini
    for s in range(0, length, B):
        cnt = min(B, length - s)
        c = replay(c, xd, yd, topol, neigh, x, length, alpha, radius, ti[s:s + cnt], start_iter=s, count=cnt,
                   data_first=s % n, alpha_type=alpha_type, weight=wt, fixed_xy=fx, use_fixed=use,
                   use_weights=int(weights)).codes
    assert np.array_equal(bits(c), bits(want))


def _fault_case(neigh):
    """one batch of a longer schedule on a 32 x 24 hexa map with fixed points, a float32 (= exact) and float64 replay"""
    xd, yd, d, n, B = 32, 24, 128, 400, 256
    radius = 1012.0 if neigh == BUBBLE else 700.0          # (1030, 5) reaches part of the map, (6, 5) all of it
    fixed = [(1030, 5), (40, 3)]
    x, _, fx, ini = make_inputs(77, n, d, xd, yd, fixed=fixed, every=9)
    rs = np.random.RandomState(5)
    win = rs.randint(0, xd * yd, B)
    win[-1] = 3 * xd + 17
    win[[r for r in range(B) if fx[r][0] >= 0]] = -3
    kw = dict(xdim=xd, ydim=yd, topol=HEXA, neigh=neigh, data=x, length=2 * B, alpha=0.05, radius=radius, winners=win,
              start_iter=0, count=B, data_first=0, fixed_xy=fx, use_fixed=1)
    return kw, ini, fx


def _seeded_faults(kw, ini, fx, r64):
    busiest = int(np.argmax(r64.hits)) if kw["neigh"] == BUBBLE else int(kw["winners"][-1])
    for fault in (("drop", busiest, -1), ("swap", busiest, -2), ("next_rate", busiest, -1), "fixed_mod_1024"):
        if fault == "fixed_mod_1024":
            fx2 = fx.copy()
            fx2[:, 0] = np.where(fx2[:, 0] >= 0, fx2[:, 0] % 1024, fx2[:, 0])
            yield fault, replay(ini, **dict(kw, fixed_xy=fx2), dtype=np.float64).codes
        else:
            yield fault, replay(ini, **kw, dtype=np.float64, fault=fault).codes


@pytest.mark.parametrize("neigh", [BUBBLE, GAUSS])
def test_allowance_sees_seeded_faults(neigh):
    """The allowance is tight enough to see a wrong update: a float64 replay with one seeded fault -- a dropped hit of the
    busiest unit, two consecutive hits swapped, a fixed point's x taken mod 1024 (the 10-bit field of the gaussian GEMM
    entry), one hit's rate from the next iteration's schedule -- is outside it for at least one element, while the fault-free
    replay holds the correct result (the float32 replay, = the exact kernels = the oracle) well inside.  (The next-
    iteration rate is detectable here because the unit's LAST hit is taken: nothing damps it afterwards.)"""
    kw, ini, fx = _fault_case(neigh)
    r32 = replay(ini, **kw).codes
    r64 = replay(ini, **kw, dtype=np.float64)
    scale = float(np.abs(r32).max())
    allow = allowance(r32, r64.codes, r64.hits, scale)
    assert (np.abs(r32 - r64.codes) <= allow).all()
    for fault, bad in _seeded_faults(kw, ini, fx, r64):
        assert (np.abs(r32 - bad) > allow).any(), fault


# ------------------------------------------------------------------ GPU: gemm mode against the float64 replay
BIG_R = [(30000, 5), (32767, 32767)]
CASES = {
    # fixed points, gaussian: (40, 3) and (1023, 7) are kept by the gemm form; (1030, 5), (5, 2000), (32767, 32767) not
    "fix_gauss_hexa_kept": dict(xd=32, yd=24, topol=HEXA, neigh=GAUSS, radius=700.0, fixed=[(40, 3), (1023, 7)]),
    "fix_gauss_hexa_1030": dict(xd=32, yd=24, topol=HEXA, neigh=GAUSS, radius=700.0, fixed=[(40, 3), (1030, 5)], gemm=False),
    "fix_gauss_rect_kept": dict(xd=40, yd=16, topol=RECT, neigh=GAUSS, radius=700.0, d=256, fixed=[(1023, 7), (40, 3)]),
    "fix_gauss_rect_far": dict(xd=40, yd=16, topol=RECT, neigh=GAUSS, radius=700.0, d=256, fixed=[(5, 2000), (32767, 32767)], gemm=False),
    "fix_gauss_hexa_far": dict(xd=32, yd=24, topol=HEXA, neigh=GAUSS, radius=3000.0, fixed=[(32767, 32767), (1030, 5)], gemm=False),
    # fixed points, bubble: membership is K4b's, the same for both modes -- gemm always applies
    "fix_bubble_patch": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=12.0, fixed=FAR),
    "fix_bubble_linear": dict(xd=13, yd=9, topol=HEXA, neigh=BUBBLE, radius=12.0, fixed=FAR),
    # radius 30 000 (constant over the batch of a long schedule): K4b's 32-bit integer patch form would overflow
    "radius_30000_patch": dict(xd=16, yd=16, topol=HEXA, neigh=BUBBLE, radius=30000.0, length=64 * 512, fixed=BIG_R, every=2),
    "radius_30000_rect": dict(xd=16, yd=16, topol=RECT, neigh=BUBBLE, radius=30000.0, length=64 * 512, fixed=BIG_R, every=2),
    "radius_30000_linear": dict(xd=13, yd=9, topol=HEXA, neigh=BUBBLE, radius=30000.0, length=64 * 512, fixed=BIG_R, every=2),
    # weights 0..5 with fixed points in the same run
    "weights_bubble": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=8.0, weights=True, fixed=[(3, 4), (40, 3)]),
    "weights_gauss": dict(xd=40, yd=16, topol=RECT, neigh=GAUSS, radius=8.0, d=256, weights=True, fixed=[(3, 4), (40, 3)]),
    # schedule
    "inverse_t": dict(xd=24, yd=16, topol=HEXA, neigh=BUBBLE, radius=6.0, alpha=0.3, alpha_type=2, length=4096, it0=1000),
    "end_of_schedule": dict(xd=24, yd=16, topol=HEXA, neigh=BUBBLE, radius=5.0, B=256, length=100000, it0=100000 - 256),
    "alpha_1": dict(xd=24, yd=16, topol=HEXA, neigh=BUBBLE, radius=5.0, alpha=1.0),
    "alpha_1_5_bubble": dict(xd=24, yd=16, topol=HEXA, neigh=BUBBLE, radius=5.0, alpha=1.5, gemm=False),
    "alpha_1_5_gauss": dict(xd=24, yd=16, topol=HEXA, neigh=GAUSS, radius=3.0, alpha=1.5, gemm=False),
    "alpha_0_6_weights": dict(xd=24, yd=16, topol=HEXA, neigh=BUBBLE, radius=5.0, alpha=0.6, weights=True),
    # run shape
    "B1": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=6.0, B=1, batch=64, length=64, it0=5),   # (batch 1 is online)
    "B15": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=6.0, B=15),
    "B17_gauss": dict(xd=32, yd=24, topol=HEXA, neigh=GAUSS, radius=6.0, B=17),
    "B61": dict(xd=32, yd=24, topol=RECT, neigh=BUBBLE, radius=6.0, B=61),
    "B_over_n": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=6.0, n=40, B=100),
    "first_n_minus_3": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=6.0, n=300, B=200, first=297),
    "deep_start": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=20.0, length=20000, it0=18000, B=300),
    # run-length boundary
    "run_max": dict(xd=16, yd=16, topol=HEXA, neigh=BUBBLE, radius=3.0, n=4096, B=GEMM_MAX_RUN, units="subset"),
    "run_max_plus_1": dict(xd=16, yd=16, topol=HEXA, neigh=BUBBLE, radius=3.0, n=4096, B=GEMM_MAX_RUN + 1, gemm=False),
    # map shape
    "partial_group": dict(xd=13, yd=9, topol=RECT, neigh=BUBBLE, radius=3.0),
    "wide_1024_gauss": dict(xd=1024, yd=4, topol=HEXA, neigh=GAUSS, radius=40.0, B=48, units="subset"),
    "wide_1025_gauss": dict(xd=1025, yd=4, topol=HEXA, neigh=GAUSS, radius=40.0, B=48, gemm=False),
    "radius_half": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=0.5),
    "radius_beyond_diagonal": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=60.0),
    "one_winner": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=4.0, same=True),
    # dims / slices
    "d256": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=8.0, d=256),
    "d384": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=8.0, d=384),
    "d640": dict(xd=32, yd=24, topol=RECT, neigh=BUBBLE, radius=8.0, d=640),
    "d1024": dict(xd=32, yd=24, topol=HEXA, neigh=BUBBLE, radius=30.0, d=1024, B=400),
    "gauss_d512": dict(xd=32, yd=24, topol=HEXA, neigh=GAUSS, radius=6.0, d=512),
    "gauss_d1024": dict(xd=24, yd=16, topol=RECT, neigh=GAUSS, radius=6.0, d=1024),
    "small_map_d512": dict(xd=8, yd=8, topol=HEXA, neigh=BUBBLE, radius=3.0, d=512),
}


def _busiest_subset(r_hits_all, xd, yd, fixed, radius, rs):
    """>= 64 units: random ones, the busiest, the last row group's rows, every unit within the radius of a fixed point"""
    nu = xd * yd
    pick = set(rs.choice(nu, 64, replace=False).tolist())
    pick.add(int(np.argmax(r_hits_all)))
    pick.update(range(max(0, nu - 64 - (nu % 64)), nu))
    for fx, fy in fixed or []:
        u = np.arange(nu)
        near = np.hypot(u % xd - fx, (u // xd - fy) * 0.8660254) <= radius + 1
        pick.update(np.nonzero(near)[0].tolist())
    return np.array(sorted(pick))


def _run(eng, E, ini, cs, ds, mode, monkeypatch, full=False):
    eng.set_update_mode(mode)
    if full:
        monkeypatch.setenv("SOMHIP_GEMM_FULL_LISTS", "1")
    try:
        cb = E.Codebook(eng, ini, cs["topol"], cs["neigh"], cs["xd"], cs["yd"])
        plan = E.update_plan(cb, ds, cs["length"], cs["alpha"], cs["radius"], cs["B"], alpha_type=cs["alpha_type"],
                             use_fixed=cs["use_fixed"], use_weights=cs["use_weights"], start_iter=cs["it0"],
                             data_first=cs["first"])
        s0 = eng.scan_stats()["gemm_entries"]
        ti, _ = E.som_train(cb, ds, cs["length"], cs["alpha"], cs["radius"], alpha_type=cs["alpha_type"],
                            use_fixed=cs["use_fixed"], use_weights=cs["use_weights"], batch=cs.get("batch", cs["B"]), start_iter=cs["it0"],
                            count=cs["B"], data_first=cs["first"])
        ran = eng.scan_stats()["gemm_entries"] - s0
        out = cb.download()
        cb.close()
    finally:
        eng.set_update_mode("exact")
        monkeypatch.delenv("SOMHIP_GEMM_FULL_LISTS", raising=False)
    return out, ti, ran, plan


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gemm_update_against_float64_replay(eng, E, oracle, monkeypatch, name):
    cs = dict(d=128, n=600, B=512, alpha=0.05, alpha_type=1, it0=0, weights=False, fixed=None, every=5, gemm=True,
              same=False, units="all")
    cs.update(CASES[name])
    cs.setdefault("length", cs["B"])
    cs.setdefault("first", cs["it0"] % cs["n"])
    cs["use_fixed"], cs["use_weights"] = int(bool(cs["fixed"])), int(cs["weights"])
    xd, yd = cs["xd"], cs["yd"]
    x, wt, fx, ini = make_inputs(1000 + sorted(CASES).index(name), cs["n"], cs["d"], xd, yd, cs["weights"], cs["fixed"],
                                 cs["every"], cs["same"])
    ds = E.Dataset(eng, x, weight=wt, fixed_xy=fx)
    exact, ti_e, ran_e, _ = _run(eng, E, ini, cs, ds, "exact", monkeypatch)
    gemm, ti_g, ran_g, plan_g = _run(eng, E, ini, cs, ds, "gemm", monkeypatch)
    assert ran_e == 0
    assert np.array_equal(ti_e, ti_g), name
    kw = dict(xdim=xd, ydim=yd, topol=cs["topol"], neigh=cs["neigh"], data=x, length=cs["length"], alpha=cs["alpha"],
              radius=cs["radius"], winners=ti_e, start_iter=cs["it0"], count=cs["B"], data_first=cs["first"],
              alpha_type=cs["alpha_type"], weight=wt, fixed_xy=fx, use_fixed=cs["use_fixed"], use_weights=cs["use_weights"])
    # the control: exact mode == the oracle's bits where it can replay the schedule, else == the float32 replay (which
    # equals the oracle: test_float32_replay_equals_batch_oracle_bits)
    oracle_ok = cs["it0"] == 0 and cs["first"] == 0 and cs["length"] == cs["B"]
    if oracle_ok:
        want, wi, _ = oracle.som_train(ini, xd, yd, cs["topol"], cs["neigh"], x, cs["length"], cs["alpha"], cs["radius"],
                                       alpha_type=cs["alpha_type"], weight=wt, fixed_xy=fx, fixed_on=cs["use_fixed"],
                                       weights_on=cs["use_weights"], batch=cs["B"])
        assert np.array_equal(ti_e, wi), name
        assert np.array_equal(bits(exact), bits(want)), name
    if not cs["gemm"]:
        assert ran_g == 0 and plan_g["apply"] != "gemm", name   # the matrix-pipe kernel did not run ...
        assert np.array_equal(bits(gemm), bits(exact)), name   # ... and the fallback is the exact kernels
        if not oracle_ok:
            assert np.array_equal(bits(exact), bits(replay(ini, **kw).codes)), name
        ds.close()
        return
    assert ran_g > 0, name                                # the matrix-pipe kernel really ran
    full, ti_f, ran_f, _ = _run(eng, E, ini, cs, ds, "gemm", monkeypatch, full=True)
    ds.close()
    assert np.array_equal(ti_f, ti_g) and np.array_equal(bits(full), bits(gemm)), name   # tail lists == whole lists
    units = None
    if cs["units"] == "subset":
        counts = np.bincount(ti_e[ti_e >= 0], minlength=xd * yd)     # the busiest unit is (near) the commonest winner
        units = _busiest_subset(counts, xd, yd, cs["fixed"], cs["radius"], np.random.RandomState(3))
        assert len(units) >= 64
    r64 = replay(ini, **kw, dtype=np.float64, units=units)
    sel = slice(None) if units is None else units
    if not oracle_ok:
        assert np.array_equal(bits(exact[sel]), bits(replay(ini, **kw, units=units).codes)), name
    scale = float(np.abs(exact).max())
    allow = allowance(exact[sel], r64.codes, r64.hits, scale)
    err = np.abs(gemm[sel].astype(np.float64) - r64.codes)
    print("ALLOW_RATIO %s %.3f (max hits %d)" % (name, float((err / allow).max()), int(r64.hits.max())))
    assert np.isfinite(gemm).all(), name
    assert (err <= allow).all(), (name, float((err / allow).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSS])
def test_gemm_result_is_outside_the_allowance_of_a_faulted_replay(eng, E, monkeypatch, neigh):
    """test_allowance_sees_seeded_faults with the kernel's own result: the gemm codebook of the fault case's batch is
    within the allowance of the correct float64 replay and outside that of every seeded fault"""
    kw, ini, fx = _fault_case(neigh)
    x = kw["data"]
    ds = E.Dataset(eng, x, fixed_xy=fx)
    cs = dict(xd=kw["xdim"], yd=kw["ydim"], topol=HEXA, neigh=neigh, length=kw["length"], alpha=kw["alpha"],
              radius=kw["radius"], alpha_type=1, use_fixed=1, use_weights=0, B=kw["count"], it0=0, first=0)
    exact, ti, _, _ = _run(eng, E, ini, cs, ds, "exact", monkeypatch)
    gemm, ti_g, ran, _ = _run(eng, E, ini, cs, ds, "gemm", monkeypatch)
    ds.close()
    assert np.array_equal(ti, ti_g)
    kw = dict(kw, winners=ti)
    if neigh == GAUSS:
        assert ran == 0 and np.array_equal(bits(gemm), bits(exact))   # (1030, 5): the exact kernels take this run
    else:
        assert ran > 0
    r64 = replay(ini, **kw, dtype=np.float64)
    scale = float(np.abs(exact).max())
    allow = allowance(exact, r64.codes, r64.hits, scale)
    assert (np.abs(gemm - r64.codes) <= allow).all()
    for fault, bad in _seeded_faults(kw, ini, fx, r64):
        assert (np.abs(gemm - bad) > allow).any(), fault


# ------------------------------------------------------------------ GPU: shards in gemm mode, gaussian fixed points
@pytest.mark.gpu
def test_gemm_gaussian_fixed_points_shard_identically(eng, E):
    """a row-offset shard pair and an interleaved 3-way shard in gemm mode, gaussian, with fixed points the gemm form keeps,
    give the unsharded gemm bits"""
    from som_lvq_pak_amd._lib import SomParams
    xd, yd, d, n, B = 32, 24, 128, 1024, 512
    x, _, fx, ini = make_inputs(55, n, d, xd, yd, fixed=[(40, 3), (1023, 7), (5, 5)], every=4)
    ds = E.Dataset(eng, x, fixed_xy=fx)
    eng.set_update_mode("gemm")
    try:
        cb = E.Codebook(eng, ini, HEXA, GAUSS, xd, yd)
        s0 = eng.scan_stats()["gemm_entries"]
        E.som_train(cb, ds, 2 * B, 0.05, 700.0, use_fixed=1, batch=B, trace=False)
        assert eng.scan_stats()["gemm_entries"] > s0
        whole = cb.download()
        cb.close()
        cut = 8 * xd * 1                                  # an 8-row boundary: both halves in patch order
        layouts = {
            "row_offset": [(np.arange(0, cut), dict(row_offset=0, n_global=xd * yd)),
                           (np.arange(cut, xd * yd), dict(row_offset=cut, n_global=xd * yd))],
            "interleaved": [(E.shard_units(xd, yd, r, 3, eng.lib), dict(interleave=(r, 3))) for r in range(3)],
        }
        p = SomParams(2 * B, 0.05, 700.0, 1, 1, 0, B, 0, 2 * B, 0)
        for tag, lay in layouts.items():
            shards = [(u, E.Codebook(eng, ini[u], HEXA, GAUSS, xd, yd, **k)) for u, k in lay]
            kb = eng.device_alloc(8 * B)
            s0 = eng.scan_stats()["gemm_entries"]
            for it0 in range(0, 2 * B, B):
                ks = []
                for _, s in shards:
                    E.check(eng.lib.somhip_batch_winner_keys(s.h, ds.h, it0 % n, B, kb))
                    k = np.empty(B, dtype=np.uint64)
                    E.check(eng.lib.somhip_copy_to_host(eng.h, k.ctypes.data_as(C.c_void_p), kb, 8 * B))
                    ks.append(k)
                merged = ks[0]
                for k in ks[1:]:
                    merged = np.minimum(merged, k)
                E.check(eng.lib.somhip_copy_to_device(eng.h, kb, merged.ctypes.data_as(C.c_void_p), 8 * B))
                for _, s in shards:
                    E.check(eng.lib.somhip_som_batch_update(s.h, ds.h, C.byref(p), it0, B, it0 % n, kb))
            eng.sync()
            eng.device_free(kb)
            assert eng.scan_stats()["gemm_entries"] > s0, tag
            full = np.empty_like(whole)
            for u, s in shards:
                full[u] = s.download()
                s.close()
            assert np.array_equal(bits(full), bits(whole)), tag
    finally:
        eng.set_update_mode("exact")
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xd,yd,topol", [(16, 16, HEXA), (16, 16, RECT), (13, 9, HEXA)])
def test_exact_mode_radius_30000_equals_oracle(eng, E, oracle, xd, yd, topol):
    """radius 30 000 with fixed points at (30000, 5) (members while the radius is above ~29 985) and (32767, 32767) (never a
    member, ~43 000 away): K4b's membership -- the 8x8-patch integer form (16 x 16) and the linear-order per-unit form
    (13 x 9) -- must stay the reference's, whole schedule, exact mode == the oracle's bits"""
    B, L = 512, 4096
    x, _, fx, ini = make_inputs(91, 700, 128, xd, yd, fixed=BIG_R, every=2)
    want, wi, _ = oracle.som_train(ini, xd, yd, topol, BUBBLE, x, L, 0.05, 30000.0, fixed_xy=fx, fixed_on=1, batch=B)
    cb, ds = E.Codebook(eng, ini, topol, BUBBLE, xd, yd), E.Dataset(eng, x, fixed_xy=fx)
    ti, _ = E.som_train(cb, ds, L, 0.05, 30000.0, use_fixed=1, batch=B)
    got = cb.download()
    cb.close(); ds.close()
    assert np.array_equal(ti, wi)
    assert np.array_equal(bits(got), bits(want))
