"""K4b (k_som_members) on the runs that newly take its two-phase form -- 8192 to 16383 iterations on maps of 512 row
groups and more (som_update_plan: decoded winners, one trip of 1024 x 8 samples) -- and on trips that hold every kind of
winner at once: far from the row group, with the whole 8 x 8 patch inside the neighbourhood, on its boundary, fixed
points at a patch corner, on a patch edge, one unit outside the map, far outside it and beyond the integer form's
guards, skipped samples.

Update mode exact against the batch oracle: a wrong mask bit, a missing entry or a wrong order changes the codebook's
bits, so array_equal on the uint32 view compares every member decision; the statistics words (row_updates,
group_updates) are held to a numpy count of the (row, iteration) members, made from the reference's own distance
(hexa_dist / rect_dist in the oracle's arithmetic, restated below) and the winner trace.  The gemm-mode case, where the
number of FULL entries decides where a list's tail ends, goes through the float64 replay and the allowance of
tests/test_gemm_replay.py.  Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

import test_gemm_replay as GR
from conftest import synth
from helpers.som_replay import replay

pytestmark = pytest.mark.gpu

HEXA, RECT, BUBBLE = 3, 4, 1


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


def radii(length, radius, count):
    """orc_som_radius of iterations 0 .. count - 1: evaluated in double, narrowed on assignment"""
    it = np.arange(count)
    left = (length - it).astype(np.float32).astype(np.float64)
    return (1.0 + (float(np.float32(radius)) - 1.0) * left / float(np.float32(length))).astype(np.float32)


def member_counts(xd, yd, topol, bx, by, trad):
    """((row, iteration) members, (row group, iteration) pairs with a member) of a run on a map in 8 x 8 patch order:
    winners at (bx, by) [count] (bx < 0: the iteration teaches nothing), radii trad [count], the reference's distance"""
    reach = int(np.ceil(float(trad.max()) / 0.8660254)) + 2
    off = np.arange(-reach, reach + 1)
    rows = pairs = 0
    for s in range(0, len(bx), 512):
        sl = slice(s, s + 512)
        ok = bx[sl] >= 0
        wx, wy, tr = bx[sl][ok].astype(np.int64), by[sl][ok].astype(np.int64), trad[sl][ok]
        tx = wx[:, None, None] + off[None, None, :]
        ty = wy[:, None, None] + off[None, :, None]
        tx, ty = np.broadcast_arrays(tx, ty)
        dx = (wx[:, None, None] - tx).astype(np.float64)
        dy = (wy[:, None, None] - ty).astype(np.float64)
        if topol == HEXA:
            odd = (wy[:, None, None] - ty) % 2 != 0
            dx = np.where(odd, np.where(wy[:, None, None] % 2 == 0, dx - 0.5, dx + 0.5), dx)
            r = dx * dx + 0.75 * dy * dy                  # exact: multiples of 1/4 far below 2^24
        else:
            r = dx * dx + dy * dy
        dd = np.sqrt(r).astype(np.float32)                # (float)sqrt((double)r)
        member = (dd <= tr[:, None, None]) & (tx >= 0) & (tx < xd) & (ty >= 0) & (ty < yd)
        rows += int(member.sum())
        it, iy, ix = np.nonzero(member)
        gid = (ty[it, iy, ix] // 8) * (xd // 8) + tx[it, iy, ix] // 8
        pairs += np.unique(it * ((xd // 8) * (yd // 8)) + gid).size
    return rows, pairs


def run_exact(eng, E, oracle, xd, yd, d, topol, B, radius, x, ini, want_plan, fixed=None, mask=None, alpha=0.05):
    """one batch of B iterations (length B: the oracle's schedule) in exact mode: the plan, the oracle's bits, the counts"""
    use = int(fixed is not None)
    want, wi, _ = oracle.som_train(ini, xd, yd, topol, BUBBLE, x, B, alpha, radius, fixed_xy=fixed, mask=mask, fixed_on=use,
                                   batch=B)
    ds = E.Dataset(eng, x, fixed_xy=fixed, mask=mask)
    cb = E.Codebook(eng, ini, topol, BUBBLE, xd, yd)
    try:
        eng.set_update_mode("exact")
        plan = E.update_plan(cb, ds, B, alpha, radius, B, use_fixed=use, data_first=0)
        got_plan = {k: plan[k] for k in ("decode", "members_nt", "members_rr")}
        got_plan["reach"] = plan["reach_max"] >= 0
        assert got_plan == want_plan, plan
        s0 = eng.scan_stats()
        ti, _ = E.som_train(cb, ds, B, alpha, radius, use_fixed=use, batch=B, count=B, data_first=0)
        s1 = eng.scan_stats()
        got = cb.download()
    finally:
        cb.close()
        ds.close()
    assert np.array_equal(ti, wi)
    assert np.array_equal(bits(got), bits(want))
    # the statistics words against the count of the members
    row = np.arange(B) % x.shape[0]
    bx = np.where(wi >= 0, wi % xd, -1)
    by = np.where(wi >= 0, wi // xd, -1)
    if fixed is not None:
        fx = fixed[row].astype(np.int64)
        isf = wi == -3
        bx, by = np.where(isf, fx[:, 0], bx), np.where(isf, fx[:, 1], by)
    # a fixed point far outside reaches nothing: its window is not worth a count (no unit within radius + 2 rows)
    far = (bx > xd + 64) | (by > yd + 64)
    bx = np.where(far, -1, bx)
    rows, pairs = member_counts(xd, yd, topol, bx, by, radii(B, radius, B))
    assert s1["row_updates"] - s0["row_updates"] == rows
    assert s1["group_updates"] - s0["group_updates"] == pairs


DECODED_8 = dict(decode=True, members_nt=1024, members_rr=8, reach=True)


@pytest.fixture(scope="module")
def big_map_inputs():
    """256 x 128 map (512 row groups), dim 8: the data and the initial codebook of the 8192-iteration cases"""
    x, _ = synth(85, 8192 + 44, 8, k=9, spread=3.0)
    rs = np.random.RandomState(6)
    ini = (x[rs.randint(0, x.shape[0], 256 * 128)] + 0.3 * rs.standard_normal((256 * 128, 8))).astype(np.float32)
    return x, ini


@pytest.mark.parametrize("topol", [HEXA, RECT])
@pytest.mark.parametrize("radius", [20.0, 6.0, 1.5])
def test_runs_of_8192_on_512_groups_decode_their_winners(eng, E, oracle, big_map_inputs, topol, radius):
    x, ini = big_map_inputs
    run_exact(eng, E, oracle, 256, 128, 8, topol, 8192, radius, x, ini, DECODED_8)


def test_the_new_decode_range_ends_where_the_pinned_plans_begin(eng, E):
    ds = E.Dataset(eng, np.zeros((100, 16), dtype=np.float32))
    try:
        for xd, yd, B, decode in ((64, 512, 8192, True), (64, 512, 8191, False), (64, 504, 8192, False),
                                  (64, 512, 16383, True), (64, 504, 16384, True), (256, 256, 2048, False)):
            cb = E.Codebook(eng, np.zeros((xd * yd, 16), dtype=np.float32), HEXA, BUBBLE, xd, yd)
            try:
                assert E.update_plan(cb, ds, B, 0.05, 6.0, B, data_first=0)["decode"] == decode, (xd, yd, B)
            finally:
                cb.close()
    finally:
        ds.close()


@pytest.fixture(scope="module")
def small_map_inputs():
    """32 x 24 map, dim 8, 16384 iterations over 6000 rows (the run wraps); fixed points at a patch corner, on a patch
    edge, one unit outside the map, far outside it and beyond the exact branch's guard (y > 25000)"""
    x, _ = synth(86, 6000, 8, k=9, spread=3.0)
    rs = np.random.RandomState(12)
    fixed = np.full((6000, 2), -1, dtype=np.int16)
    spots = [(8, 8), (15, 16), (7, 23), (16, 3), (0, 11), (32, 5), (12, 24), (31, 24), (40, 30), (200, 300), (1030, 5),
             (5, 2000), (30000, 5), (32767, 32767), (3, 26000)]
    for k, r in enumerate(rs.choice(6000, 90, replace=False)):
        fixed[r] = spots[k % len(spots)]
    ini = (x[rs.randint(0, 6000, 32 * 24)] + 0.3 * rs.standard_normal((32 * 24, 8))).astype(np.float32)
    return x, ini, fixed


@pytest.mark.parametrize("topol", [HEXA, RECT])
@pytest.mark.parametrize("radius", [3.0, 8.0, 14.0])
def test_far_interior_and_boundary_winners_in_one_trip(eng, E, oracle, small_map_inputs, topol, radius):
    x, ini, fixed = small_map_inputs
    run_exact(eng, E, oracle, 32, 24, 8, topol, 16384, radius, x, ini, DECODED_8, fixed=fixed)


def test_skipped_samples_inside_a_trip(eng, E, oracle, small_map_inputs):
    x, ini, _ = small_map_inputs
    rs = np.random.RandomState(13)
    mask = (rs.random_sample(x.shape) < 0.1).astype(np.uint8)
    mask[rs.choice(6000, 400, replace=False)] = 1        # fully masked rows: skipped iterations (reach < 0)
    run_exact(eng, E, oracle, 32, 24, 8, HEXA, 16384, 8.0, x, ini, DECODED_8, mask=mask)


def test_gemm_tail_at_a_large_radius_against_the_float64_replay(eng, E, monkeypatch):
    """64 x 512 map, dim 128, 16384 iterations at alpha 0.3 and radius 64 (the plan of test_update_routes' gemm_long_nt256:
    trips of 1024 from the end of the batch until the tail holds enough FULL entries): most near winners are interior"""
    xd, yd, d, B = 64, 512, 128, 16384
    cs = dict(xd=xd, yd=yd, topol=HEXA, neigh=BUBBLE, radius=64.0, alpha=0.3, alpha_type=1, length=1000000, B=B, it0=0,
              first=0, use_fixed=0, use_weights=0)
    x, _, _, ini = GR.make_inputs(1200, B + 44, d, xd, yd)
    ds = E.Dataset(eng, x)
    try:
        exact, ti_e, ran_e, _ = GR._run(eng, E, ini, cs, ds, "exact", monkeypatch)
        gemm, ti_g, ran_g, plan = GR._run(eng, E, ini, cs, ds, "gemm", monkeypatch)
        full, ti_f, _, _ = GR._run(eng, E, ini, cs, ds, "gemm", monkeypatch, full=True)
    finally:
        ds.close()
    assert plan["apply"] == "gemm" and plan["tail"] and plan["tail_need"] > 0 and plan["decode"]
    assert (plan["members_nt"], plan["members_rr"]) == (256, 4)
    assert ran_e == 0 and ran_g > 0
    assert np.array_equal(ti_e, ti_g) and np.array_equal(ti_f, ti_g)
    assert np.array_equal(bits(full), bits(gemm))         # the tail is what the whole lists give
    counts = np.bincount(ti_e[ti_e >= 0], minlength=xd * yd)
    units = GR._busiest_subset(counts, xd, yd, None, 64.0, np.random.RandomState(3))
    kw = dict(xdim=xd, ydim=yd, topol=HEXA, neigh=BUBBLE, data=x, length=cs["length"], alpha=0.3, radius=64.0, winners=ti_e,
              start_iter=0, count=B, data_first=0)
    r64 = replay(ini, **kw, dtype=np.float64, units=units)
    assert np.array_equal(bits(exact[units]), bits(replay(ini, **kw, units=units).codes))
    scale = float(np.abs(exact).max())
    allow = GR.allowance(exact[units], r64.codes, r64.hits, scale)
    err = np.abs(gemm[units].astype(np.float64) - r64.codes)
    print("ALLOW_RATIO gemm_tail_radius64 %.3f (max hits %d)" % (float((err / allow).max()), int(r64.hits.max())))
    assert np.isfinite(gemm).all()
    assert (err <= allow).all()
