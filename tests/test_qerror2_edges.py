"""find_qerror2 on the GPU, per sample: k_qerror2 (kernels/qerror2_lininit.hpp) and its host driver somhip_qerror2
(host_scan.inc) against the oracle, one sample at a time.

The other qerror2 tests compare the float32 total over a data set.  The reference adds the per-sample sums into one
float accumulator, so an error of a few ulps in one sample's sum lies below the total's last place after the first
dozen samples.  Here somhip_qerror2 is called directly, as engine.qerror2_sum calls it, and for every sample of the run

  * out[i] equals, bit for bit, oracle.find_qerror2 of that one row (the oracle skips a row without a winner: 0);
  * ret[i] is 0 exactly for the rows whose components are all masked, and out[i] is 0 there;
  * engine.qerror2_sum equals, bit for bit, the float32 running sum of the oracle's per-sample values in run order
    (ret == 0 skipped) and, for a run over the whole set from row 0, the oracle's own total.

CASES drives the kernel and the driver at their own edges: the driver's chunk of 4096 samples (counts 4095, 4096, 4097
and 8193 of 4200 rows: the rows come round), first != 0 and runs that wrap inside and before a chunk, 255 / 256 / 257 /
512 / 513 units (the kernel takes 256 units at a time; the bubble's row window starts and ends chunks mid-way) with
radii at and on both sides of exact lattice distances (bubble_threshold and the row window together), dims from 1 to
1030 (the staging loop's second and fifth trips, mask bytes behind d floats at offsets that are no multiple of 16),
the gaussian form's far tail at radii 1.0 to 1.5 (the float of exp(y) subnormal and zero, subnormal products; how many
such (sample, unit) pairs a case holds is counted on the CPU from the oracle's winners before the GPU runs), and
gaussian radius 0, where the reference's -0.0 / 0.0 makes the winner's term and so the sample's sum NaN (isnan on both
sides; payloads are not compared).  That case is also where out[i] of a row with every component masked showed: its
key says distance 0 at unit 0, the kernel sums over it, and NaN * 0 is not the 0 the other radii give; the driver now
writes the 0 itself.

In a whole map the tail's terms are absorbed by the winner's neighbourhood within the sample's own sum.
test_gaussian_tail_alone makes them the sum: every unit whose rate is not tiny is a copy of the sample (distance 0,
term 0; the tie goes to unit 0, a corner), so out is the sum of the far units' subnormal products alone.
Needs an MI355X:  pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth
from helpers import som_replay

pytestmark = pytest.mark.gpu

HEXA, RECT, BUBBLE, GAUSS = 3, 4, 1, 2
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def around(v):
    """a radius equal to a lattice distance, and the floats just below and above it"""
    v = f32(v)
    return [float(np.nextafter(v, f32(0.0))), float(v), float(np.nextafter(v, f32(np.inf)))]


BUBBLE_RADII = {HEXA: [0.0, 1.0, 2.5, 100.0] + around(np.sqrt(3.0)) + around(np.sqrt(7.0)) + around(2.0),
                RECT: [0.0, 1.0, 2.5, 100.0] + around(np.sqrt(2.0)) + around(np.sqrt(5.0))}


class Case:
    def __init__(self, name, xd, yd, d, n, runs, topol=HEXA, bubble=(2.5,), gauss=(2.0,), masked=False, all_masked=(),
                 place="mixture", tail=False):
        self.name, self.xd, self.yd, self.d, self.n, self.runs, self.topol = name, xd, yd, d, n, runs, topol
        self.radii = [(BUBBLE, r) for r in bubble] + [(GAUSS, r) for r in gauss]
        self.masked, self.all_masked = masked, tuple(all_masked)
        self.place = place    # "mixture": rows of the seeded mixture; "units": rows next to units 0, n - 1, a middle one
                              # and random ones; "border": rows next to every unit of the map's border and a few more
        self.tail = tail      # count the far tail's (sample, unit) pairs and assert them (radius 1.0)

    def __repr__(self):
        return self.name


def _cases():
    cases = []
    # the driver's chunk of 4096 samples; one row masked whole in the first chunk and one right at index 4096
    cases.append(Case("chunk_4096", 7, 5, 6, 4200, [(0, 4095), (0, 4096), (0, 4097), (0, 8193), (0, 4200)], bubble=(1.5,),
                      gauss=(1.5,), masked=True, all_masked=(100, 4096)))
    # first != 0 and the wrap: inside a short run; inside the first chunk with the chunk edge behind it
    cases.append(Case("first_wrap_300", 7, 5, 6, 300, [(290, 25), (299, 2), (0, 300)], all_masked=(295, 3)))
    cases.append(Case("first_wrap_4200", 7, 5, 6, 4200, [(4000, 4300)], bubble=(1.5,), gauss=(1.5,), all_masked=(4199, 0, 3895)))
    # 255, 256, 257, 512 and 513 units
    for xd, yd in ((17, 15), (16, 16), (257, 1), (32, 16), (27, 19)):
        for topol, tn in ((HEXA, "hexa"), (RECT, "rect")):
            for masked in (False, True):
                cases.append(Case("units_%dx%d_%s%s" % (xd, yd, tn, "_masked" if masked else ""), xd, yd, 5, 40, [(0, 40)],
                                  topol=topol, bubble=BUBBLE_RADII[topol], gauss=(0.7, 2.0), masked=masked,
                                  all_masked=(7,) if masked else (), place="units"))
    # dims: the staging loop's trips of 256, the mask bytes behind d floats
    for d in (1, 3, 4, 255, 256, 257, 1030):
        for masked in (False, True):
            cases.append(Case("dim_%d%s" % (d, "_masked" if masked else ""), 13, 9, d, 100, [(0, 100)], masked=masked,
                              all_masked=(50,) if masked else ()))
    # the gaussian form's far tail
    cases.append(Case("gauss_tail_hexa", 16, 16, 8, 90, [(0, 90)], bubble=(), gauss=(1.0, 1.05, 1.5), place="border", tail=True))
    cases.append(Case("gauss_tail_rect", 20, 13, 8, 90, [(0, 90)], topol=RECT, bubble=(), gauss=(1.0, 1.05, 1.5), place="border",
                      tail=True))
    # gaussian radius 0: NaN for every sample with a winner
    cases.append(Case("gauss_radius_0", 13, 9, 5, 60, [(0, 60), (50, 20)], bubble=(), gauss=(0.0,), masked=True, all_masked=(11,)))
    return cases


CASES = _cases()


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


def make_inputs(c):
    """(codes, rows, mask or None) of case c"""
    rs = np.random.RandomState(sum(map(ord, c.name)))
    units = c.xd * c.yd
    if c.place == "mixture":
        x, _ = synth(rs.randint(1 << 30), c.n, c.d)
        codes = (x[rs.randint(0, c.n, units)] + 0.3 * rs.standard_normal((units, c.d))).astype(f32)
    else:
        codes = (2.0 * rs.standard_normal((units, c.d))).astype(f32)
        if c.place == "units":
            at = np.concatenate([[0, units - 1, units // 2 + c.xd // 2], rs.randint(0, units, c.n - 3)])
        else:
            ux, uy = np.arange(units) % c.xd, np.arange(units) // c.xd
            border = np.nonzero((ux == 0) | (ux == c.xd - 1) | (uy == 0) | (uy == c.yd - 1))[0]
            at = np.concatenate([border, rs.randint(0, units, c.n)])[:c.n]
            assert len(border) <= c.n
        x = (codes[at] + 0.01 * rs.standard_normal((c.n, c.d))).astype(f32)
    mask = None
    if c.masked or c.all_masked:
        mask = (rs.random_sample((c.n, c.d)) < 0.15).astype(np.uint8) if c.masked else np.zeros((c.n, c.d), np.uint8)
        for r in c.all_masked:
            mask[r] = 1
    return codes, x, mask


def qerror2(E, cb, ds, radius, first, count):
    """somhip_qerror2 as engine.qerror2_sum calls it: (out, ret), both prefilled so that an entry left out shows"""
    from som_lvq_pak_amd import _lib
    out = np.full(count, 7.0, dtype=np.float32)
    ret = np.full(count, -1, dtype=np.int32)
    E.check(cb.e.lib.somhip_qerror2(cb.h, ds.h, C.c_float(radius), first, count, out.ctypes.data_as(_lib.c_float_p),
                                    ret.ctypes.data_as(_lib.c_i32_p)))
    return out, ret


def per_sample(oracle, codes, c, neigh, radius, x, mask, rows):
    """the oracle's find_qerror2 of each of `rows` alone (0 for a row without a winner): float32 [n], NaN elsewhere"""
    want = np.full(x.shape[0], np.nan, dtype=np.float32)
    for r in rows:
        want[r] = oracle.find_qerror2(codes, c.xd, c.topol, neigh, x[r:r + 1], radius,
                                      mask=None if mask is None else mask[r:r + 1])
    return want


def running_sum(values, live):
    q = f32(0.0)
    for v, on in zip(values, live):
        if on:
            q = f32(q + v)
    return q


def same(a, b):
    """bit for bit, NaN = NaN whatever the payload"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float32)), np.atleast_1d(np.asarray(b, dtype=np.float32))
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def tail_counts(oracle, c, codes, x, radius):
    """(sample, unit) pairs with y <= -104, with -104 < y < -87, and units whose float h is a nonzero subnormal"""
    wi, _, _ = oracle.winners(codes, x)
    tx, ty = np.arange(c.xd * c.yd) % c.xd, np.arange(c.xd * c.yd) // c.xd
    zero = window = subnormal = 0
    for w in wi[:, 0]:
        dd = som_replay.lattice_dist(c.topol, int(w) % c.xd, int(w) // c.xd, tx, ty)
        y = (-(dd * dd)).astype(np.float64) / (2.0 * float(f32(radius)) * float(f32(radius)))
        zero += int((y <= -104.0).sum())
        window += int(((y > -104.0) & (y < -87.0)).sum())
        with np.errstate(under="ignore"):
            h = np.exp(y).astype(f32)
        subnormal += int(((h > 0) & (h < np.finfo(f32).tiny)).sum())
    return zero, window, subnormal


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_qerror2_per_sample(eng, E, oracle, c):
    codes, x, mask = make_inputs(c)
    dead = np.zeros(c.n, dtype=bool) if mask is None else mask.all(axis=1)
    assert set(np.nonzero(dead)[0]) >= set(c.all_masked)
    if c.tail:                                                   # conditions on the inputs, before the first GPU call
        counts = {r: tail_counts(oracle, c, codes, x, r) for _, r in c.radii}
        print(c.name, "(zero, window, subnormal h) per radius:", counts)
        assert counts[1.0][0] >= 100 and counts[1.0][1] >= 100 and counts[1.0][2] >= 1, counts
    used = sorted({int(r) for first, count in c.runs for r in (first + np.arange(min(count, c.n))) % c.n})
    ds = E.Dataset(eng, x, mask=mask)
    cbs = {neigh: E.Codebook(eng, codes, c.topol, neigh, c.xd, c.yd) for neigh in {n for n, _ in c.radii}}
    try:
        for neigh, radius in c.radii:
            want = per_sample(oracle, codes, c, neigh, radius, x, mask, used)
            assert np.all(want[dead & ~np.isnan(want)] == 0)
            if neigh == GAUSS and radius == 0.0:
                assert np.isnan(want[used][~dead[used]]).all()           # the reference's -0.0 / 0.0
            for first, count in c.runs:
                rows = (first + np.arange(count)) % c.n
                out, ret = qerror2(E, cbs[neigh], ds, radius, first, count)
                what = (neigh, radius, first, count)
                assert np.array_equal(ret, (~dead[rows]).astype(np.int32)), what
                assert np.all(bits(out[ret == 0]) == 0), what
                if neigh == GAUSS and radius == 0.0:
                    assert np.isnan(out[ret == 1]).all(), what
                bad = [i for i in range(count) if not same(out[i], want[rows[i]])]
                assert not bad, (what, bad[:5], out[bad[:5]], want[rows[bad[:5]]])
                total = E.qerror2_sum(cbs[neigh], ds, radius, first, count)
                assert same(total, running_sum(want[rows], ~dead[rows])), what
                if first == 0 and count == c.n:
                    whole = f32(oracle.find_qerror2(codes, c.xd, c.topol, neigh, x, radius, mask=mask))
                    assert same(total, whole), what
    finally:
        for cb in cbs.values():
            cb.close()
        ds.close()


@pytest.mark.parametrize("xd,yd,topol", [(16, 16, HEXA), (20, 13, RECT)], ids=["hexa16x16", "rect20x13"])
def test_gaussian_tail_alone(eng, E, oracle, xd, yd, topol):
    """every unit with y > -80 from the corner is a copy of the sample: the sample's sum is the tail's subnormal products"""
    rs = np.random.RandomState(xd)
    units, d = xd * yd, 8
    tx, ty = np.arange(units) % xd, np.arange(units) // xd
    dd = som_replay.lattice_dist(topol, 0, 0, tx, ty)
    base = (2.0 * rs.standard_normal((units, d))).astype(f32)
    v = base[0].copy()
    x = np.stack([v, v, v])
    mask = np.zeros((3, d), np.uint8)
    mask[1, ::3] = 1                                             # the same with components left out
    mask[2] = 1                                                  # and no winner at all
    ds = E.Dataset(eng, x, mask=mask)
    try:
        for radius in (1.0, 1.05, 1.25):
            y = (-(dd * dd)).astype(np.float64) / (2.0 * float(f32(radius)) ** 2)
            codes = base.copy()
            codes[y > -80.0] = v
            far = y <= -80.0
            assert ((y[far] > -104.0) & (y[far] < -87.0)).sum() >= 5 and (y <= -104.0).sum() >= 5, radius
            want = np.array([oracle.find_qerror2(codes, xd, topol, GAUSS, x[r:r + 1], radius, mask=mask[r:r + 1])
                             for r in range(3)], dtype=f32)
            # the inputs do what they are for: nonzero sums far below the smallest normal float's neighbourhood
            assert 0 < want[0] < 1e-30 and 0 < want[1] < 1e-30 and want[2] == 0, (radius, want)
            cb = E.Codebook(eng, codes, topol, GAUSS, xd, yd)
            out, ret = qerror2(E, cb, ds, radius, 0, 3)
            cb.close()
            assert np.array_equal(ret, [1, 1, 0]), radius
            assert np.array_equal(bits(out), bits(want)), (radius, out, want)
    finally:
        ds.close()
