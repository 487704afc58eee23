"""planes past its first chunk block: several chunk blocks per row group, slabs of several row groups, windows off a
multiple of 4, patch order at several chunk blocks, and columns with NaN and infinities.

The reference is tests/planes_replay.py (pinned against the recorded reference runs by tests/test_planes.py); grey, lo
and hi are compared by bit pattern.  Every shape is chosen against a constant of the kernels, read from the source by
test_the_launch_rules_are_what_the_shapes_assume so that the shapes have to follow a change:

    wave per chunk      a wave takes one chunk of 4 components, a workgroup 4 chunks (kernels/planes.hpp)
    chunk_blocks        (nq + 3) / 4 workgroups cover the nq chunks of a window (host_planes.inc): 1 up to 16 components
    n_slabs             min(ngroups, n_cus * 8 / chunk_blocks), n_cus = 256 until a scan has set it: a slab walks the row
                        groups slab, slab + n_slabs, ...

    130 x 17      chunk_blocks 2: the second workgroup has one live wave, whose chunk holds one component and three pads
    130 x 40      windows (5, 30), (17, 4), (39, 1): q0 > 0, first off a multiple of 4, dead waves before and after the
                  window inside a live workgroup
    4485 x 1024   71 row groups, chunk_blocks 64, 32 slabs: seven of three row groups, 25 of two; window (5, 70) has
                  chunk_blocks 5 and one row group per slab
    8256 x 260    129 row groups, chunk_blocks 17, 120 slabs: nine of two row groups, 111 of one
    24 x 16 x 40, 32 x 32 x 20   maps kept as 8x8 patches, chunk_blocks 3 and 2: storage order is not unit order

In the two large shapes a block of planted components holds an extreme twice, in rows chosen by row group (see
PLANTED): the first holder in row order decides the bits of lo / hi, whichever slab, trip or storage row it lies in."""
import functools
import os
import re

import numpy as np
import pytest

import planes_replay as R
import test_planes as TP
from test_planes import assert_same_bits, bits, case_rows, eng  # noqa: F401  (eng: the module's engine fixture)

CSRC = os.path.join(TP.ROOT, "som_lvq_pak_amd", "csrc")
DEFAULT_CUS = 256                    # host_planes.inc while the engine has not counted the device's


def chunk_blocks(first, count):
    q0 = first >> 2
    return ((((first + count - 1) >> 2) - q0 + 1) + 3) // 4


def slabs(ngroups, cblocks, n_cus=DEFAULT_CUS):
    """(n_slabs, row groups of every slab)"""
    n_slabs = min(ngroups, max(1, n_cus * 8 // cblocks))
    return n_slabs, [len(range(s, ngroups, n_slabs)) for s in range(n_slabs)]


# ------------------------------------------------------------------ the planted components
PLANTED = ["lo_zero_pm", "lo_zero_mp", "hi_zero_pm", "hi_zero_mp", "max_twice"]
PLANT_AT = 8                                                     # first planted component: inside window (5, 70)


def plant(rows, at, a, b):
    """five components from `at` on that hold their extreme in rows a < b only:
    lo_zero_pm / lo_zero_mp   values from 1 up, +0.0 in a and -0.0 in b / the other way round: lo has a's sign
    hi_zero_pm / hi_zero_mp   values from -1 down, the same two zeros: hi has a's sign
    max_twice                 values below 1e6, 3e7 in a and in b"""
    assert a < b
    rs = np.random.RandomState(a + 7 * b)
    n = rows.shape[0]
    for k, kind in enumerate(PLANTED):
        col = (1.0 + np.abs(rs.standard_normal(n) * 1000.0)).astype(np.float32)
        if kind.startswith("hi_zero"):
            col = -col
        if kind == "max_twice":
            col[a] = col[b] = 3e7
        else:
            col[a], col[b] = (0.0, -0.0) if kind.endswith("pm") else (-0.0, 0.0)
        rows[:, at + k] = col
    return at + len(PLANTED)


def large_case(n, d):
    """case_rows with three planted blocks.  Row pairs by row group (lane 17 and lane 40), n_slabs for the whole range:
    group 5, group n_slabs + 3       the first holder lies in the first trip of slab 5, the second in the second trip of
                                     slab 3: the slab that k_planes_bounds reads first holds the later row
    group 3, group n_slabs + 3       both in slab 3: decided inside one wave's walk
    group n_slabs + 3, last group    second trip of slab 3 against the last slab of the walk"""
    rows = case_rows(n, d, 0)
    ngroups = (n + 63) // 64
    n_slabs, _ = slabs(ngroups, chunk_blocks(0, d))
    last = min(n - 1, 64 * (ngroups - 1) + 40)
    pairs = [(64 * 5 + 17, 64 * (n_slabs + 3) + 40), (64 * 3 + 17, 64 * (n_slabs + 3) + 40), (64 * (n_slabs + 3) + 17, last)]
    at = PLANT_AT
    for a, b in pairs:
        at = plant(rows, at, a, b)
    return rows, pairs


@functools.lru_cache(maxsize=None)
def large(n, d):
    """(rows, pairs, the replay's planes): made once per session and never written to"""
    rows, pairs = large_case(n, d)
    want = R.planes(rows)
    for arr in (rows,) + want:
        arr.setflags(write=False)
    return rows, pairs, want


def check_planted(rows, want, pairs, at=PLANT_AT):
    """the planted components decide something: the two sign placements give other lo / hi bits, the zero is the
    extreme, and the doubled maximum is the maximum"""
    _, lo, hi = want
    for a, b in pairs:
        for c, v in ((at, lo), (at + 2, hi)):
            assert (bits(v)[c], bits(v)[c + 1]) == (0, 0x80000000), (a, b, c)
            assert bits(rows[a, c]) == 0 and bits(rows[b, c]) == 0x80000000 and bits(rows[a, c + 1]) == 0x80000000
        assert hi[at + 4] == np.float32(3e7) and (rows[:, at + 4] == hi[at + 4]).sum() == 2
        at += len(PLANTED)


# ------------------------------------------------------------------ without a GPU
def test_the_launch_rules_are_what_the_shapes_assume():
    """chunk_blocks, the slab count and the wave-per-chunk rule are not exposed: read from the source"""
    host = open(os.path.join(CSRC, "host_planes.inc")).read()
    assert re.search(r"const int q0 = first_plane >> 2, nq = \(\(first_plane \+ n_planes - 1\) >> 2\) - q0 \+ 1;", host)
    assert re.search(r"const int chunk_blocks = \(nq \+ 3\) / 4;", host)
    m = re.search(r"\(e->n_cus > 0 \? e->n_cus : (\d+)\) \* 8 / chunk_blocks\)", host)
    assert m and int(m.group(1)) == DEFAULT_CUS
    assert re.search(r"n_slabs = \(int\)std::min<int64_t>\(cb->v\.ngroups, want\);", host)
    setters = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".inc", ".hip")) and
               re.search(r"e->n_cus = ", open(os.path.join(CSRC, f)).read())]
    assert setters == ["host_scan.inc"]                                      # only a scan counts the device's units
    kern = open(os.path.join(CSRC, "kernels", "planes.hpp")).read()
    rule = r"\(first >> 2\) \+ static_cast<int>\(blockIdx\.x % static_cast<unsigned>\(chunk_blocks\)\) \* 4 \+ \(threadIdx\.x >> 6\)"
    assert len(re.findall(rule, kern)) == 2                                  # k_planes_minmax and k_planes_grey
    assert re.search(r"for \(int64_t g = slab; g < cb\.ngroups; g \+= n_slabs\)", kern)


def test_the_shapes_reach_what_they_name():
    assert chunk_blocks(0, 9) == 1 and chunk_blocks(0, 16) == 1              # what tests/test_planes.py reaches
    assert chunk_blocks(0, 17) == 2
    assert [chunk_blocks(*w) for w in ((0, 40), (5, 30), (17, 4), (39, 1))] == [3, 2, 1, 1]
    n_slabs, sizes = slabs(71, chunk_blocks(0, 1024))
    assert chunk_blocks(0, 1024) == 64 and n_slabs == 32 and sizes.count(3) == 7 and sizes.count(2) == 25
    assert chunk_blocks(5, 70) == 5 and slabs(71, 5) == (71, [1] * 71)
    n_slabs, sizes = slabs(129, chunk_blocks(0, 260))
    assert chunk_blocks(0, 260) == 17 and n_slabs == 120 and sizes.count(2) == 9 and sizes.count(1) == 111
    assert chunk_blocks(0, 40) == 3 and chunk_blocks(0, 20) == 2 and chunk_blocks(5, 30) == 2 and chunk_blocks(5, 15) == 1


@pytest.mark.parametrize("n,d", [(4485, 1024), (8256, 260)])
def test_the_planted_components_decide(n, d):
    rows, pairs, want = large(n, d)
    assert PLANT_AT + 3 * len(PLANTED) <= min(d, 5 + 70)
    check_planted(rows, want, pairs)
    n_slabs, _ = slabs((n + 63) // 64, chunk_blocks(0, d))
    (a0, b0), (a1, b1), (a2, b2) = [(a // 64, b // 64) for a, b in pairs]
    assert a0 % n_slabs > b0 % n_slabs and a0 < n_slabs <= b0                # the later row lies in the earlier slab
    assert a1 % n_slabs == b1 % n_slabs and a1 < n_slabs <= b1               # one slab, two trips
    assert a2 >= n_slabs and b2 == (n + 63) // 64 - 1


@pytest.mark.parametrize("shape", TP.SHAPES, ids=["%dx%d" % s[:2] for s in TP.SHAPES])
def test_bounds_any_equals_bounds_on_finite_columns(shape):
    rows = case_rows(*shape)
    for c in range(rows.shape[1]):
        for got, want in zip(R.bounds_any(rows[:, c]), R.bounds(rows[:, c])):
            assert bits(got) == bits(want), c


NONFINITE = ["nan_among_finite", "nan_in_row_0", "both_inf_among_finite", "pinf_among_finite", "only_nan", "only_pinf",
             "pinf_and_nan", "only_ninf", "finite"]


def nonfinite_rows(n=130):
    """one column per name, 130 rows: three row groups, the last one partly padding"""
    rs = np.random.RandomState(130)
    rows = (rs.standard_normal((n, len(NONFINITE))) * 50.0).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    col = {name: c for c, name in enumerate(NONFINITE)}
    rows[[3, 64, 77, 129], col["nan_among_finite"]] = nan
    rows[[0, 65], col["nan_in_row_0"]] = nan
    rows[[5, 100], col["both_inf_among_finite"]] = inf
    rows[[6, 128], col["both_inf_among_finite"]] = -inf
    rows[[5, 100], col["pinf_among_finite"]] = inf
    rows[:, col["only_nan"]] = nan
    rows[:, col["only_pinf"]] = inf
    rows[:, col["pinf_and_nan"]] = np.where(np.arange(n) % 3 == 0, nan, inf)
    rows[:, col["only_ninf"]] = -inf
    return rows


def test_bounds_any_on_nonfinite_columns():
    """the reference's loop, one row after the other, gives what the vectorised rule gives"""
    rows = nonfinite_rows()
    fmax = np.float32(R.FLT_MAX)
    for c, name in enumerate(NONFINITE):
        minval, maxval = fmax, -fmax
        for p in rows[:, c]:
            if maxval < p:
                maxval = p
            if minval > p:
                minval = p
        lo, hi = R.bounds_any(rows[:, c])
        assert (bits(lo), bits(hi)) == (bits(minval), bits(maxval)), name
    _, lo, hi = R.planes(rows, bounds_of=R.bounds_any)
    got = {name: (float(lo[c]), float(hi[c])) for c, name in enumerate(NONFINITE)}
    inf, fmax = np.inf, float(fmax)
    for name in ("nan_among_finite", "nan_in_row_0", "finite"):
        assert np.isfinite(got[name]).all() and got[name][0] < got[name][1]
    assert got["both_inf_among_finite"] == (-inf, inf)
    assert np.isfinite(got["pinf_among_finite"][0]) and got["pinf_among_finite"][1] == inf
    assert got["only_nan"] == (fmax, -fmax) and got["only_pinf"] == (fmax, inf) == got["pinf_and_nan"]
    assert got["only_ninf"] == (-inf, -fmax)


# ------------------------------------------------------------------ on the GPU
def check_windows(E, cb, want, d, windows, what):
    for first, count in windows:
        cnt = d - first if count is None else count
        got = E.planes(cb, first, count)
        for name, g, w in zip(("grey", "lo", "hi"), got, want):
            assert_same_bits(g, w[first:first + cnt], (what, first, count, name))


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,windows", [(130, 17, [(0, None)]), (130, 40, [(0, None), (5, 30), (17, 4), (39, 1)])],
                         ids=["130x17", "130x40"])
def test_several_chunk_blocks_and_windows(n, d, windows, eng):
    from som_lvq_pak_amd import engine as E
    rows = case_rows(n, d, 0)
    cb = E.Codebook(eng, rows)
    check_windows(E, cb, R.planes(rows), d, windows, "%dx%d" % (n, d))
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,windows", [(4485, 1024, [(0, None), (5, 70)]), (8256, 260, [(0, None)])],
                         ids=["4485x1024", "8256x260"])
def test_slabs_of_several_row_groups(n, d, windows):
    """the slab walk makes a second and a third trip; the planted extremes are decided between trips of one slab and
    between slabs whose order is not row order.  On an engine of its own that has run no scan, so its count of compute
    units is still unset and the slabs are those of DEFAULT_CUS whatever the device (which is also the MI355X's count;
    torch cannot be asked here, it finds no device once the engine's HIP runtime is loaded)."""
    from som_lvq_pak_amd import engine as E
    rows, pairs, want = large(n, d)
    ngroups = (n + 63) // 64
    assert ngroups > DEFAULT_CUS * 8 // chunk_blocks(0, d)                   # some slab holds several row groups
    own = E.Engine(0)
    cb = E.Codebook(own, rows)
    check_windows(E, cb, want, d, windows, "%dx%d" % (n, d))
    cb.close()
    own.close()


@pytest.mark.gpu
@pytest.mark.parametrize("xdim,ydim,d", [(24, 16, 40), (32, 32, 20)], ids=["24x16x40", "32x32x20"])
def test_patch_order_at_several_chunk_blocks(xdim, ydim, d, eng):
    """a planted pair whose first row in unit order is stored after the second one: unit 20 lies in patch 2, unit
    xdim + 3 in patch 0"""
    from som_lvq_pak_amd import engine as E
    assert xdim % 8 == 0 and ydim % 8 == 0                                   # codebook_create's condition for patches
    rows = case_rows(xdim * ydim, d, 0)
    pair = (20, xdim + 3)
    plant(rows, PLANT_AT, *pair)
    want = R.planes(rows)
    check_planted(rows, want, [pair])
    windows = [(0, None), (5, min(30, d - 5))]
    cb = E.Codebook(eng, rows, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
    flat = E.Codebook(eng, rows)
    check_windows(E, cb, want, d, windows, "map")
    for first, count in windows:
        for name, g, f in zip(("grey", "lo", "hi"), E.planes(cb, first, count), E.planes(flat, first, count)):
            assert_same_bits(g, f, ("map against rows", first, name))
    cb.close()
    flat.close()


@pytest.mark.gpu
def test_nonfinite_components_follow_the_reference(eng):
    """NaN wins no comparison, +inf is never the minimum of a column of its own and -inf never the maximum: lo and hi by
    bits; grey by bits where it is a number, and NaN where the replay has NaN (the sign of a generated NaN is the
    machine's)"""
    from som_lvq_pak_amd import engine as E
    rows = nonfinite_rows()
    g_want, lo_want, hi_want = R.planes(rows, bounds_of=R.bounds_any)
    cb = E.Codebook(eng, rows)
    grey, lo, hi = E.planes(cb)
    cb.close()
    for c, name in enumerate(NONFINITE):
        print("%-22s lo %-14r hi %-14r (reference lo %r hi %r)" % (name, lo[c], hi[c], lo_want[c], hi_want[c]))
    assert_same_bits(lo, lo_want, "lo")
    assert_same_bits(hi, hi_want, "hi")
    number = ~np.isnan(g_want)
    some = {name: number[c].sum() for c, name in enumerate(NONFINITE)}
    assert some["nan_among_finite"] == 126 and some["nan_in_row_0"] == 128 and some["pinf_among_finite"] == 128
    assert some["finite"] == 130 and sum(some.values()) == 126 + 128 + 128 + 130
    assert np.array_equal(np.isnan(grey), ~number)
    assert_same_bits(grey[number], g_want[number], "grey")
