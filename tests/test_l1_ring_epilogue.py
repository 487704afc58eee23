"""Level 1 of the two-level pre-filter by its two kernels (somhip_debug_level1): the persistent ring kernel
(kernels/prefilter_l1_ring.hpp), whose tile epilogue folds the row quarters in registers and multiplies a tile's first
stage onto the constant 0, against the wide-tile kernel k_dist_mfma_bf16_l1w16 followed by k_group_min.  Both form the
same fma(-2, acc, cn) per (row, sample) from the same MFMA sums, and a minimum does not depend on its order: the group
minima and the per-sample minima must be EQUAL, not close."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


def level1(eng, cb, ds, rows, count, ring):
    from som_lvq_pak_amd import engine as E
    ng, bp = (rows + 63) // 64, (count + 31) // 32 * 32
    wmin = np.full((ng, bp), np.nan, dtype=np.float32)
    gmin1 = np.zeros(bp, dtype=np.uint32)
    bpad = C.c_int64(0)
    E.check(eng.lib.somhip_debug_level1(cb.h, ds.h, 0, count, ring, wmin.ctypes.data_as(C.POINTER(C.c_float)),
                                        gmin1.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bpad)))
    assert bpad.value == bp
    return wmin, gmin1


def ordered_to_float(u):
    """the inverse of the kernels' order-preserving image of a float (kernels/rerank.hpp)"""
    u = u.astype(np.uint32)
    return np.where(u & 0x80000000, u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(np.float32)


# (rows, samples, d): what each shape is there for
SHAPES = [
    (4096 + 37, 3841, 64),      # two stages: the zero-C stage is followed at once by the tile's last; 65 groups -> the last
                                # tile has one live group of four, with padding rows; the last sample column is partial
    (4096 + 37, 3841, 128),     # one pair of stages behind the peeled pair
    (4096 + 37, 3841, 192),     # three pairs of stages
    (32768 + 64, 1100, 64),     # 645 tiles: every workgroup takes two or three and changes sample column between them
    (256, 256, 64),             # one tile: most workgroups have nothing to do
]


def make_case(n, b, d, ties):
    rs = np.random.RandomState(n + 7 * b + d + (1000 if ties else 0))
    if ties:                    # every row and every sample many times over: the minima tie within and across groups
        codes = rs.standard_normal((97, d)).astype(np.float32)[rs.randint(0, 97, size=n)]
        x = rs.standard_normal((53, d)).astype(np.float32)[rs.randint(0, 53, size=b)]
    else:
        codes = rs.standard_normal((n, d)).astype(np.float32)
        x = rs.standard_normal((b, d)).astype(np.float32)
    return codes, x


@pytest.mark.parametrize("n,b,d,ties", [s + (False,) for s in SHAPES] + [(4096 + 37, 3841, 128, True)])
def test_ring_kernel_gives_the_wide_kernels_minima(eng, n, b, d, ties):
    from som_lvq_pak_amd import engine as E
    codes, x = make_case(n, b, d, ties)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    try:
        w_ring, g_ring = level1(eng, cb, ds, n, b, 1)
        w_wide, g_wide = level1(eng, cb, ds, n, b, 0)
    finally:
        cb.close()
        ds.close()
    assert not np.isnan(w_wide).any() and not np.isnan(w_ring).any()      # every (group, sample) was written
    assert np.array_equal(w_ring, w_wide), ("group minima differ at", np.argwhere(w_ring != w_wide)[:8])
    assert np.array_equal(g_ring, g_wide), ("per-sample minima differ at", np.flatnonzero(g_ring != g_wide)[:8])
    assert np.array_equal(ordered_to_float(g_ring), w_ring.min(axis=0))
    if not ties:                                # and they are the numbers they should be (whole groups, the first samples)
        k, full = min(b, 64), n // 64
        want = ((codes.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * codes.astype(np.float64) @ x[:k].astype(np.float64).T)
        want = np.stack([want[g * 64:(g + 1) * 64].min(axis=0) for g in range(full)])
        # bf16 operands: |<c,x> - <c_hi,x_hi>| <= 2^-8 (1 + 2^-8) ||c|| ||x||, twice that in s~
        tol = 2.0 * 2.0 ** -8 * 1.01 * np.sqrt((codes.astype(np.float64) ** 2).sum(1)).max() * np.sqrt((x[:k].astype(np.float64) ** 2).sum(1))
        assert (np.abs(w_ring[:full, :k] - want) <= tol[None, :] + 1e-3).all()


def test_level1_diagnostic_refuses_shapes_neither_kernel_takes(eng):
    from som_lvq_pak_amd import _lib, engine as E
    rs = np.random.RandomState(3)
    for n, b, d in ((256, 256, 32), (256, 224, 64)):       # half a pair of stages; fewer than eight sample tiles
        cb, ds = E.Codebook(eng, rs.standard_normal((n, d)).astype(np.float32)), E.Dataset(eng, rs.standard_normal((b, d)).astype(np.float32))
        with pytest.raises(_lib.SomhipError, match="neither level-1 kernel"):
            level1(eng, cb, ds, n, b, 1)
        cb.close()
        ds.close()
