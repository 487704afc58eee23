"""What the preparation of a nearest-row search leaves on the device (somhip_debug_prepared), against numpy:

  * the bf16 pieces of the codebook (chi / clo), of the samples (xhi, and xlo where a kernel reads it) and their
    sample-major copy (xrow): hi = the value rounded to nearest even, lo = the bf16 of the exact remainder;
  * the row-major fp32 copy of the rows that k_prep_codes_bf16 stages through LDS: the rows themselves, zero padding rows;
  * the squared row norms, bit for bit, in the documented order: the workgroup's waves (16 from 16 k-blocks on, 4 from 4
    on, else 1) take the k-blocks round-robin, a wave adds the eight squares of a k-block in order, and the waves'
    partial sums are added in wave order; 3.0e38 for padding rows;
  * the windows tau and tau1 that k_pack_samples_bf16 forms from the rows it packs: the float64 formula of
    kernels/prefilter_mfma.hpp (sample_windows) rounded UP to fp32.  The kernel sums ||x||^2 in double in its own order, so
    its value before that rounding is held to 1e-9 relative of numpy's, and the fp32 result may never lie below it.

Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (rows, d, samples): what each shape is there for
SHAPES = [
    (4096, 64, 8192),       # the smallest shape that gets the row-major copy; four waves, two rounds through LDS
    (4096, 36, 8192),       # odd d4: the one-level route with the copy, a round with one wave and half a k-block
    (4096, 288, 8192),      # sixteen waves, three rounds (both LDS buffers reused), the last with four waves
    (4096, 24, 8192),       # one wave, three rounds of one k-block each
    (64, 32, 256),          # no copy
    (1024, 544, 256),       # level 2 reads its samples from global memory: xlo must still be written
    (65, 32, 256),          # padding rows' norms
    (1024, 32, 225),        # ragged last sample tile: zero padding samples
    (4096, 64, 8193),       # ... behind full ones, with the copy
]


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    e.set_scan_mode("mfma_bf16")
    yield e
    e.close()


def bf16_rn(v):
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def split_bf16(v):
    hi = bf16_rn(v)
    rem = v - (hi.astype(np.uint32) << np.uint32(16)).view(np.float32)      # exact
    return hi, bf16_rn(rem)


def tiles(m, rows_per, d8):
    """[n, d] fp32 -> the (hi, lo) tiles [n / rows_per][d8][rows_per][8], zero rows and dims appended"""
    n, d = m.shape
    npad = (n + rows_per - 1) // rows_per * rows_per
    full = np.zeros((npad, d8 * 8), dtype=np.float32)
    full[:n, :d] = m
    t = full.reshape(npad // rows_per, rows_per, d8, 8).transpose(0, 2, 1, 3)
    return split_bf16(np.ascontiguousarray(t))


def row_norms(codes, d8):
    """fp32 replay of k_prep_codes_bf16's sum"""
    n, d = codes.shape
    nw = 16 if d8 >= 16 else 4 if d8 >= 4 else 1
    full = np.zeros((n, d8 * 8), dtype=np.float32)
    full[:, :d] = codes
    part = np.zeros((nw, n), dtype=np.float32)
    for kb in range(d8):
        for j in range(8):
            v = full[:, kb * 8 + j]
            part[kb % nw] = part[kb % nw] + v * v
    acc = part[0].copy()
    for w in range(1, nw):
        acc = acc + part[w]
    return acc


def err_coefficients(d):
    """prefilter_err3 (bf16) and prefilter_err_l1 (host_scan.inc)"""
    k = (d + 2) * U
    gam = k / (1.0 - k)
    k3 = 3.0 * (d + 2) * U
    prod = 4.04 * (k3 / (1.0 - k3)) + 3.1 / 65536.0 + 2.0 * U
    sq = 2.0 * gam + 2.0 * U
    l1_prod = 2.0 * ((1.0 / 256.0) * (1.0 + 1.0 / 256.0) + 2.02 * gam)
    l1_sq = 2.0 * gam + U
    return prod, sq, l1_prod, l1_sq


def up32(t):
    f = t.astype(np.float32)
    low = f.astype(np.float64) < t
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def check_window(got, want64, what):
    """got (fp32) is want64 rounded up, want64 known to 1e-9 relative"""
    assert (got.astype(np.float64) >= want64).all(), "%s below the formula at %s" % (what, np.flatnonzero(got.astype(np.float64) < want64)[:8])
    assert (got <= up32(want64 * (1.0 + 1e-9))).all(), "%s above the formula at %s" % (what, np.flatnonzero(got > up32(want64 * (1.0 + 1e-9)))[:8])


@pytest.mark.parametrize("n,d,count", SHAPES)
def test_prepared_copies(eng, n, d, count):
    from som_lvq_pak_amd import engine as E
    rs = np.random.RandomState(n + 3 * d + count)
    codes = rs.standard_normal((n, d)).astype(np.float32)
    x = (rs.standard_normal((count, d)) + 0.5).astype(np.float32)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    try:
        plan = E.scan_plan(cb, ds, count, 1)
        out = E.debug_prepared(cb, ds, 0, count)
    finally:
        cb.close()
        ds.close()
    d8, ng = (d + 7) // 8, (n + 63) // 64
    two = plan["route"] == "two_level"
    assert two == (d not in (24, 36)) and plan["l2_global"] == (d == 544)
    # the codebook's pieces, copy and norms
    chi, clo = tiles(codes, 64, d8)
    assert np.array_equal(out["chi"], chi) and np.array_equal(out["clo"], clo)
    assert (out["rowmajor"] is not None) == (count >= 8192)
    if out["rowmajor"] is not None:
        want = np.zeros((ng * 64, d), dtype=np.float32)
        want[:n] = codes
        assert np.array_equal(out["rowmajor"].view(np.uint32), want.view(np.uint32)), \
            ("row-major copy differs in rows", np.unique(np.nonzero(out["rowmajor"].view(np.uint32) != want.view(np.uint32))[0])[:8])
    cn = np.full(ng * 64, np.float32(3.0e38), dtype=np.float32)
    cn[:n] = row_norms(codes, d8)
    assert np.array_equal(out["cn"].view(np.uint32), cn.view(np.uint32)), ("norms differ in rows", np.flatnonzero(out["cn"] != cn)[:8])
    # the samples' pieces
    xhi, xlo = tiles(x, 32, d8)
    assert np.array_equal(out["xhi"], xhi)
    assert (out["xlo"] is not None) == (not two or plan["l2_global"])
    if out["xlo"] is not None:
        assert np.array_equal(out["xlo"], xlo)
    assert (out["xrow"] is not None) == two
    if two:
        bp = xhi.shape[0] * 32
        rows = np.stack([xhi.transpose(0, 2, 1, 3).reshape(bp, d8, 8), xlo.transpose(0, 2, 1, 3).reshape(bp, d8, 8)], axis=2)
        assert np.array_equal(out["xrow"], rows)
    # the windows
    prod, sq, l1_prod, l1_sq = err_coefficients(d)
    cmax = np.sqrt(np.float64(cn[:n].max()) * (1.0 + 4.0 * d * U))
    a = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    s = a + cmax
    check_window(out["tau"], 2.0 * (prod * a * cmax + sq * s * s) * 1.001, "tau")
    if two:
        d1 = (l1_prod * a * cmax + l1_sq * s * s) * 1.001
        d3 = 0.5 * out["tau"].astype(np.float64)
        check_window(out["tau1"], d1 + np.maximum(d1, 3.0 * d3), "tau1")
    else:
        assert out["tau1"] is None


def test_windows_follow_the_codebook(eng):
    """two searches in turn use the two words of the largest norm in turn: the second, against a codebook of smaller
    norm, must not see the first one's maximum"""
    from som_lvq_pak_amd import engine as E
    rs = np.random.RandomState(11)
    x = rs.standard_normal((256, 32)).astype(np.float32)
    codes = rs.standard_normal((1024, 32)).astype(np.float32)
    ds, cb = E.Dataset(eng, x), E.Codebook(eng, codes)
    try:
        taus = []
        for scale in (8.0, 1.0, 8.0, 1.0, 1.0):
            cb.upload((scale * codes).astype(np.float32))
            taus.append(E.debug_prepared(cb, ds, 0, 256)["tau"])
    finally:
        cb.close()
        ds.close()
    assert np.array_equal(taus[0], taus[2]) and np.array_equal(taus[1], taus[3]) and np.array_equal(taus[3], taus[4])
    assert (taus[1] < taus[0]).all()
