"""The data passes behind lininit and randinit at their kernels' tile edges: k_column_sums and k_centered_products
against the in-order fp32 replay of tests/lininit_replay.py (itself pinned to the real reference's find_eigenvectors by
tests/test_lininit_replay.py), bit pattern for bit pattern, and k_column_minmax against numpy on the host rows.

The shapes are the smallest at which each branch of the kernels first exists (lininit_replay.SHAPES); the inputs are
such that a re-associated, a fused or a more accurate sum changes more than half of the elements
(test_lininit_replay.py::test_inputs_tell_an_in_order_chain_from_a_better_sum)."""
import numpy as np
import pytest

import lininit_replay as R

pytestmark = pytest.mark.gpu

CASES = [(d, n, m) for d, n in R.SHAPES for m in (False, True)]
IDS = ["%dx%d%s" % (d, n, "_masked" if m else "") for d, n, m in CASES]
FLT_MAX = np.float32(3.402823466e+38)


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


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(R.bits(a), R.bits(b))


def special(dim, rows, masked):
    return masked and (dim, rows) == (33, 130)


# ------------------------------------------------------------------ k_column_sums
@pytest.mark.parametrize("dim,rows,masked", CASES, ids=IDS)
def test_column_sums_equal_the_replay(eng, E, dim, rows, masked):
    """sum bits and counts, on the generator rows and on the scaled rows (the ones whose sums discriminate); a fully
    masked column gives count 0 and sum +0; NaN and 1e30 at masked positions reach nothing; inside the float64 bound"""
    c = R.replayed(dim, rows, masked)
    for x, want, want_cnt in ((c["xs"], c["ss"], c["scnt"]), (c["x"], c["s"], c["cnt"])):
        ds = E.Dataset(eng, x, mask=c["mask"])
        got, cnt = E.column_sums(ds)
        ds.close()
        assert cnt.dtype == np.int64 and np.array_equal(cnt, want_cnt)
        assert same_bits(got, want)
        s64, bound = R.column_sums64(x, c["mask"])
        assert (np.abs(got.astype(np.float64) - s64) <= bound).all()
        if special(dim, rows, masked):
            assert cnt[R.FULL_COL] == 0 and R.bits(got)[R.FULL_COL] == 0
            assert np.isfinite(got).all() and (np.abs(got) < 1e9).all()
    if not masked:
        assert (cnt == rows).all()


# ------------------------------------------------------------------ k_centered_products
@pytest.mark.parametrize("dim,rows,masked", CASES, ids=IDS)
def test_centered_products_equal_the_replay(eng, E, dim, rows, masked):
    """with the replay's mean: the upper triangle has the replay's bits and the strict lower triangle is all zero
    bits; then the zero vector as mean on the same data set (nothing is cached), then the first mean again (nothing
    is left over in scratch from the call before, whatever shape the case before this one had)"""
    c = R.replayed(dim, rows, masked)
    ds = E.Dataset(eng, c["x"], mask=c["mask"])
    zero = np.zeros(dim, dtype=np.float32)
    iu, il = np.triu_indices(dim), np.tril_indices(dim, -1)
    for mean, want in ((c["mean"], c["R"]), (zero, c["R0"]), (c["mean"], c["R"])):
        got = E.centered_products(ds, mean)
        assert got.shape == (dim, dim) and got.dtype == np.float32
        assert (R.bits(got)[il] == 0).all()
        assert np.array_equal(R.bits(got)[iu], R.bits(want)[iu])
        r64, bound = R.centered_products64(c["x"], c["mask"], mean)
        assert (np.abs(got.astype(np.float64) - r64)[iu] <= bound[iu]).all()
        if special(dim, rows, masked):
            assert (R.bits(got)[R.FULL_COL, :] == 0).all() and (R.bits(got)[:, R.FULL_COL] == 0).all()
            assert np.isfinite(got).all() and (np.abs(got) < 1e9).all()
    if dim > 1 and rows >= 63:
        assert not np.array_equal(R.bits(c["R"])[iu], R.bits(c["R0"])[iu])      # the two means ask different questions
    E.column_sums(ds)                                   # shares the scratch slots of the products
    assert same_bits(E.centered_products(ds, c["mean"]), np.asarray(c["R"]))
    ds.close()


def test_generated_rows_equal_uploaded_rows(eng, E):
    """a data set made on the device (Dataset(generate=...)) and the same rows uploaded from gen_rows: same sums, same
    centred sums, and both the replay's"""
    seed, k, dim, rows = 4711, 6, 24, 1000
    x, _ = E.gen_rows(seed, k, dim, 0, rows)
    g = E.Dataset(eng, generate=(seed, k, dim, 0, rows))
    h = E.Dataset(eng, x)
    gs, gc = E.column_sums(g)
    hs, hc = E.column_sums(h)
    ws, wc = R.column_sums(x)
    assert same_bits(gs, hs) and same_bits(gs, ws) and np.array_equal(gc, hc) and np.array_equal(gc, wc)
    mean = R.mean_of(ws, wc)
    gr, hr = E.centered_products(g, mean), E.centered_products(h, mean)
    assert same_bits(gr, hr) and same_bits(gr, R.centered_products(x, None, mean))
    g.close()
    h.close()


# ------------------------------------------------------------------ k_column_minmax
def minmax_host(x, mask):
    """numpy on the host rows: (lo, hi, count); a component without data gives +FLT_MAX, -FLT_MAX, 0 as the ABI says"""
    on = np.ones(x.shape, dtype=bool) if mask is None else mask == 0
    lo = np.where(on, x, np.float32(np.inf)).min(0)
    hi = np.where(on, x, np.float32(-np.inf)).max(0)
    cnt = on.sum(0).astype(np.int64)
    return np.where(cnt > 0, lo, FLT_MAX), np.where(cnt > 0, hi, -FLT_MAX), cnt


def same_extremes(got, want):
    """bit patterns, except that a zero only has to be a zero: the kernel's ordered-integer fold puts -0 below +0, the
    reference's `<` leaves whichever came first, and randinit_codes cannot observe the difference"""
    return got.dtype == np.float32 and np.array_equal(np.where(got == 0, np.float32(0), got).view(np.uint32),
                                                      np.where(want == 0, np.float32(0), want).view(np.uint32))


# rows 1, one under / at / one over the 256 rows a block gets at least, 2049 * 3 (25 blocks of 246 rows, the last with
# 243), and a second block of columns
MINMAX_SHAPES = [(1, 3), (255, 3), (256, 3), (257, 3), (2049 * 3, 3), (300, 257)]


@pytest.mark.parametrize("rows,dim", MINMAX_SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_column_minmax_edges(eng, E, rows, dim, masked):
    rs = np.random.RandomState(rows * 3 + dim)
    x = (3.0 * rs.standard_normal((rows, dim)) - 1.0).astype(np.float32)
    x[rs.rand(rows, dim) < 0.05] = 0.0
    x[rs.rand(rows, dim) < 0.05] = -0.0
    mask = None
    if masked:
        mask = (rs.rand(rows, dim) < 0.3).astype(np.uint8)
        mask[:, dim - 1] = 1                                # a component without data
        if rows > 1:
            mask[0, 0] = 0
        x[(mask != 0) & (rs.rand(rows, dim) < 0.5)] = np.nan
    ds = E.Dataset(eng, x, mask=mask)
    lo, hi, cnt = E.column_minmax(ds)
    ds.close()
    wlo, whi, wcnt = minmax_host(x, mask)
    assert np.array_equal(cnt, wcnt) and same_extremes(lo, wlo) and same_extremes(hi, whi)
    if masked:
        assert cnt[dim - 1] == 0 and lo[dim - 1] == FLT_MAX and hi[dim - 1] == -FLT_MAX


def test_column_minmax_special_columns(eng, E):
    """2049 * 3 rows in 25 row blocks: a column whose unmasked values all lie in one row block (the other blocks issue
    no atomics), a column of negative denormals, a column holding only +-FLT_MAX, one of each sign alone, and a column
    with a single unmasked value in the last (short) block"""
    rows, dim = 2049 * 3, 7
    rs = np.random.RandomState(5)
    x = rs.standard_normal((rows, dim)).astype(np.float32)
    mask = np.zeros((rows, dim), dtype=np.uint8)
    mask[:, 0] = 1
    mask[300:400, 0] = 0                                    # rows 246 .. 491 are block 1
    x[:, 1] = -(rs.randint(1, 1 << 23, size=rows).astype(np.uint32)).view(np.float32)
    x[:, 2] = np.where(rs.rand(rows) < 0.5, FLT_MAX, -FLT_MAX)
    x[:, 3] = FLT_MAX
    x[:, 4] = -FLT_MAX
    mask[:, 5] = 1
    mask[rows - 1, 5] = 0
    x[(mask != 0)] = np.float32(1e30)
    assert (x[:, 1] < 0).all() and (np.abs(x[:, 1]) < np.float32(1.17549435e-38)).all()
    ds = E.Dataset(eng, x, mask=mask)
    lo, hi, cnt = E.column_minmax(ds)
    ds.close()
    wlo, whi, wcnt = minmax_host(x, mask)
    assert np.array_equal(cnt, wcnt) and cnt[0] == 100 and cnt[5] == 1
    assert np.array_equal(R.bits(lo), R.bits(wlo)) and np.array_equal(R.bits(hi), R.bits(whi))
    assert lo[2] == -FLT_MAX and hi[2] == FLT_MAX and lo[3] == FLT_MAX and hi[4] == -FLT_MAX
    assert lo[5] == hi[5] == x[rows - 1, 5]
