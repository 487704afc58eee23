"""numpy restatement of SOM_PAK's lininit (find_eigenvectors som_rout.c:211-345, lininit_codes :347-429), bit for bit:
the witness the GPU tests of the two data passes compare against.

The two passes over the data, as the reference runs them.  Every output element is its own fp32 chain over the rows in
file order; a masked component takes no part, whatever value is stored at it:

    m[i]    = (float)(m[i] + x[r][i])                                       :250
    c_i     = (float)(x[r][i] - m[i])                                       :281, one rounding
    R[i][j] = (float)(R[i][j] + (float)(c_i * c_j))     for j >= i          :281, product rounded before the add

column_sums / centered_products below walk the rows and form all elements of a row at once, one numpy operation per
rounding, so nothing is re-associated and nothing is fused.  column_sums64 / centered_products64 are the same sums in
float64 with the bounds a recursive fp32 sum cannot leave (Higham, Accuracy and Stability of Numerical Algorithms,
sec. 4.2: n - 1 adds give gamma(n - 1) <= gamma(n); with one more rounding per product, gamma(n + 1)):

    |m32 - m64| <= gamma(n)     * sum_r |x_ri|                  gamma(k) = k u / (1 - k u), u = 2^-24
    |R32 - R64| <= gamma(n + 1) * sum_r |c_ri * c_rj|           on the same fp32-centred c

The rest of the reference's path carries the type C gives each operation (float = np.float32, double = np.float64; the
reference is built with -ffp-contract=off):

    m[i] /= k2[i];  r[j][i] = r[i][j] /= k                      float / (float) long
    u = orand() / 16384.0 - 1.0                                 double, stored as float
    normalize: sum += v*v float chain; sum = (float) sqrt((double) sum); v /= sum
    v[i][j] = mu[i] * dotprod(r[j], u[i]) + u[i][j]             float; dotprod a float chain in index order
    gram_schmidt: sum -= w[t] * w[p] * v[p]                     ((w[t] * w[p]) * v[p]) float, chain over p
    sum += fabs(v[i][j] / dotprod(r[j], v[i]))                  float quotient, double add, float store; NOT reset
    mu[i] = sum / n                                             between the two vectors
    axis[i][j] = (float)((double) u[i][j] / sqrt((double) mu[i]))
    xf = (float)(4.0 * (float)(index % xdim) / (xdim - 1.0) - 2.0);  code = (m + xf * e1) + yf * e2   float

tests/test_lininit_replay.py pins all of this to the real reference's find_eigenvectors in memory.

Also here: the shapes of the edge tests, their seeded inputs, and the writer of masked text data that
tests/golden/make_golden.py and the tool tests share.
"""
import functools

import numpy as np

from som_lvq_pak_amd import engine as E

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------ the two data passes, in order, in fp32
def _unmasked(x, mask):
    return np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) == 0


def column_sums(x, mask=None):
    """(sum float32[dim], count int64[dim]): m[i] += x[r][i] over the unmasked entries, rows in order (:244-254)"""
    x = np.ascontiguousarray(x, dtype=f32)
    on = _unmasked(x, mask)
    acc = np.zeros(x.shape[1], dtype=f32)
    with np.errstate(all="ignore"):
        for r in range(x.shape[0]):
            acc = np.where(on[r], acc + x[r], acc)
    return acc, on.sum(0).astype(np.int64)


def mean_of(s, cnt):
    """m[i] /= k2[i] (:258-259): float by (float) long; 0 / 0 where a component has no data"""
    with np.errstate(all="ignore"):
        return (np.asarray(s, dtype=f32) / np.asarray(cnt).astype(f32)).astype(f32)


def centered_products(x, mask, mean):
    """float32[dim, dim], j >= i filled and j < i zero: R[i][j] += (x_i - m_i) * (x_j - m_j), rows in order (:269-283)"""
    x = np.ascontiguousarray(x, dtype=f32)
    mean = np.asarray(mean, dtype=f32)
    on = _unmasked(x, mask)
    d = x.shape[1]
    R = np.zeros((d, d), dtype=f32)
    with np.errstate(all="ignore"):
        for r in range(x.shape[0]):
            c = x[r] - mean
            p = np.outer(c, c)
            R = np.where(np.outer(on[r], on[r]), R + p, R)
    return np.triu(R)


# ------------------------------------------------------------------ the same sums in float64, with their bounds
def column_sums64(x, mask=None):
    """(sum float64[dim], bound float64[dim]): the exact-in-double sums and gamma(n) * sum |x|"""
    on = _unmasked(x, mask)
    v = np.where(on, np.asarray(x, dtype=f32), f32(0)).astype(f64)
    return v.sum(0), gamma(x.shape[0]) * np.abs(v).sum(0)


def centered_products64(x, mask, mean):
    """(R float64[dim, dim], bound float64[dim, dim]), full squares: the products of the SAME fp32-centred values,
    summed in double, and gamma(n + 1) * sum |c_i c_j|"""
    x = np.ascontiguousarray(x, dtype=f32)
    on = _unmasked(x, mask)
    with np.errstate(all="ignore"):
        c = (x - np.asarray(mean, dtype=f32)[None, :]).astype(f32)
    c = np.where(on, c, f32(0)).astype(f64)
    return c.T @ c, gamma(x.shape[0] + 1) * (np.abs(c).T @ np.abs(c))


# ------------------------------------------------------------------ the host part of find_eigenvectors
def _chain(terms):
    """fp32 sum of `terms` along the last axis, in index order, starting from 0"""
    acc = np.zeros(terms.shape[:-1], dtype=f32)
    for p in range(terms.shape[-1]):
        acc = acc + terms[..., p]
    return acc


def _normalize(v):
    s = f32(np.sqrt(f64(_chain(v * v))))
    return v / s


def _dots(r, u):
    """[dotprod(r[j], u) for j] (:178-185): a chain over the index of u for every row of r"""
    return _chain(r * u[None, :])


def _gram_schmidt2(v):
    """gram_schmidt(v, n, 2) (:188-209)"""
    w0 = _normalize(v[0].copy())
    s = v[1].copy()
    for p in range(v.shape[1]):
        s = s - (w0 * w0[p]) * v[1][p]
    return np.stack([w0, _normalize(s)])


def eigenvectors(s, cnt, R, k, seed):
    """find_eigenvectors from :256 on: `s`, `cnt` the column sums and counts, `R` the upper triangle of the centred
    sums (as centered_products returns it), k rows.  float32[3, dim] (mean, two scaled axes), or None (:256, :313)."""
    if k < 3:
        return None
    n = R.shape[0]
    with np.errstate(all="ignore"):
        m = mean_of(s, cnt)
        r = (np.triu(R) / f32(k)).astype(f32)
        r = np.where(np.tri(n, k=-1, dtype=bool), r.T, r)
        u = (E.orand_stream(seed, 2 * n).astype(f64) / 16384.0 - 1.0).astype(f32).reshape(2, n)
        u = np.stack([_normalize(u[0]), _normalize(u[1])])
        mu = [f32(1.0), f32(1.0)]
        for _ in range(10):
            v = np.stack([mu[i] * _dots(r, u[i]) + u[i] for i in range(2)])
            v = _gram_schmidt2(v)
            acc = f32(0.0)
            for i in range(2):
                q = np.abs(v[i] / _dots(r, v[i])).astype(f64)
                for j in range(n):
                    acc = f32(f64(acc) + q[j])
                mu[i] = acc / f32(n)
            u = v
        if mu[0] == 0.0 or mu[1] == 0.0:
            return None
        ax = [(u[i].astype(f64) / np.sqrt(f64(mu[i]))).astype(f32) for i in range(2)]
    return np.stack([m, ax[0], ax[1]])


def find_eigenvectors(x, mask, seed):
    """the whole of find_eigenvectors from this file's own sums and its own R"""
    x = np.ascontiguousarray(x, dtype=f32)
    s, cnt = column_sums(x, mask)
    if x.shape[0] < 3:
        return None
    return eigenvectors(s, cnt, centered_products(x, mask, mean_of(s, cnt)), x.shape[0], seed)


def plane_of_codes(eig, xdim, ydim):
    """lininit_codes :409-424: the map laid out on the plane of the two axes, float32[xdim * ydim, dim]"""
    idx = np.arange(xdim * ydim)
    with np.errstate(all="ignore"):
        xf = (4.0 * (idx % xdim).astype(f32).astype(f64) / (xdim - 1.0) - 2.0).astype(f32)
        yf = (4.0 * (idx // xdim).astype(f32).astype(f64) / (ydim - 1.0) - 2.0).astype(f32)
        return (eig[0][None, :] + xf[:, None] * eig[1][None, :]) + yf[:, None] * eig[2][None, :]


def lininit_codes(x, mask, xdim, ydim, seed):
    """lininit_codes (som_rout.c:347-429) after init_random(seed); None where it cannot find eigenvectors"""
    eig = find_eigenvectors(x, mask, seed)
    return None if eig is None else plane_of_codes(eig, xdim, ydim)


# ------------------------------------------------------------------ the shapes of the edge tests and their inputs
# (dim, rows): the smallest at which each branch of k_column_sums (256 columns a block) and k_centered_products (16 x 16
# elements a block, 64 rows a stage) first exists
SHAPES = [(1, 3),                 # smallest case
          (15, 63), (16, 64),     # one block, under and at both edges
          (17, 65),               # a second block in i and j, one skipped bj < bi block, a ragged last row block
          (33, 130),              # 3 x 3 blocks; three row blocks, the last partial
          (257, 70),              # second block of k_column_sums; 17 x 17 blocks
          (300, 200)]             # larger multi-block case
MASK_RATE = 0.15
FULL_COL, FULL_ROW = 20, 77       # of the masked (33, 130) case


def gen_spec(dim, rows):
    """(seed, centres) of the generator stream of a shape"""
    return 7000 + 31 * dim + rows, 5


def case(dim, rows, masked):
    """the inputs of one case: x (engine.gen_rows, for the centred sums), xs (the same rows scaled element-wise by
    10**U(-3, 3), for the column sums: plain rows round too rarely differently from a double sum), mask or None.
    The masked (33, 130) case has one column masked in every row, one row masked entirely, and NaN / 1e30 stored at
    masked positions."""
    seed, k = gen_spec(dim, rows)
    x, _ = E.gen_rows(seed, k, dim, 0, rows)
    rs = np.random.RandomState(seed)
    with np.errstate(all="ignore"):
        xs = (x.astype(f64) * 10.0 ** rs.uniform(-3.0, 3.0, size=x.shape)).astype(f32)
    mask = None
    if masked:
        mask = (rs.rand(rows, dim) < MASK_RATE).astype(np.uint8)
        if (dim, rows) == (33, 130):
            mask[:, FULL_COL] = 1
            mask[FULL_ROW, :] = 1
            x, xs = x.copy(), xs.copy()
            for a in (x, xs):
                a[(mask != 0) & (rs.rand(rows, dim) < 0.5)] = np.nan
                a[(mask != 0) & ~np.isnan(a) & (rs.rand(rows, dim) < 0.5)] = f32(1e30)
    return {"dim": dim, "rows": rows, "x": x, "xs": xs, "mask": mask}


@functools.lru_cache(maxsize=None)
def replayed(dim, rows, masked):
    """the case and its replay, computed once and shared read-only: s, cnt (sums of x), mean, R (with that mean),
    R0 (with the zero vector as mean), ss, scnt (sums of xs)"""
    c = case(dim, rows, masked)
    c["s"], c["cnt"] = column_sums(c["x"], c["mask"])
    c["ss"], c["scnt"] = column_sums(c["xs"], c["mask"])
    c["mean"] = mean_of(c["s"], c["cnt"])
    c["R"] = centered_products(c["x"], c["mask"], c["mean"])
    c["R0"] = centered_products(c["x"], c["mask"], np.zeros(dim, dtype=f32))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ------------------------------------------------------------------ masked text data for the tools
GEN_CASES = [(17, 65), (257, 70), (512, 300)]       # `-din gen:...` sources (dim, n), seeds from gen_spec
TEXT_CASES = [(33, 130), (300, 200)]                # masked text (dim, rows)


def masked_text_rows(dim, rows):
    """(x, mask) of a text case: generator rows and a 15 % mask without a fully masked column or row"""
    seed, k = gen_spec(dim, rows)
    x, _ = E.gen_rows(seed + 1, k, dim, 0, rows)
    mask = (np.random.RandomState(seed + 1).rand(rows, dim) < MASK_RATE).astype(np.uint8)
    mask[mask.all(1), 0] = 0
    mask[0, mask.all(0)] = 0
    return x, mask


def write_text(path, x, mask=None):
    """a .dat file of the rows: %.9g values (an exact round trip through sscanf("%f")), `x` for masked entries"""
    with open(path, "w") as f:
        f.write("%d\n" % x.shape[1])
        for r in range(x.shape[0]):
            f.write(" ".join("x" if mask is not None and mask[r, i] else "%.9g" % x[r, i]
                             for i in range(x.shape[1])) + "\n")


def write_masked_text(path, dim, rows):
    x, mask = masked_text_rows(dim, rows)
    write_text(path, x, mask)
    return x, mask


def rows_of(src):
    """(x, mask) of a recorded data source of tests/golden/cli/expected.json["som"]["lininit_edges"]["data"]"""
    if "gen" in src:
        f = dict(kv.split("=") for kv in src["gen"][4:].split(","))
        return E.gen_rows(int(f["seed"]), int(f["k"]), int(f["dim"]), 0, int(f["n"]))[0], None
    return masked_text_rows(*src["masked_text"])


def cod_text(codes, args):
    """the bytes lininit writes for `codes` (header, the seed comment of mapinit.c, "%g " per value, datafile.c:420-447);
    `args` the recorded command line"""
    a = dict(zip(args[0::2], args[1::2]))
    out = ["%d %s %s %s %s\n# random seed: %s\n" % (codes.shape[1], a["-topol"], a["-xdim"], a["-ydim"], a["-neigh"], a["-rand"])]
    for row in codes:
        out.append("".join("%g " % float(v) for v in row) + "\n")
    return "".join(out).encode()
