"""CPU replay of map distortion (somhip_distortion_*, K1d) for tests/test_map_distortion.py.

The winners, the per-unit counts and sums and the neighbourhood weights are the batch map's replay (batchmap_replay.py),
imported and unchanged.  New here: q_s = |x_s|^2 in the order the header writes down (64 lane partials over k = l, l + 64,
..., then the xor butterfly 32 .. 1), the per-unit chains Q of them in data order, and the energy formed in np.longdouble
together with the bounds its fp64 evaluation has to meet.

The bounds, eps = 2^-52, R_j = A_j + sum_k (2 |m_jk| Nabs_jk + D_j m_jk^2) with Nabs = H |S|:
  |e_j - ref| <= c_unit(units, dim) * eps * R_j,     c_unit = 2 units + dim + 24
  |E - ref|   <= c_total(units, dim) * eps * sum_j R_j,  c_total = 3 units + dim + 24
and, for states accumulated from data, `chain_extra` more on R formed from the samples' absolute values."""
import numpy as np

from batchmap_replay import lattice_dist, sums, weights, winners  # noqa: F401  (re-exported for the tests)

f32, f64, ld = np.float32, np.float64, np.longdouble
EPS = ld(2.0) ** -52


def sample_sq(x):
    """q_s of every row of x (float32 [n, dim]) in fp64: lane l adds (double)x[k] * (double)x[k] for k = l, l + 64, ... in
    order from +0.0 (a product of two floats is exact in fp64); the 64 partials are folded by the butterfly"""
    n, d = x.shape
    xd = x.astype(f64)
    part = np.zeros((n, 64), dtype=f64)
    for k0 in range(0, d, 64):
        blk = xd[:, k0:k0 + 64]
        w = blk.shape[1]
        part[:, :w] = part[:, :w] + blk * blk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    assert (part == part[:, :1]).all()
    return part[:, 0].copy()


def sq_sums(win, q, n_units, first=0, n=None):
    """Q[u]: per unit one chain of fp64 additions of q_s from +0.0 over rows (first + s) % len(q), s < n, in data order"""
    rows = len(q)
    n = rows if n is None else n
    Q = np.zeros(n_units, dtype=f64)
    for s in range(n):
        r = (first + s) % rows
        Q[int(win[r])] = Q[int(win[r])] + q[r]
    return Q


def c_unit(units, dim):
    """2 units + 16: the MFMA sums over the source units, as K8 derives it (two fp64 roundings per term, the weight's exp,
    slack); 2: the three roundings of m * (D * m - 2 N); dim + 1: the additions over k, the column blocks and A_j in any
    order; 5: second-order terms"""
    return 2 * units + dim + 24


def c_total(units, dim):
    """c_unit, and the additions of the e_j over the units in any order"""
    return 3 * units + dim + 24


def chain_extra(max_hits, dim):
    """what the accumulated chains add, relative to the samples' absolute sums: hits * 2^-53 per chain of S and Q, and
    (ceil(dim / 64) + 6) * 2^-53 for q_s itself -- bounded by (max_hits + dim + 7) * 2^-52"""
    return max_hits + dim + 7


def evaluate(h, hits, S, Q, codes):
    """(e, E, R, D, scale) in np.longdouble from per-unit inputs: e_j = A_j - 2 sum_k m_jk N_jk + D_j |m_j|^2 where D_j > 0,
    else 0; R_j the sum of the absolute values of its terms; scale = sum_j 2 (A_j + D_j |m_j|^2) over the same units"""
    hl, m = h.astype(ld), codes.astype(ld)
    N = hl @ S.astype(ld)
    Nabs = hl @ np.abs(S).astype(ld)
    D = hl @ hits.astype(ld)
    A = hl @ Q.astype(ld)
    Aabs = hl @ np.abs(Q).astype(ld)
    msq = (m * m).sum(axis=1)
    live = D > 0
    e = np.where(live, A - 2 * (m * N).sum(axis=1) + D * msq, ld(0))
    R = np.where(live, Aabs + 2 * (np.abs(m) * Nabs).sum(axis=1) + D * msq, ld(0))
    scale = np.where(live, 2 * (A + D * msq), ld(0)).sum()
    return e, e.sum(), R, D, scale


def direct(h, win, x, codes):
    """(e, E, R) in np.longdouble from the samples: e_j = sum_s h(j, c(s)) |x_s - m_j|^2, and R_j = sum_s h(j, c(s))
    (|x_s|^2 + 2 sum_k |m_jk| |x_sk| + |m_j|^2), the absolute values of the terms the device's form is made of"""
    xl, m = x.astype(ld), codes.astype(ld)
    hw = h.astype(ld)[:, np.asarray(win)]                              # [units, samples]
    e = np.zeros(len(codes), dtype=ld)
    R = np.zeros(len(codes), dtype=ld)
    xsq = (xl * xl).sum(axis=1)
    for j in range(len(codes)):
        diff = xl - m[j]
        e[j] = (hw[j] * (diff * diff).sum(axis=1)).sum()
        R[j] = (hw[j] * (xsq + 2 * (np.abs(xl) * np.abs(m[j])).sum(axis=1) + (m[j] * m[j]).sum())).sum()
    return e, e.sum(), R
