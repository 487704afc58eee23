"""CPU replay of the batch map (somhip_som_batchmap, K8) for tests/test_batchmap.py.

The winners are the oracle's find_winner_euc (the lowest index on equal distances).  Everything else is numpy: the
per-unit sums are loops of np.float64 additions in data order from +0.0; the lattice distances restate hexa_dist /
rect_dist (som_rout.c:434-470) float by float and double by double; the bubble membership is the reference's own
`dist <= radius` (som_rout.c:496) and the gaussian weight its exp((double)(-dd * dd / (2.0 * radius * radius)))
(som_rout.c:808); the combine is formed in np.longdouble together with the bound its fp64 evaluation has to meet."""
import numpy as np

TOPOL_HEXA, TOPOL_RECT = 3, 4
NEIGH_BUBBLE, NEIGH_GAUSSIAN = 1, 2
f32, f64 = np.float32, np.float64


def radius_at(radius, epochs, t):
    """r_t = 1.0f + (radius - 1.0f) * (float)(T - t) / (float)T, every operation in float (som_rout.c:615)"""
    return f32(f32(1.0) + f32(f32(f32(radius) - f32(1.0)) * f32(epochs - t)) / f32(epochs))


def winners(oracle, codes, data):
    """(winner, squared distance) of every data row: find_winner_euc"""
    idx, diff, ret = oracle.winners(np.ascontiguousarray(codes, dtype=f32), np.ascontiguousarray(data, dtype=f32), 1, False, None)
    assert (ret != 0).all() and (idx[:, 0] >= 0).all()
    return idx[:, 0].astype(np.int64), diff[:, 0].copy()


def sums(win, data, n_units, first=0, n=None):
    """hits[u] and S[u][k] over data rows (first + s) % len(data), s < n: per unit one chain of fp64 additions in data
    order, starting from +0.0"""
    rows, dim = data.shape
    n = rows if n is None else n
    hits = np.zeros(n_units, dtype=np.uint32)
    S = np.zeros((n_units, dim), dtype=f64)
    x = data.astype(f64)
    for s in range(n):
        r = (first + s) % rows
        u = int(win[r])
        hits[u] += 1
        S[u] = S[u] + x[r]                 # elementwise: dim independent chains
    return hits, S


def qerror_chain(d1, first=0, n=None):
    """find_qerror's float: qerror += sqrt((double) diff) on a float accumulator (som_rout.c:715), in data order"""
    rows = len(d1)
    n = rows if n is None else n
    q = f32(0.0)
    for s in range(n):
        q = f32(f64(q) + np.sqrt(f64(d1[(first + s) % rows])))
    return q


def lattice_dist(topol, xdim, ydim):
    """dist[i][j]: hexa_dist / rect_dist (floats) between the winner j (bx, by) and the unit i (tx, ty)"""
    u = np.arange(xdim * ydim)
    x, y = u % xdim, u // xdim
    bx, by, tx, ty = x[None, :], y[None, :], x[:, None], y[:, None]
    diff = (bx - tx).astype(f32)
    dyi = by - ty + 0 * bx
    dy = dyi.astype(f32)
    if topol == TOPOL_RECT:
        ret = diff * diff
        ret = ret + dy * dy                                          # float, som_rout.c:461-464
    else:
        odd = (dyi % 2) != 0
        shift = np.where((by + 0 * ty) % 2 == 0, f64(-0.5), f64(0.5))
        diff = np.where(odd, (diff.astype(f64) + shift).astype(f32), diff)      # diff -= 0.5 / += 0.5, :441-446
        ret = diff * diff
        ret = (ret.astype(f64) + f64(0.75) * dy.astype(f64) * dy.astype(f64)).astype(f32)   # ret += 0.75 * diff * diff, :449
    assert ret.dtype == f32
    return np.sqrt(ret.astype(f64)).astype(f32)                      # (float) sqrt((double) ret)


def weights(topol, neigh, xdim, ydim, r):
    """h[i][j] in float64 at radius r (a float)"""
    r = f32(r)
    dd = lattice_dist(topol, xdim, ydim)
    if neigh == NEIGH_BUBBLE:
        return (dd <= r).astype(f64)
    neg = -(dd * dd)
    assert neg.dtype == f32
    return np.exp(neg.astype(f64) / (f64(2.0) * f64(r) * f64(r)))


def ulp32(q):
    """the spacing of floats in the binade of |q| (q: float64 array)"""
    _, e = np.frexp(np.abs(q))
    e = np.where(q == 0, -10000, e)
    return np.ldexp(f64(1.0), np.maximum(e - 24, -149))


def combine(h, hits, S):
    """(q, D, bound): q = N / D in np.longdouble where D > 0, and the allowance
    ulp32(q) / 2 + (2 * units + 16) * 2^-52 * A / D, A[i][k] = sum_j h |S[j][k]|"""
    ld = np.longdouble
    units = h.shape[0]
    hl = h.astype(ld)
    N = hl @ S.astype(ld)
    A = hl @ np.abs(S).astype(ld)
    D = hl @ hits.astype(ld)
    live = D > 0
    Ds = np.where(live, D, 1)[:, None]
    q = N / Ds
    bound = ulp32(q.astype(f64)).astype(ld) / 2 + ld(2 * units + 16) * ld(2.0) ** -52 * A / Ds
    return q, D, bound


def epoch(oracle, codes, data, topol, neigh, xdim, ydim, r, first=0, n=None):
    """one epoch in float64 (N / D rounded to float): the codebook after it, the qerror before it"""
    win, d1 = winners(oracle, codes, data)
    hits, S = sums(win, data, codes.shape[0], first, n)
    h = weights(topol, neigh, xdim, ydim, r)
    D = h @ hits.astype(f64)
    out = codes.copy()
    live = D > 0
    out[live] = ((h @ S)[live] / D[live][:, None]).astype(f32)
    return out, qerror_chain(d1, first, n)
