"""CPU replay of batch GLVQ (somhip_glvq_train, K9) for tests/test_glvq.py.  Plain numpy.

The squared distances are float32 chains -- sub, mul, add in dimension order, each a float32 array operation, so each
rounds once.  Everything behind them is float64 with the operation order of include/somhip.h written out: one numpy
operation per rounding.  The per-prototype sums are loops of float64 additions in data order from +0.0.  For the sigmoid
the replay also returns the bounds its comparison with the device has to meet (DESIGN.md K9 derives them), and the
update is formed in np.longdouble with its allowance, the way batchmap_replay.combine does."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -53                                   # the unit roundoff of float64


def alpha_at(alpha, epochs, t):
    """alpha_t = alpha * (float)(T - t) / (float)T, every operation in float"""
    return f32(f32(f32(alpha) * f32(epochs - t)) / f32(epochs))


def dist_sq(codes, data):
    """d[s][j]: the reference's float chain, acc += (c - x) * (c - x) in dimension order with three roundings"""
    ct, dt = np.ascontiguousarray(np.asarray(codes, dtype=f32).T), np.ascontiguousarray(np.asarray(data, dtype=f32).T)
    acc = np.zeros((dt.shape[1], ct.shape[1]), dtype=f32)
    for k in range(ct.shape[0]):
        t = ct[k][None, :] - dt[k][:, None]
        p = t * t
        acc = acc + p
    assert acc.dtype == f32
    return acc


def search(codes, clab, data, dlab, first=0, n=None):
    """(dplus, iplus, dminus, iminus) of run samples s < n, data rows (first + s) % rows: per role the smallest distance
    and, among equal distances, the lowest row (np.argmin takes the first minimum)"""
    rows = data.shape[0]
    n = rows if n is None else n
    r = (first + np.arange(n)) % rows
    d = dist_sq(codes, data)[r]
    own = np.asarray(clab)[None, :] == np.asarray(dlab)[r][:, None]
    assert own.any(axis=1).all() and (~own).any(axis=1).all()
    big = f32(np.inf)
    ip = np.argmin(np.where(own, d, big), axis=1)
    im = np.argmin(np.where(own, big, d), axis=1)
    s = np.arange(n)
    return d[s, ip].copy(), ip.astype(np.int32), d[s, im].copy(), im.astype(np.int32)


def terms(dplus, iplus, dminus, iminus, beta=0.0):
    """(xi_plus, xi_minus, f, correct) in float64, one rounding per operation in the order of the definition"""
    dp, dm = dplus.astype(f64), dminus.astype(f64)
    D = dp + dm
    zero = D == 0.0
    Ds = np.where(zero, f64(1.0), D)
    num = dp - dm
    mu = np.where(zero, f64(0.0), num / Ds)
    if beta == 0.0:
        f, fp = mu.copy(), np.ones_like(mu)
    else:
        b = f64(f32(beta))
        t = b * mu
        ex = np.array([math.exp(v) for v in -t], dtype=f64)        # the C library's exp: within 1 ulp
        den = f64(1.0) + ex
        f = f64(1.0) / den
        bf = b * f
        om = f64(1.0) - f
        fp = bf * om
    four = f64(4.0) * fp
    DD = Ds * Ds
    xp = np.where(zero, f64(0.0), (four * dm) / DD)
    xm = np.where(zero, f64(0.0), (four * dp) / DD)
    kp = (dplus.view(np.uint32).astype(np.uint64) << np.uint64(32)) | iplus.astype(np.uint64)
    km = (dminus.view(np.uint32).astype(np.uint64) << np.uint64(32)) | iminus.astype(np.uint64)
    return xp, xm, f, int((kp < km).sum())


def sums(data, iplus, iminus, xp, xm, f, n_units, first=0):
    """dict of step 4: sums_plus / sums_minus [units][dim + 1] (last column the sum of xi), n_plus, n_minus, cost; each a
    chain of float64 additions from +0.0 in data order, the product rounded before it is added.  abs_plus / abs_minus:
    the same sums over |xi x| (what the sigmoid's bounds scale with)."""
    rows, dim = data.shape
    n = len(iplus)
    x = np.concatenate([data.astype(f64), np.ones((rows, 1), dtype=f64)], axis=1)     # xi * 1.0 is xi: the trailing column
    out = {"sums_plus": np.zeros((n_units, dim + 1), dtype=f64), "sums_minus": np.zeros((n_units, dim + 1), dtype=f64),
           "abs_plus": np.zeros((n_units, dim + 1), dtype=f64), "abs_minus": np.zeros((n_units, dim + 1), dtype=f64),
           "n_plus": np.zeros(n_units, dtype=np.uint32), "n_minus": np.zeros(n_units, dtype=np.uint32),
           "cost": np.zeros(n_units, dtype=f64)}
    for s in range(n):
        xr = x[(first + s) % rows]
        j, k = int(iplus[s]), int(iminus[s])
        p = xp[s] * xr
        out["sums_plus"][j] = out["sums_plus"][j] + p
        out["abs_plus"][j] += np.abs(p)
        out["cost"][j] = out["cost"][j] + f[s]
        out["n_plus"][j] += 1
        m = xm[s] * xr
        out["sums_minus"][k] = out["sums_minus"][k] + m
        out["abs_minus"][k] += np.abs(m)
        out["n_minus"][k] += 1
    return out


def update(codes, S, alpha_t, n):
    """step 5 in float64: the rows after it; rows no sample chose keep their bits"""
    W = codes.astype(f64)
    a = f64(f32(alpha_t)) / f64(n)
    d = codes.shape[1]
    Sp, sp = S["sums_plus"][:, :d], S["sums_plus"][:, d:]
    Sm, sm = S["sums_minus"][:, :d], S["sums_minus"][:, d:]
    pw, mw = sp * W, sm * W
    gp, gm = Sp - pw, Sm - mw
    g = gp - gm
    step = a * g
    new = (W + step).astype(f32)
    live = (S["n_plus"] > 0) | (S["n_minus"] > 0)
    out = codes.copy()
    out[live] = new[live]
    return out


def epoch(codes, clab, data, dlab, alpha_t, beta=0.0, first=0, n=None):
    """(the rows after one epoch, its cost, its correct count, the stage results)"""
    n = data.shape[0] if n is None else n
    dp, ip, dm, im = search(codes, clab, data, dlab, first, n)
    xp, xm, f, correct = terms(dp, ip, dm, im, beta)
    S = sums(data, ip, im, xp, xm, f, codes.shape[0], first)
    chain = f64(0.0)
    for c in S["cost"]:
        chain = chain + c
    return update(codes, S, alpha_t, n), chain / f64(n), correct, S


def train(codes, clab, data, dlab, epochs, alpha, beta=0.0, first=0, n=None, start_epoch=0, count=None):
    """(rows, cost[count], correct[count]) of epochs [start_epoch, start_epoch + count)"""
    count = epochs - start_epoch if count is None else count
    cost, correct = np.zeros(count, dtype=f64), np.zeros(count, dtype=np.int64)
    for i in range(count):
        codes, cost[i], correct[i], _ = epoch(codes, clab, data, dlab, alpha_at(alpha, epochs, start_epoch + i), beta, first, n)
    return codes, cost, correct


# ---- the sigmoid's bounds -------------------------------------------------------------------------------
def xi_rel_bound(beta):
    """|xi_device - xi_replay| <= this * xi: both exps within 1 ulp of the true value, |beta mu| <= beta"""
    return (20.0 + 8.0 * math.exp(float(f32(beta)))) * U


F_REL_BOUND = 8.0 * U           # ... and of f


def sums_bound(S, beta):
    """(bound of sums_plus, of sums_minus, of cost): a list of m terms, each within xi_rel_bound + 2 U of the replay's,
    added by a chain whose m roundings may each differ on both sides"""
    rel = xi_rel_bound(beta) + 2.0 * U
    mp = S["n_plus"].astype(f64)[:, None]
    mm = S["n_minus"].astype(f64)[:, None]
    tiny = np.finfo(f64).tiny
    return ((rel + 2.0 * mp * U) * S["abs_plus"] * 1.001 + tiny, (rel + 2.0 * mm * U) * S["abs_minus"] * 1.001 + tiny,
            (F_REL_BOUND + 2.0 * U + 2.0 * mp[:, 0] * U) * np.abs(S["cost"]) * 1.001 + tiny)


def ulp32(q):
    """the spacing of floats in the binade of |q| (q: float64 array)"""
    _, e = np.frexp(np.abs(q))
    e = np.where(q == 0, -10000, e)
    return np.ldexp(f64(1.0), np.maximum(e - 24, -149))


def update_longdouble(codes, S, alpha_t, n, beta):
    """(q, bound): q = W + a ((Sp - sp W) - (Sm - sm W)) in np.longdouble from the replay's sums, and the allowance a
    device row formed from the device's own sums has to meet: the rounding to float, the sums' bounds carried through
    a g, and the float64 roundings of the update (at most 8 U on each of the four magnitudes, 2 U on the result)"""
    ld = np.longdouble
    d = codes.shape[1]
    W = codes.astype(ld)
    a = ld(f64(f32(alpha_t))) / ld(n)
    bp, bm, _ = sums_bound(S, beta)
    Sp, sp = S["sums_plus"][:, :d].astype(ld), S["sums_plus"][:, d:].astype(ld)
    Sm, sm = S["sums_minus"][:, :d].astype(ld), S["sums_minus"][:, d:].astype(ld)
    q = W + a * ((Sp - sp * W) - (Sm - sm * W))
    mag = np.abs(Sp) + np.abs(sp * W) + np.abs(Sm) + np.abs(sm * W)
    carried = bp[:, :d] + bp[:, d:] * np.abs(W) + bm[:, :d] + bm[:, d:] * np.abs(W)
    bound = ulp32(q.astype(f64)).astype(ld) / 2 + a * (carried + 8 * U * mag) + 2 * U * np.abs(q)
    return q, bound
