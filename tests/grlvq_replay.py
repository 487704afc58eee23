"""CPU replay of batch GRLVQ (somhip_grlvq_train, K11) for tests/test_grlvq.py.  Plain numpy, on top of glvq_replay.

The weighted squared distances are float32 chains -- sub, mul by lambda, mul, add in dimension order, each a float32 array
operation, so each rounds once.  The terms are glvq_replay's.  The sums are glvq_replay's with the relevance chains beside
them: loops of float64 additions in data order from +0.0, one numpy operation per rounding.  The relevance gradient is a
loop over the rows in unit order, the update and the relevance step follow include/somhip.h operation by operation.  For
the sigmoid the replay also returns the bounds its comparison with the device has to meet."""
import numpy as np

import glvq_replay as G

f32, f64 = np.float32, np.float64
U = G.U


def rate_at(rate, epochs, t):
    """alpha_t and eps_t alike: rate * (float)(T - t) / (float)T, every operation in float"""
    return G.alpha_at(rate, epochs, t)


def dist_weighted(codes, data, lam):
    """d[s][j]: acc += (lambda[k] * (c - x)) * (c - x) in dimension order, four float32 roundings per component"""
    ct, dt = np.ascontiguousarray(np.asarray(codes, dtype=f32).T), np.ascontiguousarray(np.asarray(data, dtype=f32).T)
    lam = np.asarray(lam, dtype=f32)
    acc = np.zeros((dt.shape[1], ct.shape[1]), dtype=f32)
    for k in range(ct.shape[0]):
        t = ct[k][None, :] - dt[k][:, None]
        u = lam[k] * t
        p = u * t
        acc = acc + p
    assert acc.dtype == f32
    return acc


def search(codes, clab, data, dlab, lam, first=0, n=None):
    """glvq_replay.search under d_lambda: per role the smallest distance and, among equal distances, the lowest row"""
    rows = data.shape[0]
    n = rows if n is None else n
    r = (first + np.arange(n)) % rows
    d = dist_weighted(codes, data, lam)[r]
    own = np.asarray(clab)[None, :] == np.asarray(dlab)[r][:, None]
    assert own.any(axis=1).all() and (~own).any(axis=1).all()
    big = f32(np.inf)
    ip = np.argmin(np.where(own, d, big), axis=1)
    im = np.argmin(np.where(own, big, d), axis=1)
    s = np.arange(n)
    return d[s, ip].copy(), ip.astype(np.int32), d[s, im].copy(), im.astype(np.int32)


def sums(codes, data, iplus, iminus, xp, xm, f, first=0):
    """glvq_replay.sums' dict, and beside it rel_plus / rel_minus [units][dim]: per row and component one chain from +0.0
    in data order of xi * (td * td), td = (double)x - (double)w, and rel_abs_plus / rel_abs_minus, the same sums (their
    terms are not negative; what the sigmoid's bounds scale with); grad [dim]: the chain over the rows in unit order of
    (rel_plus - rel_minus)"""
    units, dim = codes.shape
    rows = data.shape[0]
    out = G.sums(data, iplus, iminus, xp, xm, f, units, first)
    W, x = codes.astype(f64), data.astype(f64)
    Rp, Rm = np.zeros((units, dim), dtype=f64), np.zeros((units, dim), dtype=f64)
    for s in range(len(iplus)):
        xr = x[(first + s) % rows]
        j, k = int(iplus[s]), int(iminus[s])
        td = xr - W[j]
        tt = td * td
        pr = xp[s] * tt
        Rp[j] = Rp[j] + pr
        td = xr - W[k]
        tt = td * td
        pr = xm[s] * tt
        Rm[k] = Rm[k] + pr
    grad = np.zeros(dim, dtype=f64)
    for j in range(units):
        t = Rp[j] - Rm[j]
        grad = grad + t
    out.update(rel_plus=Rp, rel_minus=Rm, grad=grad)
    return out


def update(codes, S, lam, alpha_t, n):
    """step 6 in float64: the rows after it; rows no sample chose keep their bits"""
    W = codes.astype(f64)
    a = f64(f32(alpha_t)) / f64(n)
    d = codes.shape[1]
    Sp, sp = S["sums_plus"][:, :d], S["sums_plus"][:, d:]
    Sm, sm = S["sums_minus"][:, :d], S["sums_minus"][:, d:]
    pw, mw = sp * W, sm * W
    gp, gm = Sp - pw, Sm - mw
    g = gp - gm
    al = a * np.asarray(lam, dtype=f32).astype(f64)
    step = al[None, :] * g
    new = (W + step).astype(f32)
    live = (S["n_plus"] > 0) | (S["n_minus"] > 0)
    out = codes.copy()
    out[live] = new[live]
    return out


def relevance_step(lam, grad, eps_t, n):
    """step 7 in float64: lambda after it (the array given where eps_t == 0 or every component is clamped)"""
    lam = np.asarray(lam, dtype=f32)
    if not f32(eps_t) > 0:
        return lam.copy()
    e = f64(f32(eps_t)) / (f64(2.0) * f64(n))
    step = e * np.asarray(grad, dtype=f64)
    l = lam.astype(f64) - step
    l = np.where(l < 0.0, f64(0.0), l)
    s = f64(0.0)
    for v in l:
        s = s + v
    if not s > 0:
        return lam.copy()
    return (l / s).astype(f32)


def epoch(codes, clab, data, dlab, lam, alpha_t, eps_t, beta=0.0, first=0, n=None):
    """(the rows after one epoch, lambda after it, its cost, its correct count, the stage results)"""
    n = data.shape[0] if n is None else n
    dp, ip, dm, im = search(codes, clab, data, dlab, lam, first, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im, beta)
    S = sums(codes, data, ip, im, xp, xm, f, first)
    chain = f64(0.0)
    for c in S["cost"]:
        chain = chain + c
    return update(codes, S, lam, alpha_t, n), relevance_step(lam, S["grad"], eps_t, n), chain / f64(n), correct, S


def train(codes, clab, data, dlab, lam, epochs, alpha, eps, beta=0.0, first=0, n=None, start_epoch=0, count=None):
    """(rows, lambda, cost[count], correct[count]) of epochs [start_epoch, start_epoch + count)"""
    count = epochs - start_epoch if count is None else count
    lam = np.asarray(lam, dtype=f32).copy()
    cost, correct = np.zeros(count, dtype=f64), np.zeros(count, dtype=np.int64)
    for i in range(count):
        t = start_epoch + i
        codes, lam, cost[i], correct[i], _ = epoch(codes, clab, data, dlab, lam, rate_at(alpha, epochs, t), rate_at(eps, epochs, t),
                                                   beta, first, n)
    return codes, lam, cost, correct


def evaluate(codes, clab, data, dlab, lam, beta=0.0):
    """(cost, accuracy) of a codebook under lambda: what an epoch reports of the state it starts from"""
    dp, ip, dm, im = search(codes, clab, data, dlab, lam)
    _, _, f, correct = G.terms(dp, ip, dm, im, beta)
    return float(f.sum()) / len(f), correct / len(f)


# ---- the sigmoid's bounds ------------------------------------------------------------------------------
def rel_bound(S, beta):
    """(bound of rel_plus, of rel_minus, of grad).  A term xi * tt has no cancellation: td and tt are the same roundings on
    both sides, xi is within glvq_replay.xi_rel_bound of the replay's, the product adds U on either side; a chain of m such
    non-negative terms is within (rel + 2 m U) of its own value.  grad: the bounds of both roles summed
    over the rows, the subtraction's and the chain's roundings on the magnitudes."""
    rel = G.xi_rel_bound(beta) + 2.0 * U
    mp = S["n_plus"].astype(f64)[:, None]
    mm = S["n_minus"].astype(f64)[:, None]
    tiny = np.finfo(f64).tiny
    bp = (rel + 2.0 * mp * U) * S["rel_plus"] * 1.001 + tiny
    bm = (rel + 2.0 * mm * U) * S["rel_minus"] * 1.001 + tiny
    units = S["rel_plus"].shape[0]
    mag = (S["rel_plus"] + S["rel_minus"]).sum(axis=0)
    bg = (bp + bm).sum(axis=0) + 2.0 * (units + 1) * U * mag * 1.001 + tiny
    return bp, bm, bg


def learning_case(seed):
    """the issue's learning data: three unit-variance classes with means (0,0), (3,0), (0,3) in components 0 and 1, six
    noise components of standard deviation 3, 200 rows per class, permuted; the prototypes the first two rows of each class"""
    rs = np.random.RandomState(seed)
    means = np.zeros((3, 8))
    means[1, 0] = 3.0
    means[2, 1] = 3.0
    scale = np.array([1, 1, 3, 3, 3, 3, 3, 3], dtype=f64)
    x = np.concatenate([means[c] + rs.standard_normal((200, 8)) * scale for c in range(3)]).astype(f32)
    lab = np.repeat(np.arange(3), 200).astype(np.int32)
    perm = rs.permutation(600)
    x, lab = x[perm], lab[perm]
    codes = np.concatenate([x[lab == c][:2] for c in range(3)]).astype(f32)
    clab = np.repeat(np.arange(3), 2).astype(np.int32)
    return x, lab, codes, clab
