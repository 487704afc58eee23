"""CPU replay of batch GMLVQ (somhip_gmlvq_train, K12) for tests/test_gmlvq.py.  Plain numpy, on top of glvq_replay.

The projection is a float64 chain in dimension order: the product of two floats is exact in float64, so acc + o * z rounds
once, which is the device's fma.  The search, the terms and the sums are glvq_replay's, on the projected rows.  The update,
the gradient of Omega in blocks of BLOCK samples and Omega's step follow include/somhip.h operation by operation, one numpy
operation per rounding.  For the sigmoid the replay also returns what its comparison with the device scales with
(abs_grad)."""
import numpy as np

import glvq_replay as G
import grlvq_replay as R

f32, f64 = np.float32, np.float64
U = G.U
BLOCK = 4096                                     # GMLVQ_BLOCK: part of the definition


def default_omega(dim, rank=None):
    """(float)(1 / sqrt(dim)) where k % rank == r, else 0"""
    rank = dim if rank is None else rank
    om = np.zeros((rank, dim), dtype=f32)
    k = np.arange(dim)
    om[k % rank, k] = f32(1.0 / np.sqrt(f64(dim)))
    return om


def project(omega, rows):
    """y[z][r] = (float)(the chain from +0.0 over k of acc + (double)omega[r][k] * (double)rows[z][k])"""
    om, z = np.asarray(omega, dtype=f32).astype(f64), np.asarray(rows, dtype=f32).astype(f64)
    acc = np.zeros((z.shape[0], om.shape[0]), dtype=f64)
    for k in range(om.shape[1]):
        p = z[:, k][:, None] * om[:, k][None, :]          # exact
        acc = acc + p
    return acc.astype(f32)


def search(codes, clab, data, dlab, omega, first=0, n=None):
    """glvq_replay.search on the projected rows"""
    return G.search(project(omega, codes), clab, project(omega, data), dlab, first, n)


def omega_grad(codes, data, omega, iplus, iminus, xp, xm, first=0):
    """(Gm [m][dim], abs_grad [m][dim]): per block of BLOCK samples one chain per element in data order of
    + (xi+ u+[r]) t+[k], then - (xi- u-[r]) t-[k]; Gm the chain over the blocks.  abs_grad: the sum of |xi u t| of every
    term (what the sigmoid's bound scales with)."""
    rows = data.shape[0]
    V, Y = project(omega, codes).astype(f64), project(omega, data).astype(f64)
    W, X = codes.astype(f64), data.astype(f64)
    m, dim = np.asarray(omega).shape
    Gm, mag = np.zeros((m, dim), dtype=f64), np.zeros((m, dim), dtype=f64)
    n = len(iplus)
    for s0 in range(0, n, BLOCK):
        acc = np.zeros((m, dim), dtype=f64)
        for s in range(s0, min(n, s0 + BLOCK)):
            row = (first + s) % rows
            j, k = int(iplus[s]), int(iminus[s])
            up, um = Y[row] - V[j], Y[row] - V[k]
            tp, tm = X[row] - W[j], X[row] - W[k]
            a = xp[s] * up
            p = a[:, None] * tp[None, :]
            acc = acc + p
            c = xm[s] * um
            q = c[:, None] * tm[None, :]
            acc = acc - q
            mag += np.abs(p) + np.abs(q)
        Gm = Gm + acc
    return Gm, mag


def update(codes, S, omega, alpha_t, n):
    """step 6 in float64: the rows after it; rows no sample chose keep their bits"""
    W = codes.astype(f64)
    om = np.asarray(omega, dtype=f32).astype(f64)
    m, d = om.shape
    a = f64(f32(alpha_t)) / f64(n)
    Sp, sp = S["sums_plus"][:, :d], S["sums_plus"][:, d:]
    Sm, sm = S["sums_minus"][:, :d], S["sums_minus"][:, d:]
    pw, mw = sp * W, sm * W
    gp, gm = Sp - pw, Sm - mw
    g = gp - gm
    P = np.zeros((codes.shape[0], m), dtype=f64)
    for k in range(d):
        p = g[:, k][:, None] * om[:, k][None, :]
        P = P + p
    Dl = np.zeros((codes.shape[0], d), dtype=f64)
    for r in range(m):
        p = P[:, r][:, None] * om[r][None, :]
        Dl = Dl + p
    step = a * Dl
    new = (W + step).astype(f32)
    live = (S["n_plus"] > 0) | (S["n_minus"] > 0)
    out = codes.copy()
    out[live] = new[live]
    return out


def omega_step(omega, grad, eps_t, n):
    """step 8 in float64: omega after it (the array given where eps_t == 0 or the step lands on the zero matrix)"""
    omega = np.asarray(omega, dtype=f32)
    if not f32(eps_t) > 0:
        return omega.copy()
    e = f64(f32(eps_t)) / f64(n)
    step = e * np.asarray(grad, dtype=f64)
    O = omega.astype(f64) - step
    s = f64(0.0)
    for v in (O * O).reshape(-1):
        s = s + v
    if not s > 0:
        return omega.copy()
    return (O / np.sqrt(s)).astype(f32)


def epoch(codes, clab, data, dlab, omega, alpha_t, eps_t, beta=0.0, first=0, n=None):
    """(the rows after one epoch, omega after it, its cost, its correct count, the stage results)"""
    n = data.shape[0] if n is None else n
    dp, ip, dm, im = search(codes, clab, data, dlab, omega, first, n)
    xp, xm, f, correct = G.terms(dp, ip, dm, im, beta)
    S = G.sums(data, ip, im, xp, xm, f, codes.shape[0], first)
    S.update(xi_plus=xp, xi_minus=xm, f=f, correct=correct, iplus=ip, iminus=im)
    new_omega = np.asarray(omega, dtype=f32).copy()
    if f32(eps_t) > 0:
        S["grad"], S["abs_grad"] = omega_grad(codes, data, omega, ip, im, xp, xm, first)
        new_omega = omega_step(omega, S["grad"], eps_t, n)
    chain = f64(0.0)
    for c in S["cost"]:
        chain = chain + c
    return update(codes, S, omega, alpha_t, n), new_omega, chain / f64(n), correct, S


def train(codes, clab, data, dlab, omega, epochs, alpha, eps, beta=0.0, first=0, n=None, start_epoch=0, count=None):
    """(rows, omega, cost[count], correct[count]) of epochs [start_epoch, start_epoch + count)"""
    count = epochs - start_epoch if count is None else count
    omega = np.asarray(omega, dtype=f32).copy()
    cost, correct = np.zeros(count, dtype=f64), np.zeros(count, dtype=np.int64)
    for i in range(count):
        t = start_epoch + i
        codes, omega, cost[i], correct[i], _ = epoch(codes, clab, data, dlab, omega, R.rate_at(alpha, epochs, t), R.rate_at(eps, epochs, t),
                                                     beta, first, n)
    return codes, omega, cost, correct


def evaluate(codes, clab, data, dlab, omega, beta=0.0):
    """(cost, accuracy) of a codebook under omega: what an epoch reports of the state it starts from"""
    dp, ip, dm, im = search(codes, clab, data, dlab, omega)
    _, _, f, correct = G.terms(dp, ip, dm, im, beta)
    return float(f.sum()) / len(f), correct / len(f)


# ---- the sigmoid's bound -------------------------------------------------------------------------------
def grad_bound(abs_grad, beta, n):
    """|Gm_device - Gm_replay| <= this.  u and t are the same roundings on both sides; xi is within glvq_replay.xi_rel_bound
    of the replay's, the two products add U each on either side: a term is within (xi_rel_bound + 4 U) of its replay value,
    relative to |xi u t|.  The terms have mixed signs, so the chains' roundings are bounded on the magnitudes: 2 U per
    addition of a block chain (2 min(n, BLOCK) additions) and of the reduction over the blocks, on either side."""
    adds = 2 * min(n, BLOCK) + (n + BLOCK - 1) // BLOCK
    return (G.xi_rel_bound(beta) + 4.0 * U + 2.0 * adds * U) * abs_grad + np.finfo(f64).tiny


def learning_case(seed):
    """the issue's learning data: grlvq_replay.learning_case's rows multiplied by a fixed orthogonal matrix before the
    permutation, so that no single axis separates the classes; (x, labels, codes, code labels, Q)"""
    rs = np.random.RandomState(seed)
    means = np.zeros((3, 8))
    means[1, 0] = 3.0
    means[2, 1] = 3.0
    scale = np.array([1, 1, 3, 3, 3, 3, 3, 3], dtype=f64)
    x = np.concatenate([means[c] + rs.standard_normal((200, 8)) * scale for c in range(3)])
    Q = np.linalg.qr(np.random.RandomState(1234).standard_normal((8, 8)))[0]
    x = (x @ Q.T).astype(f32)
    lab = np.repeat(np.arange(3), 200).astype(np.int32)
    perm = rs.permutation(600)
    x, lab = x[perm], lab[perm]
    codes = np.concatenate([x[lab == c][:2] for c in range(3)]).astype(f32)
    clab = np.repeat(np.arange(3), 2).astype(np.int32)
    return x, lab, codes, clab, Q


def informative_share(omega, Q):
    """the share of trace(Omega^T Omega) in span(Q[:, :2])"""
    om = np.asarray(omega, dtype=f64)
    return float(((om @ Q[:, :2]) ** 2).sum() / (om ** 2).sum())
