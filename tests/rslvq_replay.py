"""CPU replay of batch Robust Soft LVQ (somhip_rslvq_train, K13) for tests/test_rslvq.py.  Plain numpy, written from the
definition in include/somhip_rslvq.h.

The squared distances are glvq_replay's float32 chains.  The posteriors are float64 with one numpy operation per rounding
in the order of the definition; the two normalisers are chains of float64 additions in row order from +0.0 (a loop over
the rows, vectorised over the samples).  exp and log are the C library's, within 1 ulp like the device's, so the device is
compared with this replay within the bounds DESIGN.md K13 derives (posterior_bounds).  The yardsticks of the sums and of
the update are np.longdouble."""
import math

import numpy as np

from glvq_replay import alpha_at, dist_sq, ulp32   # noqa: F401  (alpha_at: the same step 1)

f32, f64 = np.float32, np.float64
U = 2.0 ** -53                                   # the unit roundoff of float64
ULP = 2.0 ** -52                                 # 1 ulp as a relative error: what exp and log promise
SLACK = 1.001                                    # the second-order terms of every bound
TINY = 2.0 ** -1000                              # results in the subnormal range: exp's ulp is absolute there


def _exp(a):
    return np.array([math.exp(v) for v in a.ravel()], dtype=f64).reshape(a.shape)


def _log(a):
    return np.array([math.log(v) for v in a.ravel()], dtype=f64).reshape(a.shape)


def run_rows(n_rows, first, n):
    return (first + np.arange(n)) % n_rows


def keys(d, own):
    """(key_own, key_other) per sample: the smallest (distance bits << 32 | row) over each role's rows"""
    k = (np.ascontiguousarray(d).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(d.shape[1], dtype=np.uint64)[None, :]
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.where(own, k, none).min(axis=1), np.where(own, none, k).min(axis=1)


def posterior(codes, clab, data, dlab, sigma2, first=0, n=None, d=None):
    """Steps 2 and 3 as a dict: q [n][rows], cost, pown [n], correct int32[n], and what the bounds scale with: P, t (the own
    class's normalised terms, 0 elsewhere), z_all, z_own, la = m_all + log Z_all, lo = m_own + log Z_own"""
    rows = data.shape[0]
    n = rows if n is None else n
    r = run_rows(rows, first, n)
    d = dist_sq(codes, data)[r] if d is None else d
    own = np.asarray(clab)[None, :] == np.asarray(dlab)[r][:, None]
    assert own.any(axis=1).all() and (~own).any(axis=1).all()
    two_s = f64(2.0) * f64(f32(sigma2))
    g = (-d.astype(f64)) / two_s
    m_all = g.max(axis=1)
    m_own = np.where(own, g, -np.inf).max(axis=1)
    ea = _exp(g - m_all[:, None])
    eo = np.where(own, _exp(np.where(own, g - m_own[:, None], 0.0)), f64(0.0))
    z_all, z_own = np.zeros(n, dtype=f64), np.zeros(n, dtype=f64)
    for j in range(d.shape[1]):                  # ONE chain in row order, per sample
        z_all = z_all + ea[:, j]
        z_own = z_own + eo[:, j]                 # (+0.0 off the own class leaves the bits)
    P = ea / z_all[:, None]
    t = eo / z_own[:, None]
    q = np.where(own, t - P, -P)
    la, lo = m_all + _log(z_all), m_own + _log(z_own)
    cost = la - lo
    ko, kx = keys(d, own)
    return {"q": q, "cost": cost, "pown": _exp(-cost), "correct": (ko < kx).astype(np.int32), "P": P, "t": t, "own": own,
            "z_all": z_all, "z_own": z_own, "la": la, "lo": lo, "d": d}


PER_SAMPLE = ("q", "cost", "pown", "correct", "P", "t", "own", "z_all", "z_own", "la", "lo", "d")


def posterior_by_row(codes, clab, data, dlab, sigma2):
    """posterior() of every data row once: a sample's figures depend on its data row alone, so those of a run of any
    length are posterior_of_run of this"""
    return posterior(codes, clab, data, dlab, sigma2, 0, data.shape[0])


def posterior_of_run(by_row, first, n):
    """the dict posterior(..., first, n) returns, taken from posterior_by_row's: run sample s is data row (first + s) % rows"""
    r = run_rows(by_row["cost"].shape[0], first, n)
    return {key: by_row[key][r] for key in PER_SAMPLE}


def posterior_bounds(p):
    """(bound of q [n][rows], of cost [n], of pown [n], of sum_j q [n]) between two evaluations of the definition whose exp
    and log are each within 1 ulp.  R = the rows.
      an exponential:    the two sides differ by rho_e = 2 ULP of its value
      a normaliser:      a chain of R non-negative terms, each within rho_e, each addition rounded on both sides:
                         rho_z = rho_e + 2 R U
      P_j and t_j:       a quotient of the two, rounded on both sides: rho_p = rho_e + rho_z + 2 U
      q_j:               t_j - P_j, rounded on both sides: rho_p (t_j + P_j) + 2 U |q_j|
      m + log Z:         the argument within rho_z, so the logarithm within rho_z; its own ulp on both sides, 2 ULP log Z
                         (Z >= 1); the addition rounded on both sides, 2 U |m + log Z|
      cost:              the two of them, and the subtraction rounded on both sides, 2 U |cost|
      pown:              exp(-cost): pown (the cost's bound) + 2 ULP pown
      sum_j q_j:         sum_j t_j and sum_j P_j are each 1 within (R + 1) U (the chain, the quotients), every q_j rounds
                         once: 2 (R + 1) U + U sum |q_j|, which is at most 2 U"""
    R = p["q"].shape[1]
    rho_e = 2.0 * ULP
    rho_z = rho_e + 2.0 * R * U
    rho_p = rho_e + rho_z + 2.0 * U
    bq = (rho_p * (p["t"] + p["P"]) + 2.0 * U * np.abs(p["q"])) * SLACK + TINY
    bl = lambda z, l: rho_z + 2.0 * ULP * np.abs(_log(z)) + 2.0 * U * np.abs(l)
    bc = (bl(p["z_all"], p["la"]) + bl(p["z_own"], p["lo"]) + 2.0 * U * np.abs(p["cost"])) * SLACK
    bp = p["pown"] * (bc + 2.0 * ULP) * SLACK + TINY
    bs = np.full(p["q"].shape[0], (2.0 * (R + 1) + 2.0) * U * SLACK)
    return bq, bc, bp, bs


def sums_longdouble(q, data, first=0):
    """(G [rows][dim], c [rows], the bound of G, of c): Q^T [X | 1] in np.longdouble, and K8's combine bound with the samples
    as the inner dimension, (2 n + 16) 2^-52 sum_s |q| |x| per element"""
    ld = np.longdouble
    n = q.shape[0]
    x = data[run_rows(data.shape[0], first, n)].astype(ld)
    ql = q.astype(ld)
    G, c = ql.T @ x, ql.sum(axis=0)
    k = (2.0 * n + 16.0) * ULP
    return G, c, k * (np.abs(ql).T @ np.abs(x)).astype(f64) + TINY, k * np.abs(ql).sum(axis=0).astype(f64) + TINY


def sums_by_row_longdouble(q_rows, data, first, n):
    """sums_longdouble of the run (first, n) from one q row per data row (posterior_by_row's): every distinct row enters
    once, weighted by how often the run takes it -- the same sums and the same bound with the same n, without the
    [n][rows] array of a long run over a large codebook"""
    ld = np.longdouble
    w = np.bincount(run_rows(data.shape[0], first, n), minlength=data.shape[0]).astype(ld)
    x, ql = data.astype(ld), q_rows.astype(ld)
    qw, aw = ql * w[:, None], np.abs(ql) * w[:, None]
    G, c = qw.T @ x, qw.sum(axis=0)
    k = (2.0 * n + 16.0) * ULP
    return G, c, k * (aw.T @ np.abs(x)).astype(f64) + TINY, k * aw.sum(axis=0).astype(f64) + TINY


def sums_mfma(q, data, first=0):
    """[G | c] in float64 the way step 4 orders it, as far as numpy can follow: four consecutive samples form one exact sum
    of products (np.longdouble here; the instruction's own rounding inside a group of four is the hardware's), group after
    group into one float64 accumulator.  Not a bit-level yardstick: the tests hold the device to sums_longdouble's bound."""
    n = q.shape[0]
    x = np.concatenate([data[run_rows(data.shape[0], first, n)].astype(f64), np.ones((n, 1))], axis=1)
    acc = np.zeros((q.shape[1], x.shape[1]), dtype=f64)
    for s in range(0, n, 4):
        acc = (acc.astype(np.longdouble) + q[s:s + 4].astype(np.longdouble).T @ x[s:s + 4].astype(np.longdouble)).astype(f64)
    return acc[:, :-1], acc[:, -1]


def update(codes, G, c, alpha_t, sigma2, n):
    """step 5 in float64, one operation per rounding: the rows after it"""
    W = codes.astype(f64)
    a = f64(f32(alpha_t)) / (f64(f32(sigma2)) * f64(n))
    cw = c[:, None] * W
    gg = G - cw
    step = a * gg
    return (W + step).astype(f32)


def update_longdouble(codes, G, c, alpha_t, sigma2, n, bG=0.0, bc=0.0):
    """(q, bound): W + a (G - c W) in np.longdouble, and the allowance of a device row formed from sums within (bG, bc) of
    these: the rounding to float, the sums' bounds carried through a, and the float64 roundings of the update (the
    product, the difference and the step: at most 4 U on each magnitude, 2 U on the result)"""
    ld = np.longdouble
    W = codes.astype(ld)
    a = ld(f64(f32(alpha_t))) / (ld(f64(f32(sigma2))) * ld(n))
    Gl, cl = G.astype(ld), c.astype(ld)[:, None]
    q = W + a * (Gl - cl * W)
    mag = np.abs(Gl) + np.abs(cl * W)
    carried = bG + np.asarray(bc)[..., None] * np.abs(W) if np.ndim(bc) else bG + bc * np.abs(W)
    bound = ulp32(q.astype(f64)).astype(ld) / 2 + a * (carried + 4 * U * mag) + 2 * U * np.abs(q)
    return q, bound


def epoch(codes, clab, data, dlab, alpha_t, sigma2, first=0, n=None):
    """(the rows after one epoch, its cost, its correct count) with the sums in np.longdouble rounded to float64: the
    replay of whole runs, which the device follows within the stages' bounds"""
    n = data.shape[0] if n is None else n
    p = posterior(codes, clab, data, dlab, sigma2, first, n)
    G, c, _, _ = sums_longdouble(p["q"], data, first)
    chain = f64(0.0)
    for v in p["cost"]:
        chain = chain + v
    return update(codes, G.astype(f64), c.astype(f64), alpha_t, sigma2, n), chain / f64(n), int(p["correct"].sum())


def train(codes, clab, data, dlab, epochs, alpha, sigma2, first=0, n=None, start_epoch=0, count=None):
    """(rows, cost[count], correct[count]) of epochs [start_epoch, start_epoch + count)"""
    count = epochs - start_epoch if count is None else count
    cost, correct = np.zeros(count, dtype=f64), np.zeros(count, dtype=np.int64)
    for i in range(count):
        codes, cost[i], correct[i] = epoch(codes, clab, data, dlab, alpha_at(alpha, epochs, start_epoch + i), sigma2, first, n)
    return codes, cost, correct
