"""CPU replay of the batch map over data with missing values (somhip_som_batchmap_missing, K8m) for
tests/test_batchmap_missing.py, on top of batchmap_replay.py (the lattice, the weights, ulp32 and radius_at are its own).

The winners are the oracle's find_winner_euc under the sample's mask (the lowest index on equal distances); a sample with
every component masked has none.  The per-unit sums are loops of np.float64 additions in data order from +0.0 that skip a
masked component -- its stored value is never added -- and count the known ones per component.  The combine is formed in
np.longdouble per component, together with the bound its fp64 evaluation has to meet."""
import numpy as np

from batchmap_replay import f32, f64, radius_at, ulp32, weights   # noqa: F401  (re-exported for the tests)

NONE = -1


def winners(oracle, codes, data, mask):
    """(winner, squared distance) of every data row under its mask; NONE for a row with every component masked"""
    clean = np.where(mask != 0, f32(0.0), data) if mask is not None else data      # (a masked value is never read; keep NaNs out)
    idx, diff, ret = oracle.winners(np.ascontiguousarray(codes, dtype=f32), np.ascontiguousarray(clean, dtype=f32), 1, False, mask)
    win = idx[:, 0].astype(np.int64)
    if mask is not None:
        win = np.where((mask != 0).all(axis=1), NONE, win)
    assert (win[win != NONE] >= 0).all()
    return win, diff[:, 0].copy()


def sums(win, data, mask, n_units, first=0, n=None):
    """S[u][k] and C[u][k] over data rows (first + s) % len(data), s < n: per unit and component one chain of fp64
    additions in data order from +0.0 over the samples that know the component, and their number"""
    rows, dim = data.shape
    n = rows if n is None else n
    S = np.zeros((n_units, dim), dtype=f64)
    Cn = np.zeros((n_units, dim), dtype=f64)
    x = data.astype(f64)
    for s in range(n):
        r = (first + s) % rows
        u = int(win[r])
        if u == NONE:
            continue
        if mask is None:
            S[u] = S[u] + x[r]
            Cn[u] += 1.0
        else:
            known = mask[r] == 0
            S[u][known] = S[u][known] + x[r][known]          # the masked components' values are not touched
            Cn[u][known] += 1.0
    return S, Cn


def qerror_chain(d1, win, first=0, n=None):
    """find_qerror's float over the samples that have a winner (som_rout.c:712-715), in data order"""
    rows = len(d1)
    n = rows if n is None else n
    q = f32(0.0)
    for s in range(n):
        r = (first + s) % rows
        if win[r] != NONE:
            q = f32(f64(q) + np.sqrt(f64(d1[r])))
    return q


def combine(h, S, Cn):
    """(q, D, bound): q = N / D in np.longdouble where D > 0, per component, and the allowance
    ulp32(q) / 2 + (4 * units + 16) * 2^-52 * A / D with A[i][k] = sum_j h |S[j][k]|: at most two roundings per term (the
    FMA and the weight) in each of N and D -- D's relative error acts on |q| <= A / D -- and 16 for the division and slack"""
    ld = np.longdouble
    units = h.shape[0]
    hl = h.astype(ld)
    N = hl @ S.astype(ld)
    A = hl @ np.abs(S).astype(ld)
    D = hl @ Cn.astype(ld)
    live = D > 0
    Ds = np.where(live, D, 1)
    q = N / Ds
    bound = ulp32(q.astype(f64)).astype(ld) / 2 + ld(4 * units + 16) * ld(2.0) ** -52 * A / Ds
    return q, D, bound
