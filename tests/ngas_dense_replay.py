"""CPU replay of dense batch neural gas (somhip_ng_train_dense, K10d) for tests/test_ngas_dense.py: the definition in
include/somhip_ng_dense.h, on top of ngas_replay.py, which stays as it is.

The ranks are restated at bit level -- lexsort((-rows, d)) inverted: rank[s][j] is the number of rows before row j in
the order (distance ascending, the later row first among equal distances).  The sums have no bit-level yardstick (the
fp64 MFMA adds four samples a step with fused multiply-adds): the epoch is built on ngas_replay.dense_longdouble, and the
bound of a comparison comes from rslvq_replay.sums_longdouble, which derives it for k_rslvq_sums with the samples as
the inner dimension.  The weights come from the caller (engine.ng_dense_schedule: the library's own host arithmetic), so
no libm difference enters a comparison."""
import numpy as np

import ngas_replay as R
import rslvq_replay as RS

f32, f64 = np.float32, np.float64
FLT_MAX = R.FLT_MAX


def ranks(codes, x):
    """(rank int32[n, units], d float32[n, units]): per sample and row the number of rows before it, and its distance"""
    d = R.distances(codes, x)
    n, units = d.shape
    rows = np.broadcast_to(np.arange(units), d.shape)
    order = np.lexsort((-rows, d), axis=1)
    rank = np.empty(d.shape, dtype=np.int32)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(units, dtype=np.int32), d.shape), axis=1)
    return rank, d


def weights_matrix(codes, x, w):
    """Q float64[n, units] = w[rank], +0.0 where the distance is not below FLT_MAX"""
    rank, d = ranks(codes, x)
    q = np.asarray(w, dtype=f64)[rank]
    q[~(d < FLT_MAX)] = 0.0
    return q


def sums_bound(codes, data, w, first=0, n=None):
    """(S, W in np.longdouble, the bound of S, of W) of the run (first, n): Q^T [X | 1] and k_rslvq_sums's bound"""
    n = data.shape[0] if n is None else n
    q = weights_matrix(codes, R.rows_of(data, first, n), w)
    return RS.sums_longdouble(q, np.ascontiguousarray(data, dtype=f32), first)


def epoch(codes, data, w, first=0, n=None):
    """one dense epoch with the weights w[units]: (S / W in np.longdouble where W > 0, S, W, A = sum w |x|, the q chain of
    the codebook before it) -- ngas_replay.dense_longdouble is the yardstick"""
    n = data.shape[0] if n is None else n
    x = R.rows_of(data, first, n)
    q, S, W, A = R.dense_longdouble(codes, x, w)
    d0 = R.distances(codes, x).min(axis=1)
    return q, S, W, A, R.qerror_chain(d0)


def update(codes, S, W):
    """the rows after the epoch: float32 of the np.longdouble quotient where W > 0 (the yardstick's rows, not the device's bits)"""
    out = np.array(codes, dtype=f32, copy=True)
    live = np.asarray(W > 0)
    out[live] = (S[live] / W[live][:, None]).astype(f64).astype(f32)
    return out


def train(codes, data, schedule, epochs, truncate=None):
    """`epochs` epochs in the replay; schedule(t) -> w[units].  truncate K: the weights behind rank K - 1 are dropped (K10's
    truncation, in the same arithmetic, for the comparison of behaviour).  Returns the rows."""
    rows = np.array(codes, dtype=f32, copy=True)
    for t in range(epochs):
        w = np.array(schedule(t), dtype=f64, copy=True)
        if truncate is not None:
            w[truncate:] = 0.0
        _, S, W, _, _ = epoch(rows, data, w)
        rows = update(rows, S, W)
    return rows
