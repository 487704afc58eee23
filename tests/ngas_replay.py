"""CPU replay of batch neural gas (somhip_ng_train, K10) for tests/test_ngas.py: the definition in include/somhip.h, literally.

Distances are float32 sums of (c - x)^2 in dimension order, a rounding after the subtraction, the multiplication and the
addition; ranks sort by (distance ascending, row descending) -- find_winner_knn's order of equal distances; the sums are
loops of np.float64 in data order, per entry a multiplication and then an addition, from +0.0; the q chain is
find_qerror's float.  lambda_t, K_t and the weights come from the caller (engine.ng_schedule: the library's own host
arithmetic), so no libm difference enters a comparison."""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = np.finfo(f32).max


def distances(codes, x):
    """d[s][j] = find_winner_euc's squared distance of sample s to row j, float32"""
    codes, x = np.ascontiguousarray(codes, dtype=f32), np.ascontiguousarray(x, dtype=f32)
    acc = np.zeros((x.shape[0], codes.shape[0]), dtype=f32)
    for k in range(codes.shape[1]):
        diff = codes[None, :, k] - x[:, None, k]
        acc = acc + diff * diff
    assert acc.dtype == f32
    return acc


def ranks(codes, x, K):
    """(units int32[n, K], dist float32[n, K]): the K nearest rows of every sample, nearest first, the later row first among
    equal distances; -1 / -1.0 where the codebook has no such row below FLT_MAX"""
    d = distances(codes, x)
    n, units = d.shape
    rows = np.broadcast_to(np.arange(units), d.shape)
    order = np.lexsort((-rows, d), axis=1)                  # last key first: distance, then the row descending
    u = np.full((n, K), -1, dtype=np.int32)
    dist = np.full((n, K), -1.0, dtype=f32)
    k = min(K, units)
    u[:, :k] = order[:, :k]
    dist[:, :k] = np.take_along_axis(d, order[:, :k], axis=1)
    dead = ~(dist < FLT_MAX) | (u < 0)
    u[dead], dist[dead] = -1, -1.0
    return u, dist


def sums(rank_units, x, w, n_units):
    """(hits uint32[n_units], S float64[n_units, dim], W float64[n_units]) from rank_units[n, K] (sample s is x[s]) and the
    weights w[K]: per unit one chain in data order of w[r] * (double)x -- a multiply, then an add -- and of w[r]"""
    n, K = rank_units.shape
    w = np.asarray(w, dtype=f64)
    assert w.shape == (K,)
    hits = np.zeros(n_units, dtype=np.uint32)
    S = np.zeros((n_units, x.shape[1]), dtype=f64)
    W = np.zeros(n_units, dtype=f64)
    xd = np.ascontiguousarray(x, dtype=f32).astype(f64)
    for s in range(n):
        live = rank_units[s] >= 0
        u = rank_units[s][live]                             # distinct units: the chains of one sample are independent
        prod = w[live][:, None] * xd[s][None, :]
        S[u] = S[u] + prod
        W[u] = W[u] + w[live]
        hits[u] += 1
    return hits, S, W


def update(codes, S, W):
    """m_j = (float)(S[j] / W[j]) where W[j] > 0; the other rows keep their bits"""
    out = np.array(codes, dtype=f32, copy=True)
    live = W > 0
    out[live] = (S[live] / W[live][:, None]).astype(f32)
    return out


def qerror_chain(d0):
    """find_qerror's float: qerror += sqrt((double) diff) on a float accumulator, in data order"""
    q = f32(0.0)
    for d in d0:
        q = f32(f64(q) + np.sqrt(f64(d)))
    return q


def rows_of(data, first, n):
    return np.ascontiguousarray(data[(first + np.arange(n)) % data.shape[0]], dtype=f32)


def epoch(codes, data, K, w, first=0, n=None):
    """one epoch with K ranks and weights w[K] over data rows (first + s) % len(data): (the codebook after it, the q chain
    of the codebook before it, hits)"""
    n = data.shape[0] if n is None else n
    x = rows_of(data, first, n)
    u, dist = ranks(codes, x, 2 if K == 1 and codes.shape[0] >= 2 else K)
    u, dist = u[:, :K], dist[:, :K]
    hits, S, W = sums(u, x, w, codes.shape[0])
    return update(codes, S, W), qerror_chain(dist[:, 0]), hits


def train(codes, data, schedule, epochs, start_epoch=0, count=None, first=0, n=None):
    """epochs [start_epoch, start_epoch + count) of a run of `epochs`; schedule(t) -> (lambda_t, K_t, w).  Returns (rows,
    q float32[count])"""
    count = epochs - start_epoch if count is None else count
    rows = np.array(codes, dtype=f32, copy=True)
    q = np.zeros(count, dtype=f32)
    for i in range(count):
        _, K, w = schedule(start_epoch + i)
        rows, q[i], _ = epoch(rows, data, K, w, first, n)
    return rows, q


def dense_longdouble(codes, x, w):
    """The dense form of steps 2-4 in np.longdouble, every unit fed by every sample: (q = S / W, S, W, A = sum w |x|) with
    the weight w[rank] (0 beyond len(w)).  What the chains approximate."""
    ld = np.longdouble
    d = distances(codes, x)
    n, units = d.shape
    rows = np.broadcast_to(np.arange(units), d.shape)
    order = np.lexsort((-rows, d), axis=1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(units), d.shape), axis=1)
    wl = np.zeros(units, dtype=ld)
    wl[:min(len(w), units)] = np.asarray(w, dtype=ld)[:units]
    h = wl[rank]                                            # h[s][j]
    xl = np.asarray(x, dtype=f32).astype(ld)
    S, A, W = h.T @ xl, h.T @ np.abs(xl), h.sum(axis=0)
    return S / np.where(W > 0, W, 1)[:, None], S, W, A
