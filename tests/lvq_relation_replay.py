"""Host replay of relation (*) of the exact batched LVQ engine (kernels/lvq_batch.hpp, K6) and of its components.

numpy only, never the GPU.  What the engine must find is stated twice:

  must[i, j]      the mathematical relation with no slack, in float64 over the components both samples have:
                  ||x_i - x_j|| <= (1 + amax) (R_i + R_j), R_j = sqrt of sample j's 8th frozen distance (+inf where the
                  list is not full or that distance is at or above FLT_MAX; everything where amax is unknown).  A pair
                  that is `must` and has no edge lets two workgroups stage the same code row.
  must_not[i, j]  the pair lies beyond everything the code documents as slack, so an edge there is parallelism thrown
                  away.  From the rho and the fp32 norms the engine returned:
                    direct form  D (1 - 2^-12) (1 - (d + 2) 2^-24) > rho_i + rho_j
                        the kernel tests sqrt(acc) (1 - 2^-12) <= rho_i + rho_j on an fp32 sum acc >= D^2 (1 - gamma_{d+2}),
                        and sqrt(1 - gamma_{d+2}) >= 1 - (d + 2) 2^-24;
                    Gram form    D^2 > (rho_i + rho_j)^2 (1 + 2^-10) + 16 (d + 8) 2^-24 (n_i + n_j)
                        the kernel's slack 8 (d + 8) u (n_i + n_j) plus its stated error bound (3 d + 16) u (n_i + n_j),
                        which is below that slack term.
                  Both constants are the ones in the comments and code of lvq_batch.hpp; the derivation there gives no other.

Between the two lies a band of about 2^-9 relative in which either answer is right.

The candidate keys are the reference's: fp32 (c - x)^2 summed over the dims in order (masked data: over the sample's own
components), key = distance bits << 32 | tag, tag = the row, or its complement under the k-NN tie rule of LVQ2.1 / LVQ3.
"""
import numpy as np

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FLT_MAX_BITS = 0x7F7FFFFF
FLT_MAX = float(np.finfo(np.float32).max)
K0 = 8                       # LVQ_K0: listed candidates per sample
BMAX, AW = 1024, 32          # LVQ_BMAX, LVQ_AW
U = 2.0 ** -24
LVQ1, OLVQ1, LVQ2, LVQ3 = 1, 2, 3, 4


# ---------------------------------------------------------------------------------------------- schedule, amax
def alpha_schedule(alpha_type, it0, count, length, alpha):
    """alpha_at (schedule.hpp) for iterations [it0, it0 + count): the reference's fp32 arithmetic"""
    f = np.float32
    it = np.arange(it0, it0 + count, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        if alpha_type == 2:
            c = f(length) / f(100.0)
            return ((f(alpha) * c) / (c + it.astype(np.float32))).astype(np.float32)
        return ((f(alpha) * (length - it).astype(np.float32)) / f(length)).astype(np.float32)


def amax_schedule(alphas, epsilon):
    """LVQ1 / LVQ2.1 / LVQ3: max(|alpha_t|, |alpha_t epsilon|) over the batch, fp32; None = unknown (a NaN)"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(alphas.astype(np.float32))
        ae = np.abs((alphas.astype(np.float32) * np.float32(epsilon)).astype(np.float32))
    if np.isnan(a).any() or np.isnan(ae).any():
        return None
    return np.float32(max(np.float32(0.0), a.max(), ae.max()))


def amax_olvq(keys, knn2, talpha, clamp):
    """OLVQ1: max(clamp, largest listed rate) if every listed rate and the clamp lie in [0, 1), else None"""
    listed = keys != KEY_NONE
    tag = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    row = (~tag if knn2 else tag).astype(np.int64)
    t = np.asarray(talpha, dtype=np.float32)[np.where(listed, row, 0)][listed]
    clamp = np.float32(clamp)
    if not (clamp >= 0 and clamp < 1) or not ((t >= 0) & (t < 1)).all():
        return None
    return np.float32(max(clamp, t.max() if t.size else np.float32(0.0)))


# ---------------------------------------------------------------------------------------------- candidate keys
def topk_keys(codes, xs, masks=None, knn2=False):
    """[m, 8] uint64: every sample's 8 smallest keys, ascending, KEY_NONE where the codebook has fewer rows"""
    codes = np.ascontiguousarray(codes, dtype=np.float32)
    xs = np.ascontiguousarray(xs, dtype=np.float32)
    m, n = xs.shape[0], codes.shape[0]
    acc = np.zeros((m, n), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(codes.shape[1]):
            t = codes[None, :, i] - xs[:, None, i]
            term = acc + t * t
            acc = term if masks is None else np.where(masks[:, None, i] != 0, acc, term)
    rows = np.arange(n, dtype=np.uint32)
    tag = (~rows if knn2 else rows).astype(np.uint64)
    keys = (acc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tag[None, :]
    keys = np.sort(keys, axis=1)[:, :K0]
    if n < K0:
        keys = np.concatenate([keys, np.full((m, K0 - n), KEY_NONE, dtype=np.uint64)], axis=1)
    return keys


def key_distance(keys):
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def radii(keys):
    """R_j = sqrt(float64(8th distance)); +inf where the list is not full or the 8th distance is at or above FLT_MAX"""
    k8 = keys[:, K0 - 1]
    bits = (k8 >> np.uint64(32)).astype(np.uint32)
    ok = (k8 != KEY_NONE) & (bits < FLT_MAX_BITS)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(bits.view(np.float32).astype(np.float64))
    return np.where(ok, r, np.inf)


# ---------------------------------------------------------------------------------------------- the relation
def _clean(xs, masks):
    x = np.asarray(xs, dtype=np.float64)
    if masks is None:
        return x, np.ones(x.shape, dtype=bool)
    w = np.asarray(masks) == 0
    return np.where(w, x, 0.0), w


def pair_distances(xs, masks=None):
    """[m, m] float64 ||x_i - x_j|| over the components both samples have (0 where they share none)"""
    x, w = _clean(xs, masks)
    m = x.shape[0]
    out = np.empty((m, m), dtype=np.float64)
    for s in range(0, m, 64):
        t = x[s:s + 64, None, :] - x[None, :, :]
        if masks is not None:
            t = np.where(w[s:s + 64, None, :] & w[None, :, :], t, 0.0)
        out[s:s + 64] = np.sqrt((t * t).sum(axis=2))
    return out


def own_norms(xs, masks=None):
    """float64 ||x_j||^2 over the sample's own components"""
    x, _ = _clean(xs, masks)
    return (x * x).sum(axis=1)


def must_pairs(D, R, amax):
    """the slack-free relation; the diagonal is not a pair"""
    m = D.shape[0]
    if amax is None:
        must = np.ones((m, m), dtype=bool)
    else:
        with np.errstate(invalid="ignore"):
            bound = (1.0 + float(amax)) * (R[:, None] + R[None, :])
        must = (D <= bound) | np.isinf(R)[:, None] | np.isinf(R)[None, :]
    must[np.arange(m), np.arange(m)] = False
    return must


def rho_value(R, amax, n32):
    """v of k_lvq_sample_rho in float64 from the fp32 norm the engine summed: rho is v rounded up to fp32"""
    if amax is None:
        return np.full(R.shape, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (1.0 + float(amax)) * R * (1.0 + 2.0 ** -10) + 2.0 ** -18 * (np.sqrt(1.001 * np.asarray(n32, dtype=np.float64)) + R)
    return np.where(np.isinf(R), np.inf, v)                # (the engine decides "+inf" before it looks at the norm)


def must_not_pairs(D, rho, n32, d, form):
    """beyond the documented slack (module docstring); form: 'direct' (also the masked kernel) or 'gram'"""
    rho = np.asarray(rho, dtype=np.float64)
    n = np.asarray(n32, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = rho[:, None] + rho[None, :]
        if form == "gram":
            out = D * D > r * r * (1.0 + 2.0 ** -10) + 16.0 * (d + 8) * U * (n[:, None] + n[None, :])
        else:
            out = D * (1.0 - 2.0 ** -12) * (1.0 - (d + 2) * U) > r
    out = out & np.isfinite(r)
    m = D.shape[0]
    out[np.arange(m), np.arange(m)] = False
    return out


def check_rho_band(rho, xnorm, R, amax, N64, d):
    """rho in [v, nextafter(float32(v))] with v from the returned norm; the norm within gamma_{d+6} of float64's"""
    rho = np.asarray(rho, dtype=np.float32)
    xnorm = np.asarray(xnorm, dtype=np.float32)
    g = (d + 6) * U / (1.0 - (d + 6) * U)
    x64 = xnorm.astype(np.float64)
    inside = np.abs(x64 - N64) <= g * N64
    over = N64 * (1.0 + g) > FLT_MAX                       # the fp32 sum may overflow ...
    sure = N64 * (1.0 - g) > FLT_MAX                       # ... or must
    ok = np.where(sure, np.isposinf(x64), inside | (over & np.isposinf(x64)))
    ok = np.where(np.isnan(N64), np.isnan(x64), ok)        # a NaN among the sample's own values
    assert ok.all(), ("xnorm outside gamma_{d+6}", np.flatnonzero(~ok)[:8], xnorm[~ok][:8], N64[~ok][:8])
    v = rho_value(R, amax, xnorm)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.nextafter(v.astype(np.float32), np.float32(np.inf))
    r64 = rho.astype(np.float64)
    low = r64 >= v
    up = rho <= hi
    assert low.all(), ("rho below its formula", np.flatnonzero(~low)[:8], rho[~low][:8], v[~low][:8])
    assert up.all(), ("rho more than one step above its formula", np.flatnonzero(~up)[:8], rho[~up][:8], v[~up][:8])


# ---------------------------------------------------------------------------------------------- adjacency, components
def unpack_adj(adj, count):
    """[count, count] bool from the bit rows [count, 32] (bit i % 32 of word i / 32 of row j)"""
    a = np.ascontiguousarray(adj, dtype=np.uint32).reshape(count, AW)
    bits = (a[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(count, AW * 32)[:, :count].astype(bool)


def pack_adj(A):
    """the bit rows [count, 32] of a bool matrix"""
    count = A.shape[0]
    full = np.zeros((count, AW * 32), dtype=np.uint32)
    full[:, :count] = A
    return (full.reshape(count, AW, 32) << np.arange(32, dtype=np.uint32)[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def host_components(A):
    """(ncomp, start, comp_samples) of a symmetric bool adjacency by a host union-find (quick-find: labels[] holds every
    sample's root, a union relabels): a component's root is its smallest sample; components by size descending, then
    root ascending; start = exclusive prefix sums of the sizes; inside a component the samples ascend"""
    count = A.shape[0]
    labels = np.arange(count, dtype=np.int64)
    for j in range(count):
        nb = np.flatnonzero(A[j, :j])
        if nb.size == 0:
            continue
        roots = np.unique(np.append(labels[nb], labels[j]))
        if roots.size > 1:
            labels[np.isin(labels, roots)] = roots[0]
    roots, sizes = np.unique(labels, return_counts=True)
    order = np.lexsort((roots, -sizes))
    start = np.concatenate([[0], np.cumsum(sizes[order])]).astype(np.int32)
    comp = np.concatenate([np.flatnonzero(labels == roots[o]) for o in order]).astype(np.int32)
    return int(roots.size), start, comp


# ---------------------------------------------------------------------------------------------- the checkers
def check_sound(A, must):
    miss = must & ~A
    assert not miss.any(), "%d of %d must pairs have no edge; first %s" % (miss.sum() // 2, must.sum() // 2, np.argwhere(miss)[:4].tolist())


def check_tight(A, must_not):
    extra = must_not & A
    assert not extra.any(), "%d of %d separable pairs have an edge; first %s" % (extra.sum() // 2, must_not.sum() // 2, np.argwhere(extra)[:4].tolist())


def check_layout(adj, count):
    """symmetric, clear diagonal, no bit at or above count in the first ceil(count / 32) words, nothing in the others"""
    a = np.ascontiguousarray(adj, dtype=np.uint32).reshape(count, AW)
    A = unpack_adj(a, count)
    assert np.array_equal(A, A.T), ("adjacency not symmetric", np.argwhere(A != A.T)[:4].tolist())
    assert not A[np.arange(count), np.arange(count)].any(), "a sample is related to itself"
    assert np.array_equal(pack_adj(A), a), "bits at or above count are set"


def check_components(A, ncomp, start, comp_samples):
    """exactly host_components(A)"""
    wn, ws, wc = host_components(A)
    assert ncomp == wn, ("component count", ncomp, wn)
    start = np.asarray(start)
    assert start.shape == ws.shape and np.array_equal(start, ws), (
        "start", np.flatnonzero(start != ws)[:8] if start.shape == ws.shape else start.shape, start[-4:], ws[-4:])
    comp_samples = np.asarray(comp_samples)
    assert np.array_equal(np.sort(comp_samples), np.arange(A.shape[0])), "comp_samples is not a permutation"
    assert np.array_equal(comp_samples, wc), ("comp_samples", np.flatnonzero(comp_samples != wc)[:8])
