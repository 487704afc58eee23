"""LVQ training replayed one iteration at a time from the oracle's primitives, with the sample's mask.

oracle.lvq_train has no mask argument (the reference's training loops take none apart from what find_winner_* and
adapt_vector do with the sample's own mask, lvq_pak.c:179-186 and :343-347).  This module restates the four loops of
lvq_rout.c around those primitives -- oracle.winners for one sample, oracle.adapt_vector, oracle.alpha -- with every
scalar of the rules in fp32 and in the order of operations kernels/lvq.hpp cites:

  LVQ1    lvq_rout.c:542-555   the winner moves by +alpha(t) if its label is the sample's, else by -alpha(t)
  OLVQ1   lvq_rout.c:650-673   ... by its own rate a, which becomes a / (1 + a) or min(a / (1 - a), alpha)
  LVQ2.1  lvq_rout.c:750-783   two nearest of different labels, one of them the sample's, d0 / d1 > (1 - w) / (1 + w)
                                on the squared distances: the right one by +alpha(t), the other by -alpha(t)
  LVQ3    lvq_rout.c:855-896   the same, and both by alpha(t) * epsilon where both carry the sample's label

Unmasked it must equal oracle.lvq_train bit for bit (tests/test_online_stream.py checks that on the CPU); masked it
is the witness of the masked k_lvq_online_step runs.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

F = np.float32


def lvq_replay(oracle, kind, codes, clabels, data, dlabels, length, alpha, alpha_type=1, winlen=0.0, epsilon=0.0,
               talpha=None, mask=None, start_iter=0, count=None):
    """(codes, talpha, trace_index, trace_diff) as oracle.lvq_train returns them; iterations [start_iter, start_iter +
    count) of a schedule of `length` on data rows start_iter, start_iter + 1, ... (mod the rows)."""
    codes = np.ascontiguousarray(codes, dtype=np.float32).copy()
    data = np.ascontiguousarray(data, dtype=np.float32)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    n, m = codes.shape[0], data.shape[0]
    count = length - start_iter if count is None else count
    knn = 2 if kind in (3, 4) else 1
    if kind == 2:
        talpha = np.full(n, alpha, dtype=np.float32) if talpha is None else np.asarray(talpha, dtype=np.float32).copy()
    one = F(1)
    ratio = (one - F(winlen)) / (one + F(winlen))                    # lvq_rout.c:770, fp32
    ti = np.zeros(count * knn, dtype=np.int64)
    td = np.zeros(count * knn, dtype=np.float32)

    def adapt(k, x, mk, a):
        codes[k] = oracle.adapt_vector(codes[k], x, float(a), mask=mk)

    for j in range(count):
        le = start_iter + j
        row = le % m
        x = data[row]
        mk = None if mask is None else mask[row]
        want = dlabels[row]
        idx, dist, ret = oracle.winners(codes, data[row:row + 1], knn=knn, use_knn_fn=knn == 2,
                                        mask=None if mask is None else mask[row:row + 1])
        idx, dist = idx[0], dist[0]
        ti[j * knn:(j + 1) * knn] = idx
        td[j * knn:(j + 1) * knn] = dist
        if not ret[0] or (idx < 0).any():
            raise FloatingPointError("iteration %d has no winner" % le)
        a = F(oracle.alpha(alpha_type, le, length, alpha))
        if kind == 1:
            adapt(idx[0], x, mk, a if clabels[idx[0]] == want else -a)
        elif kind == 2:
            k = idx[0]
            ta = talpha[k]
            if clabels[k] == want:
                adapt(k, x, mk, ta)
                talpha[k] = ta / (one + ta)
            else:
                adapt(k, x, mk, -ta)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ta = ta / (one - ta)
                talpha[k] = F(alpha) if ta > F(alpha) else ta
        else:
            first, second = idx[0], idx[1]
            l1, l2 = clabels[first], clabels[second]
            if l1 != l2:
                if l1 == want or l2 == want:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        inside = (dist[0] / dist[1]) > ratio
                    if inside:
                        if l2 == want:
                            first, second = second, first
                        adapt(first, x, mk, a)
                        adapt(second, x, mk, -a)
            elif kind == 4 and l1 == want:
                ae = a * F(epsilon)
                adapt(first, x, mk, ae)
                adapt(second, x, mk, ae)
    return codes, talpha, ti, td
