"""numpy restatement of SOM_PAK's sammon (sammon.c:84-242), bit for bit: the witness the GPU tests compare against.

Every operation below carries the type C gives it in the reference (float = np.float32, double = np.float64, each
operation rounded on its own; the reference is built with -ffp-contract=off):

    xd = x[j] - x[k]; yd = y[j] - y[k]                                float
    dpj = (float) sqrt((double)xd * (double)xd + (double)(float)(yd * yd))
    dt = dd(j, k); dq = dt - dpj; dr = dt * dpj                       float
    e1x = (float)(e1x + (float)((float)(xd * dq) / dr))               float chain
    t   = (double)dq - ((double)(float)(xd * xd) * (1.0 + (double)(float)(dq / dpj))) / (double)dpj
    e2x = (float)((double)e2x + t / (double)dr)                       double term, float running sum
    xu[j] = (float)((double)x[j] + (0.2 * (double)e1x) / fabs((double)e2x))
    xx = float sum of xu[] in order; xx = xx / (float)noc; x[j] = xu[j] - xx

The terms of all (j, k) are formed at once (they are independent); only the four running sums walk k in order, one
vector operation over j per k.  tests/test_sammon.py checks this file against outputs of the real reference
(tests/golden/sammon, written by tests/golden/make_golden_sammon.py), so the table above is pinned by the reference.

Also here: orand (lvq_pak.c:459-484) for the initial table, the list walk of remove_identicals with the reference's
way of counting `ij`, and the generators of the test inputs that are not stored as fixtures.
"""
import os

import numpy as np

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------ random numbers, initial table
def orand_stream(seed, count):
    """the next `count` values of orand() after init_random(seed) (seed != 0)"""
    out = np.empty(count, dtype=np.int64)
    nxt = int(seed)
    for i in range(count):
        nxt = (nxt * 23) % 100000001
        out[i] = nxt % 32767
    return out


def initial_table(noc, seed):
    """x[i] = (float)(orand() % noc) / noc, y[i] = (float) i / noc (sammon.c:164-167)"""
    r = orand_stream(seed, noc) % noc
    x = r.astype(f32) / f32(noc)
    y = np.arange(noc).astype(f32) / f32(noc)
    return x, y


# ------------------------------------------------------------------ distances (vector_dist_euc, lvq_pak.c:291-316)
def distances(rows):
    """D[j, k] = (float) sqrt((double) sum_i (a_i - b_i)^2), the sum in fp32 in the order of i"""
    rows = np.ascontiguousarray(rows, dtype=f32)
    n, dim = rows.shape
    acc = np.zeros((n, n), dtype=f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(dim):
            c = rows[:, i]
            diff = c[:, None] - c[None, :]
            acc = acc + diff * diff
        return np.sqrt(acc.astype(f64)).astype(f32)


def zero_pairs(D):
    """the pairs i < j with dd == 0, ordered"""
    i, j = np.nonzero(np.triu(D == 0, 1))
    return np.stack([i, j], axis=1).astype(np.int64)


def remove_identicals(D):
    """remove_identicals (sammon.c:84-128) on the distance table of the rows as read: the surviving row indices and the
    stderr text.  The reference's counters: ii counts the outer entries from 1, ij starts at ii + 1 and advances by
    two after a removal (sammon.c:115), by one otherwise."""
    alive = list(range(D.shape[0]))
    msgs = []
    pos, ii = 0, 1
    while pos < len(alive):
        i = alive[pos]
        ij = ii + 1
        q = pos + 1
        while q < len(alive):
            if D[i, alive[q]] == 0:
                msgs.append("Identical entries in codebook (entries %d, %d), removing one.\n" % (ii, ij))
                del alive[q]
                ij += 2
            else:
                q += 1
                ij += 1
        pos += 1
        ii += 1
    return np.array(alive, dtype=np.int64), "".join(msgs)


# ------------------------------------------------------------------ the iteration
def _ordered_sum(v):
    return np.cumsum(np.concatenate([np.zeros(1, f32), v]), dtype=f32)[-1]


def sweep(x, y, D):
    """one iteration of sammon.c:188-225: the new centred x, y"""
    n = x.shape[0]
    with np.errstate(all="ignore"):
        xd = x[:, None] - x[None, :]                     # [j, k]
        yd = y[:, None] - y[None, :]
        dpj = np.sqrt(xd.astype(f64) * xd.astype(f64) + (yd * yd).astype(f64)).astype(f32)
        dq = D - dpj
        dr = D * dpj
        drd = dr.astype(f64)
        dpd = dpj.astype(f64)
        fac = 1.0 + (dq / dpj).astype(f64)
        terms = [(xd * dq) / dr, (yd * dq) / dr,
                 (dq.astype(f64) - ((xd * xd).astype(f64) * fac) / dpd) / drd,
                 (dq.astype(f64) - ((yd * yd).astype(f64) * fac) / dpd) / drd]
        # k == j is skipped by the reference; adding +0.0 is the same (the sums start at +0.0 and can never be -0.0)
        terms = [np.ascontiguousarray(t.T) for t in terms]     # [k, j]
        for t in terms:
            np.fill_diagonal(t, 0.0)
        e1x = np.zeros(n, f32); e1y = np.zeros(n, f32); e2x = np.zeros(n, f32); e2y = np.zeros(n, f32)
        for k in range(n):
            e1x = e1x + terms[0][k]
            e1y = e1y + terms[1][k]
            e2x = (e2x.astype(f64) + terms[2][k]).astype(f32)
            e2y = (e2y.astype(f64) + terms[3][k]).astype(f32)
        xu = (x.astype(f64) + (0.2 * e1x.astype(f64)) / np.abs(e2x.astype(f64))).astype(f32)
        yu = (y.astype(f64) + (0.2 * e1y.astype(f64)) / np.abs(e2y.astype(f64))).astype(f32)
        xx = _ordered_sum(xu) / f32(n)
        yy = _ordered_sum(yu) / f32(n)
        return xu - xx, yu - yy


def mapping_error(x, y, D):
    """the reference's own number (sammon.c:227-240): fp32 sums in the order j = 1.., k < j"""
    n = x.shape[0]
    j, k = np.nonzero(np.tril(np.ones((n, n), dtype=bool), -1))      # row-major: j ascending, k < j ascending
    with np.errstate(all="ignore"):
        d = D[j, k]
        xd = x[j] - x[k]
        yd = y[j] - y[k]
        ee = d - np.sqrt(xd.astype(f64) * xd.astype(f64) + (yd * yd).astype(f64)).astype(f32)
        return _ordered_sum(ee * ee / d) / _ordered_sum(d)


def iterate(x, y, D, rlen, snapshots=(), errors=False):
    """rlen sweeps from (x, y); returns x, y (and {iteration: (x, y)} for the iterations in `snapshots`, and the
    mapping error after every sweep if asked for)"""
    x = np.ascontiguousarray(x, dtype=f32).copy()
    y = np.ascontiguousarray(y, dtype=f32).copy()
    snap, err = {}, []
    if 0 in snapshots:
        snap[0] = (x.copy(), y.copy())
    for it in range(1, rlen + 1):
        x, y = sweep(x, y, D)
        if errors:
            err.append(mapping_error(x, y, D))
        if it in snapshots:
            snap[it] = (x.copy(), y.copy())
    out = (x, y)
    if snapshots:
        out += (snap,)
    if errors:
        out += (np.array(err, dtype=f32),)
    return out


def sammon(rows, seed, rlen, errors=False):
    """the whole program on the rows of a codebook: (survivors, stderr text, x, y[, errors])"""
    D = distances(rows)
    alive, msgs = remove_identicals(D)
    D = np.ascontiguousarray(D[np.ix_(alive, alive)])
    x, y = initial_table(len(alive), seed)
    return (alive, msgs) + iterate(x, y, D, rlen, errors=errors)


# ------------------------------------------------------------------ inputs that are generated, not stored
def fmt_cod_rows(points, labels=None):
    out = []
    for r in range(points.shape[0]):
        line = "".join("%g " % float(v) for v in points[r])
        if labels is not None and labels[r]:
            line += labels[r] + " "
        out.append(line)
    return out


def write_seeded_map(path, xdim=35, ydim=31, dim=16, seed=4242):
    """a smooth seeded rect map, as text: 1085 rows by default (not a multiple of 64)"""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal((2, dim)).astype(f32)
    gx, gy = np.meshgrid(np.arange(xdim, dtype=f32), np.arange(ydim, dtype=f32))
    pts = (gx.reshape(-1, 1) * a[0] + gy.reshape(-1, 1) * a[1]).astype(f32)
    pts = (pts + f32(0.3) * rs.standard_normal(pts.shape).astype(f32)).astype(f32)
    with open(path, "w") as f:
        f.write("%d rect %d %d bubble\n" % (dim, xdim, ydim))
        f.write("\n".join(fmt_cod_rows(pts)) + "\n")


def write_duplicated_map(path, src):
    """the map `src` with row 40 and 41 repeated after row 41 and row 3 repeated twice at the end (100 rows under the
    header of a 96-unit map): removals next to each other, far apart and twice for one row"""
    lines = open(src).read().split("\n")
    head, rows = lines[0], [ln for ln in lines[1:] if ln.strip()]
    rows = rows[:42] + [rows[40], rows[41]] + rows[42:] + [rows[3], rows[3]]
    with open(path, "w") as f:
        f.write(head + "\n" + "\n".join(rows) + "\n")


GENERATED = {"seeded_35x31x16.cod": lambda path, cli: write_seeded_map(path),
             "som_hexa_gaussian_dup.cod": lambda path, cli: write_duplicated_map(path, os.path.join(cli, "som_hexa_gaussian.cod"))}


def write_generated(dst, cli):
    """every generated input into directory dst (cli = tests/golden/cli)"""
    for name, make in GENERATED.items():
        make(os.path.join(dst, name), cli)
