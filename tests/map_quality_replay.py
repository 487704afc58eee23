"""CPU replay of somhip_map_quality (K1q) on the oracle binding and numpy.

b1 is the oracle's find_winner_euc; b2 the same function on the codebook with row b1 taken out, its index mapped back;
adjacency is the reference's hexa_dist / rect_dist arithmetic before the square root (som_rout.c:434-468), float by float
and double by double; the qsum chain is a loop of np.float64 additions in data order and the qerror chain the reference's
`qerror += sqrt((double) diff)` on a float (som_rout.c:715)."""
import numpy as np

TOPOL_HEXA, TOPOL_RECT = 3, 4


def lattice_sq(topol, bx, by, tx, ty):
    """the squared lattice distance as hexa_dist / rect_dist form it: a float32"""
    diff = np.float32(bx - tx)
    if topol == TOPOL_RECT:
        ret = np.float32(diff * diff)
        diff = np.float32(by - ty)
        return np.float32(ret + np.float32(diff * diff))
    if (by - ty) % 2 != 0:
        diff = np.float32(np.float64(diff) - 0.5) if by % 2 == 0 else np.float32(np.float64(diff) + 0.5)
    ret = np.float32(diff * diff)
    diff = np.float32(by - ty)
    return np.float32(np.float64(ret) + np.float64(0.75) * np.float64(diff) * np.float64(diff))


def adjacent(topol, xdim, u1, u2):
    return bool(lattice_sq(topol, u1 % xdim, u1 // xdim, u2 % xdim, u2 // xdim) <= np.float32(1.0))


def pairs(oracle, codes, data, mask=None):
    """per data row: (b1, d1, b2, searched) -- b1 / b2 are -1 where there is none"""
    codes = np.ascontiguousarray(codes, dtype=np.float32)
    data = np.ascontiguousarray(data, dtype=np.float32)
    m = data.shape[0]
    idx, diff, ret = oracle.winners(codes, data, 1, False, mask)
    searched = ret != 0
    b1 = np.where(searched, idx[:, 0], -1).astype(np.int64)
    d1 = diff[:, 0].copy()
    b2 = np.full(m, -1, dtype=np.int64)
    if codes.shape[0] >= 2:
        for u in np.unique(b1[b1 >= 0]):
            rows = np.nonzero(b1 == u)[0]
            rest = np.delete(codes, u, axis=0)
            i2, _, r2 = oracle.winners(rest, data[rows], 1, False, None if mask is None else mask[rows])
            i2 = i2[:, 0]
            b2[rows] = np.where((r2 != 0) & (i2 >= 0), i2 + (i2 >= u), -1)
    return b1, d1, b2, searched


class Replay:
    """The pairs of every data row once (the oracle's part); run() then replays any window of them."""

    def __init__(self, oracle, codes, xdim, ydim, topol, data, mask=None):
        assert xdim * ydim == codes.shape[0]
        self.n_units, self.xdim, self.topol, self.n = codes.shape[0], xdim, topol, data.shape[0]
        self.b1, self.d1, self.b2, self.searched = pairs(oracle, codes, data, mask)
        self.error = np.array([b >= 0 and c >= 0 and not adjacent(topol, xdim, int(b), int(c))
                               for b, c in zip(self.b1, self.b2)], dtype=bool)

    def run(self, first=0, count=None, hits=None, qsum=None, qerror=0.0):
        count = self.n if count is None else count
        hits = np.zeros(self.n_units, dtype=np.uint32) if hits is None else np.array(hits, dtype=np.uint32)
        qsum = np.zeros(self.n_units, dtype=np.float64) if qsum is None else np.array(qsum, dtype=np.float64)
        q = np.float32(qerror)
        tot = {"searched": 0, "topo_defined": 0, "topo_errors": 0}
        for s in range(count):
            r = (first + s) % self.n
            if not self.searched[r]:
                continue
            tot["searched"] += 1
            u = int(self.b1[r])
            root = np.sqrt(np.float64(self.d1[r]))
            q = np.float32(np.float64(q) + root)
            if u < 0:
                continue
            hits[u] += 1
            qsum[u] = qsum[u] + root
            tot["topo_defined"] += int(self.b2[r] >= 0)
            tot["topo_errors"] += int(self.error[r])
        tot["qerror"] = q
        return tot, hits, qsum


def unit_lines(xdim, hits, qsum):
    """somqual's -uout file: x y hits mean per unit"""
    out = []
    for u in range(len(hits)):
        mean = "%f" % (qsum[u] / float(hits[u])) if hits[u] else "0"
        out.append("%d %d %d %s\n" % (u % xdim, u // xdim, int(hits[u]), mean))
    return "".join(out)
