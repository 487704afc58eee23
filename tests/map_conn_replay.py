"""CPU replay of somhip_map_connectivity (K1c): the table of ordered (best unit, second-best unit) pairs with the number of
samples that have each, from map_quality_replay.pairs (the oracle's find_winner_euc twice) and np.unique.

A table is (b1 uint32[], b2 uint32[], count uint64[]), ascending by (b1, b2), counts non-zero."""
import numpy as np

from map_quality_replay import lattice_sq, pairs


def table_of(b1, b2, n_units):
    """the table of per-sample b1 / b2 (int64, -1 where there is none)"""
    b1, b2 = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)
    defined = (b1 >= 0) & (b2 >= 0)
    word, count = np.unique(b1[defined] * n_units + b2[defined], return_counts=True)
    return (word // n_units).astype(np.uint32), (word % n_units).astype(np.uint32), count.astype(np.uint64)


def add_tables(n_units, *tables):
    """the table that holds what several runs added, one after the other"""
    word = np.concatenate([t[0].astype(np.int64) * n_units + t[1].astype(np.int64) for t in tables])
    count = np.concatenate([t[2] for t in tables])
    u, inv = np.unique(word, return_inverse=True)
    total = np.zeros(len(u), dtype=np.uint64)
    np.add.at(total, inv, count)
    return (u // n_units).astype(np.uint32), (u % n_units).astype(np.uint32), total


class ConnReplay:
    """The pairs of every data row once (the oracle's part); table() then counts any window of them, wrapped runs and runs
    far longer than the data by indexing."""

    def __init__(self, oracle, codes, data, mask=None):
        self.n_units, self.n = codes.shape[0], data.shape[0]
        self.b1, self.d1, self.b2, self.searched = pairs(oracle, codes, data, mask)

    def table(self, first=0, count=None):
        count = self.n if count is None else count
        rows = (first + np.arange(count, dtype=np.int64)) % self.n
        return table_of(self.b1[rows], self.b2[rows], self.n_units)


def apart(topol, xdim, b1, b2):
    """per pair: the squared lattice distance is above 1 (the pair is a topographic error)"""
    return np.array([lattice_sq(topol, int(a) % xdim, int(a) // xdim, int(b) % xdim, int(b) // xdim) > np.float32(1.0)
                     for a, b in zip(b1, b2)], dtype=bool)


def pair_lines(topol, xdim, table):
    """somqual's -conn file: x1 y1 x2 y2 count lsq per pair"""
    out = []
    for a, b, c in zip(*table):
        a, b = int(a), int(b)
        lsq = lattice_sq(topol, a % xdim, a // xdim, b % xdim, b // xdim)
        out.append("%d %d %d %d %d %s\n" % (a % xdim, a // xdim, b % xdim, b // xdim, int(c), "%g" % float(lsq)))
    return "".join(out)
