"""A plain NumPy replay of one mini-batch run of som_training (som_rout.c:556-671) with its winners given.

The run is iterations [start_iter, start_iter + count) of a schedule of `length` iterations; iteration j of the run
reads data row (data_first + j) mod n and is taught at winners[j]: a unit index, -3 for a sample whose fixed point
replaces the winner (som_rout.c:628-632, also when the point lies beyond the map's edge), or -2 for a sample that
teaches nothing (som_rout.c:635-640).  The updates are applied in iteration order, as the batch oracle and the exact
kernels apply them.  Every scalar is formed in the reference's own C types:

  radius   (float)(1.0 + (radius - 1.0) * (double)(float)(length - le) / (double)(float)length)   som_rout.c:615
  rate     linear_alpha / inverse_t_alpha in float                                              lvq_pak.c:903-921
  weights  1 - (float)pow(1 - talp, weight)                                                     som_rout.c:622-624
  lattice  hexa_dist / rect_dist: float diff (+-0.5 on odd row differences), the sum in double
           stored into a float, (float)sqrt((double)ret)                                        som_rout.c:433-467
  bubble   dist <= radius, in float                                                             som_rout.c:496
  gaussian alpha * (float)exp((double)(-dd*dd) / (2.0 * radius * radius)), the C library's exp   som_rout.c:539-542

dtype=np.float32 runs adapt_vector's c += a * (x - c) with its three roundings (lvq_pak.c:339-351): it equals the batch
oracle bit for bit.  dtype=np.float64 runs the same updates in double: the yardstick for forms that round differently.

The result also carries, per unit, the number of hits (updates with a nonzero rate) and, per (unit, dim),
S = P0 |c| + sum_j |w_j| |x_j| (w_j = a_j prod_{i>j} (1 - a_i), P0 = prod (1 - a_i)), the magnitude a sum-of-products
form of the same update works with, formed by the recursion S <- |1 - a| S + |a| |x|.

`fault` seeds one error into the replay (to show that a tolerance can see it):
  ("drop", u, k)       hit k of unit u is not applied
  ("swap", u, k)       hits k and k + 1 of unit u are applied in the opposite order
  ("next_rate", u, k)  hit k of unit u takes its rate from the next iteration's schedule
k < 0 counts from the unit's last hit.  A fixed point taken wrongly is a fault of the inputs: pass altered fixed_xy."""
import math
from collections import namedtuple

import numpy as np

TOPOL_HEXA, TOPOL_RECT = 3, 4
NEIGH_BUBBLE, NEIGH_GAUSSIAN = 1, 2
ALPHA_LINEAR, ALPHA_INVERSE_T = 1, 2

Replay = namedtuple("Replay", "codes hits S")
f32 = np.float32


def som_radius(le, length, radius):
    return f32(1.0 + (float(f32(radius)) - 1.0) * float(f32(length - le)) / float(f32(length)))


def som_alpha(alpha_type, le, length, alpha):
    alpha = f32(alpha)
    if alpha_type == ALPHA_INVERSE_T:
        c = f32(f32(length) / f32(100.0))
        return f32(f32(alpha * c) / f32(c + f32(le)))
    return f32(f32(alpha * f32(length - le)) / f32(length))


def weighted_alpha(talp, w):
    return f32(1.0 - float(f32(math.pow(1.0 - float(talp), float(w)))))


def lattice_dist(topol, bx, by, tx, ty):
    """hexa_dist / rect_dist from winner (bx, by) to the units (tx, ty): float32 array"""
    dx = (bx - tx).astype(f32)
    dy = (by - ty).astype(f32)
    if topol == TOPOL_RECT:
        r = (dx * dx) + (dy * dy)                         # float arithmetic throughout (som_rout.c:457-467)
    else:
        odd = ((by - ty) % 2) != 0
        dx = np.where(odd, (dx.astype(np.float64) + (0.5 if by % 2 else -0.5)).astype(f32), dx)
        r = (dx * dx).astype(np.float64)
        r = (r + 0.75 * dy.astype(np.float64) * dy.astype(np.float64)).astype(f32)
    return np.sqrt(r.astype(np.float64)).astype(f32)


def _gauss_factor(dd, trad):
    """(float)exp((double)(-dd*dd) / (2.0 * radius * radius)) per unit, with the C library's exp"""
    neg = -(dd * dd)
    den = 2.0 * float(trad) * float(trad)
    vals, inv = np.unique(neg, return_inverse=True)
    h = np.array([f32(math.exp(float(v) / den)) for v in vals], dtype=f32)
    return h[inv.reshape(-1)]


def replay(codes, xdim, ydim, topol, neigh, data, length, alpha, radius, winners, start_iter=0, count=None,
           data_first=None, alpha_type=ALPHA_LINEAR, weight=None, fixed_xy=None, use_fixed=0, use_weights=0,
           dtype=np.float32, units=None, fault=None):
    """Replay one run; `units` (indices) restricts the work and the result to those units (default: all)."""
    data = np.ascontiguousarray(data, dtype=f32)
    n = data.shape[0]
    count = len(winners) if count is None else count
    assert len(winners) >= count
    data_first = start_iter % n if data_first is None else data_first
    nunits = xdim * ydim
    units = np.arange(nunits) if units is None else np.asarray(units, dtype=np.int64)
    tx, ty = units % xdim, units // xdim
    c = np.array(codes, dtype=f32)[units].astype(dtype)
    S = np.abs(c.astype(np.float64))
    hits = np.zeros(len(units), dtype=np.int64)
    data_t = data.astype(dtype)
    gauss = neigh == NEIGH_GAUSSIAN
    fu = fk = None
    if fault is not None:
        kind, fu_unit, fk = fault
        (pos,) = np.nonzero(units == fu_unit)
        assert len(pos) == 1, "the faulted unit must be one of the replayed units"
        fu = int(pos[0])
        assert kind in ("drop", "swap", "next_rate")
        if fk < 0:          # count from the end: a clean pass finds the unit's number of hits first
            clean = replay(codes, xdim, ydim, topol, neigh, data, length, alpha, radius, winners, start_iter, count,
                           data_first, alpha_type, weight, fixed_xy, use_fixed, use_weights, np.float64, units[pos])
            fk = int(clean.hits[0]) + fk
            assert fk >= 0
    fhit, deferred = 0, None

    def scalars(le, row):
        trad = som_radius(le, length, radius)
        talp = som_alpha(alpha_type, le, length, alpha)
        w = float(weight[row]) if weight is not None else 0.0
        if w > 0.0 and use_weights:
            talp = weighted_alpha(talp, w)
        return trad, talp

    def rates(trad, talp, bx, by, sel=slice(None)):
        """(rate, member) of the units sel for a winner at (bx, by)"""
        dd = lattice_dist(topol, bx, by, tx[sel], ty[sel])
        if gauss:
            return f32(talp) * _gauss_factor(dd, trad), np.ones(len(dd), dtype=bool)
        inside = dd <= trad
        return np.where(inside, f32(talp), f32(0.0)).astype(f32), inside

    for j in range(count):
        le, row = start_iter + j, (data_first + j) % n
        w = int(winners[j])
        if use_fixed and fixed_xy is not None and fixed_xy[row][0] >= 0:
            assert w == -3, "a sample with a fixed point is traced as -3"
        if w == -2:
            continue
        if w == -3:
            bx, by = int(fixed_xy[row][0]), int(fixed_xy[row][1])
        else:
            assert 0 <= w < nunits
            bx, by = w % xdim, w // xdim
        trad, talp = scalars(le, row)
        a, member = rates(trad, talp, bx, by)
        x = data_t[row]
        if fu is not None and member[fu] and a[fu] != 0:
            if fhit == fk:
                if fault[0] == "next_rate":
                    a = a.copy()
                    a[fu] = rates(*scalars(le + 1, row), bx, by, slice(fu, fu + 1))[0][0]
                else:           # drop; swap: hold this hit back and apply it right after the unit's next one
                    if fault[0] == "swap":
                        deferred = (a[fu], x)
                    member = member.copy()
                    member[fu] = False
            fhit += 1
        idx = np.nonzero(member)[0]
        if len(idx):
            ai = a[idx].astype(dtype)[:, None]
            ci = c[idx]
            c[idx] = ci + ai * (x - ci)                   # float32: adapt_vector's three roundings, in its order
            ad = np.abs(a[idx].astype(np.float64))[:, None]
            S[idx] = np.abs(1.0 - ad) * S[idx] + ad * np.abs(x.astype(np.float64))
            hits[idx] += a[idx] != 0
        if deferred is not None and fhit == fk + 2:
            ad, xd = deferred
            c[fu] = c[fu] + dtype(ad) * (xd - c[fu])
            hits[fu] += 1
            deferred = None
    assert deferred is None, "a swap needs a later hit of the unit"
    return Replay(c, hits, S)

