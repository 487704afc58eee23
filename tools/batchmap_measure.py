#!/usr/bin/env python3
"""Times the batch map (somhip_som_batchmap, K8) per stage on one MI355X and sets it beside the online engine.

Per shape, neighbourhood and radius: one epoch (epochs = 1, so r_0 is the radius given) from the same codebook every time
(re-uploaded outside the timed window).  One warm-up call, then `--reps` calls with the host clock from an engine
synchronise to the return of the call (the call ends in a device synchronise), events off; then `--reps` calls with the
LaunchTimer on for the stage totals (somhip_batchmap_timing) and the winner search's kernels (the published table).

Derived figures, computed here from the shapes:
  sums     bytes = n * dim * 4 (every row once) + n * 4 (the list) + units * (dim + 1) * 8 (S written), over the sums' time,
           against the HBM figures of MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured)
  combine  useful FLOP = 2 * units^2 * (dim + 1) (H dense); issued FLOP = 2 * 64 * 64 * 80 per (destination group, source
           group, column block) that the kernel does not skip, counted here by the kernel's own box rule; over the combine's
           time, against the fp64 matrix rate: MI355X_MICROARCH.md lists none, so AMD's published 78.6 TFLOP/s for the MI355X
           is used (half the guide's 157.3 TFLOP/s fp32 matrix rate)

--parent-lib PATH: also times somhip_som_train at batch auto over the same number of vectors with that library (the parent
commit's, built from a clean checkout of it), in a child process that loads it through SOMHIP_LIB."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12
FP64_MATRIX = 78.6e12
SHAPES = [  # xdim, ydim, dim, vectors, radii
    (256, 256, 512, 1000000, (128.0, 16.0, 1.0)),
    (32, 32, 128, 1000000, (16.0, 4.0, 1.0)),
]


def group_boxes(xdim, ydim):
    """the lattice boxes of the 64-row groups, as bm_group_box (kernels/batchmap.hpp) forms them"""
    units = xdim * ydim
    ng = (units + 63) // 64
    g = np.arange(ng)
    if xdim % 8 == 0 and ydim % 8 == 0:
        pw = xdim // 8
        x0, y0 = (g % pw) * 8, (g // pw) * 8
        return x0, x0 + 7, y0, y0 + 7
    u0, u1 = g * 64, np.minimum(g * 64 + 63, units - 1)
    y0, y1 = u0 // xdim, u1 // xdim
    one = y0 == y1
    return np.where(one, u0 % xdim, 0), np.where(one, u1 % xdim, xdim - 1), y0, y1


def issued_tiles(xdim, ydim, topol, gauss, thresh):
    """(destination group, source group) pairs the combine stages and multiplies"""
    x0, x1, y0, y1 = group_boxes(xdim, ydim)
    ng = len(x0)
    if gauss:
        return ng * ng
    gx = np.maximum(0, np.maximum(x0[None, :] - x1[:, None], x0[:, None] - x1[None, :])).astype(np.float64)
    gy = np.maximum(0, np.maximum(y0[None, :] - y1[:, None], y0[:, None] - y1[None, :])).astype(np.float64)
    hx = gx if topol == 4 else np.maximum(0.0, gx - 0.5)
    least = hx * hx + (1.0 if topol == 4 else 0.75) * gy * gy
    return int((least <= thresh * 1.000001).sum())


def med(v):
    return statistics.median(v)


def fmt(v):
    return "[" + ", ".join("%.3f" % x for x in v) + "]"


def measure_batchmap(E, eng, reps, shapes, out):
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]                # the next rows of the stream: spread like the data, unordered
        for neigh, nname in ((E.NEIGH_BUBBLE, "bubble"), (E.NEIGH_GAUSSIAN, "gaussian")):
            cb = E.Codebook(eng, codes, E.TOPOL_HEXA, neigh, xdim, ydim)
            for radius in radii:
                def epoch(events):
                    cb.upload(codes)
                    eng.timing(events)
                    eng.timing_reset()
                    eng.sync()
                    t0 = time.perf_counter()
                    E.som_batchmap(cb, ds, 1, radius, qerror=False)
                    wall = (time.perf_counter() - t0) * 1e3
                    st = eng.batchmap_timing() if events else None
                    tab = eng.timing_table() if events else None
                    eng.timing(False)
                    return wall, st, tab
                epoch(False)
                walls = [epoch(False)[0] for _ in range(reps)]
                timed = [epoch(True) for _ in range(reps)]
                grp = [t[1]["group"][1] for t in timed]
                sums = [t[1]["k_batchmap_sums"][1] for t in timed]
                comb = [t[1]["k_batchmap_combine"][1] for t in timed]
                search = [sum(ms for _, ms in t[2].values()) for t in timed]
                wall_ev = [t[0] for t in timed]
                sum_bytes = n * dim * 4 + n * 4 + units * (dim + 1) * 8
                useful = 2.0 * units * units * (dim + 1)
                thresh = radius * radius                          # (the box rule against the squared radius, as the kernel's thresh)
                tiles = issued_tiles(xdim, ydim, E.TOPOL_HEXA, neigh == E.NEIGH_GAUSSIAN, thresh)
                issued = 2.0 * 64 * 64 * 80 * tiles * ((dim + 63) // 64)
                out("== %d x %d x %d hexa %s, radius %g, %d generated vectors, one epoch" % (xdim, ydim, dim, nname, radius, n))
                out("  wall ms, events off: median %.3f of %s" % (med(walls), fmt(walls)))
                out("  wall ms, events on:  median %.3f of %s" % (med(wall_ev), fmt(wall_ev)))
                out("  stage ms (events): group %.3f %s | sums %.3f %s | combine %.3f %s | winner-search kernels %.3f %s"
                    % (med(grp), fmt(grp), med(sums), fmt(sums), med(comb), fmt(comb), med(search), fmt(search)))
                w = med(wall_ev)
                out("  shares of the events-on wall: search %.1f %%, group %.1f %%, sums %.1f %%, combine %.1f %%, rest (copies, gaps) %.1f %%"
                    % (100 * med(search) / w, 100 * med(grp) / w, 100 * med(sums) / w, 100 * med(comb) / w,
                       100 * (w - med(search) - med(grp) - med(sums) - med(comb)) / w))
                bps = sum_bytes / (med(sums) * 1e-3)
                out("  sums: %.1f MB in %.3f ms = %.3f TB/s: %.1f %% of 8.0 TB/s spec, %.1f %% of 6.29 TB/s measured"
                    % (sum_bytes / 1e6, med(sums), bps / 1e12, 100 * bps / HBM_SPEC, 100 * bps / HBM_MEASURED))
                out("  combine: useful %.3f TFLOP (dense H), issued %.3f TFLOP (%d of %d group pairs) in %.3f ms = %.2f useful / %.2f issued "
                    "TFLOP/s: %.1f %% / %.1f %% of 78.6 TFLOP/s"
                    % (useful / 1e12, issued / 1e12, tiles, ((units + 63) // 64) ** 2, med(comb), useful / med(comb) / 1e9,
                       issued / med(comb) / 1e9, 100 * useful / (med(comb) * 1e-3) / FP64_MATRIX,
                       100 * issued / (med(comb) * 1e-3) / FP64_MATRIX))
            cb.close()
        ds.close()


def measure_online(E, eng, reps, shapes, out, who):
    """somhip_som_train at batch auto over as many vectors as an epoch reads"""
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
        walls = []
        for rep in range(min(reps, 2) + 1):
            cb.upload(codes)
            eng.sync()
            t0 = time.perf_counter()
            E.som_train(cb, ds, n, 0.05, radii[0], batch=-1, trace=False)
            eng.sync()
            walls.append((time.perf_counter() - t0) * 1e3)
        out("== %s: somhip_som_train, batch auto, %d x %d x %d hexa bubble, radius %g -> 1, alpha 0.05, %d iterations over %d generated vectors"
            % (who, xdim, ydim, dim, radii[0], n, n))
        out("  wall ms: median %.3f of %s after a warm-up run of %.3f" % (med(walls[1:]), fmt(walls[1:]), walls[0]))
        cb.close(); ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--online-only", default=None, help="(the child process) label of the library under SOMHIP_LIB")
    ap.add_argument("--batchmap-only", action="store_true", help="leave the online runs out")
    ap.add_argument("--small", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [(24, 16, 40, 5000, (6.0, 1.0))] if a.small else SHAPES
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    from som_lvq_pak_amd import _lib, engine as E
    if a.online_only:                                   # the parent's library has no batch map: bind what it has
        for name in [k for k in _lib.SIGNATURES if "batchmap" in k]:
            del _lib.SIGNATURES[name]
    eng = E.Engine(0)
    if a.online_only:
        measure_online(E, eng, a.reps, shapes, out, a.online_only)
    else:
        measure_batchmap(E, eng, a.reps, shapes, out)
        if not a.batchmap_only:
            measure_online(E, eng, a.reps, shapes, out, "this commit")
    eng.close()
    if a.parent_lib and not a.online_only and not a.batchmap_only:
        cmd = [sys.executable, os.path.abspath(__file__), "--online-only", "parent", "--reps", str(a.reps)] + (["--small"] if a.small else [])
        p = subprocess.run(cmd, env=dict(os.environ, SOMHIP_LIB=os.path.abspath(a.parent_lib)), stdout=subprocess.PIPE, text=True, check=True)
        for s in p.stdout.rstrip("\n").split("\n"):
            out(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"lines": len(lines)}))


if __name__ == "__main__":
    main()
