#!/usr/bin/env python3
"""Times map distortion (somhip_distortion_*, K1d) per stage on one MI355X beside the batch map's stages it is made from.

Per shape, over generated vectors, with the LaunchTimer on (HIP events around every launch; somhip_distortion_timing and
somhip_batchmap_timing), one warm-up and `--reps` timed repetitions each, medians:
  accumulate   Distortion.accumulate into a cleared state beside somhip_debug_batchmap_sums on the same inputs.  The search,
               the group stage and the sums kernel are the same code, so the difference of the sums ids is the two Q passes;
               the bytes of one read of the data over that difference is set against the HBM figures of
               MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured).
  evaluate     Distortion.evaluate beside somhip_debug_batchmap_combine (its combine id: the table and the kernel) from the
               same hits and sums, bubble and gaussian, at the radii given.  Both issue the same MFMAs.
  the tool     `somqual` and `somqual -distortion R` end to end on a gen: source (process start to exit, the host clock of this
               script), for shapes whose map file is small enough to write as text."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12
SHAPES = [  # xdim, ydim, dim, vectors, radii
    (256, 256, 512, 1000000, (1.0, 128.0)),
    (32, 32, 128, 1000000, (1.0, 16.0)),
]
TOOL_MAX_VALUES = 1 << 20      # a map file of more values than this is not written


def med(v):
    return statistics.median(v)


def fmt(v):
    return "[" + ", ".join("%.3f" % x for x in v) + "]"


def timed(eng, fn, read):
    eng.timing(True)
    eng.timing_reset()
    eng.sync()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    out = read()
    eng.timing(False)
    return wall, out


def measure(E, eng, reps, shapes, out):
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
        st = E.Distortion(cb)

        def acc():
            st.clear()
            st.accumulate(cb, ds)
        out("== %d x %d x %d hexa, %d generated vectors" % (xdim, ydim, dim, n))
        timed(eng, acc, eng.distortion_timing)
        runs = [timed(eng, acc, eng.distortion_timing) for _ in range(reps)]
        timed(eng, lambda: E.batchmap_sums(cb, ds), eng.batchmap_timing)
        base = [timed(eng, lambda: E.batchmap_sums(cb, ds), eng.batchmap_timing) for _ in range(reps)]
        dg, dsum = [r[1]["group"][1] for r in runs], [r[1]["sums"][1] for r in runs]
        bg, bsum = [r[1]["group"][1] for r in base], [r[1]["k_batchmap_sums"][1] for r in base]
        out("  accumulate: wall ms median %.3f of %s (somhip_debug_batchmap_sums with its copy to the host: %.3f of %s)"
            % (med([r[0] for r in runs]), fmt([r[0] for r in runs]), med([r[0] for r in base]), fmt([r[0] for r in base])))
        out("  group ms: distortion %.3f %s | batch map %.3f %s" % (med(dg), fmt(dg), med(bg), fmt(bg)))
        out("  sums ms:  distortion (sums<true>, q, q sums) %.3f %s | batch map (sums<false>) %.3f %s" % (med(dsum), fmt(dsum), med(bsum), fmt(bsum)))
        qms = med(dsum) - med(bsum)
        bps = n * dim * 4 / (qms * 1e-3) if qms > 0 else float("nan")
        out("  the two Q passes: %.3f ms; one read of the data, %.1f MB, in that time = %.3f TB/s: %.1f %% of 8.0 TB/s spec, %.1f %% of "
            "6.29 TB/s measured" % (qms, n * dim * 4 / 1e6, bps / 1e12, 100 * bps / HBM_SPEC, 100 * bps / HBM_MEASURED))
        hits, S, _ = st.read()
        st.close(); cb.close()
        for neigh, nname in ((E.NEIGH_BUBBLE, "bubble"), (E.NEIGH_GAUSSIAN, "gaussian")):
            cb = E.Codebook(eng, codes, E.TOPOL_HEXA, neigh, xdim, ydim)
            st = E.Distortion(cb)
            st.accumulate(cb, ds)
            for r in radii:
                tot = st.evaluate(cb, r, units=False)[0]
                ev = [timed(eng, lambda: st.evaluate(cb, r, units=False), eng.distortion_timing)[1]["evaluate"][1] for _ in range(reps)]

                def combine():
                    E.batchmap_combine(cb, r, hits, S)
                cb.upload(codes)
                timed(eng, combine, eng.batchmap_timing)
                cm = []
                for _ in range(reps):
                    cb.upload(codes)
                    cm.append(timed(eng, combine, eng.batchmap_timing)[1]["k_batchmap_combine"][1])
                cb.upload(codes)
                out("  %s radius %g: evaluate %.3f ms %s | k_batchmap_combine %.3f ms %s | E / sample %.9g, scale / E %.3g"
                    % (nname, r, med(ev), fmt(ev), med(cm), fmt(cm), tot["energy"] / tot["samples"], tot["scale"] / tot["energy"]))
            st.close(); cb.close()
        ds.close()
        if units * dim > TOOL_MAX_VALUES:
            out("  the tool: not run at this shape (a map file of %d values as text)" % (units * dim))
            continue
        with tempfile.TemporaryDirectory() as tmp:
            cod = os.path.join(tmp, "m.cod")
            with open(cod, "w") as fh:
                fh.write("%d hexa %d %d bubble\n" % (dim, xdim, ydim))
                for row in codes:
                    fh.write(" ".join("%.9g" % v for v in row) + "\n")
            gen = "gen:k=16,dim=%d,n=%d,seed=9" % (dim, n)
            exe = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "somqual")
            for name, extra in (("somqual", []), ("somqual -distortion %g" % radii[-1], ["-distortion", str(radii[-1])])):
                walls = []
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    p = subprocess.run([exe, "-din", gen, "-cin", cod] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                    walls.append(time.perf_counter() - t0)
                    assert p.returncode == 0, p.stderr
                out("  %s: process wall s, first %.3f, then median %.3f of %s" % (name, walls[0], med(walls[1:]), fmt(walls[1:])))
                out("    " + p.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="the 32 x 32 x 128 shape only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from som_lvq_pak_amd import engine as E
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    eng = E.Engine(0)
    measure(E, eng, a.reps, SHAPES[1:] if a.small else SHAPES, out)
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
