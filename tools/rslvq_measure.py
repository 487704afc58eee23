#!/usr/bin/env python3
"""Times batch Robust Soft LVQ (somhip_rslvq_train, K13) per stage on one MI355X, next to batch GLVQ's epoch at the same
shape from the same visit, over 100 000 samples at 30 x 16, 1000 x 256 and 10 000 x 256.

Data and codebook are a seeded mixture stream like bench.py's LVQ configurations (c3's seed and classes at 256 dims): the
data its first 100 000 rows, the codebook the rows behind them, each row labelled with its mixture id.  sigma2 = dim / 2:
the mean squared distance of a sample to a row of its own cluster is 2 dim, so the posteriors are neither uniform nor all
but one zero.

Per shape, best of `--reps` after one warm-up call, the epoch chosen by the host clock, its stages from the HIP events of
somhip_rslvq_timing / somhip_glvq_timing:
  rslvq    one epoch of somhip_rslvq_train: distances, posteriors, sums, update, and the host clock around the call
  glvq     one epoch of somhip_glvq_train: search, terms + group, sums, update -- the yardstick: RSLVQ's distance stage does
           the work of GLVQ's scan, what the posteriors and the sums add is RSLVQ's own
  sums     the fp64 MFMA work of k_rslvq_sums: useful = 2 n rows (dim + 1); issued = what the 64 x 64 tiles and the fifth
           accumulator tile of the first column block multiply, zeros included; both against 78.6 TFLOP/s
  posterior  the bytes it moves (three streams of the distances, the write, read-back and rewrite of Q) per second, and the
           exponentials per second
--out FILE also writes the lines there."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (codebook rows, dim, classes, seed of the stream)
    "small": (30, 16, 3, 1234),       # (three classes: 30 rows of the stream carry every one of them)
    "mid": (1000, 256, 100, 2345),
    "c3": (10000, 256, 100, 2345),
}
SAMPLES = 100000
PEAK_F64_MATRIX = 78.6e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="small,mid,c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from som_lvq_pak_amd import engine as E

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = E.Engine(0)
    n = a.samples
    for name in a.shapes.split(","):
        rows, dim, classes, seed = SHAPES[name]
        sigma2 = dim / 2.0
        ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
        src.close()
        cb = E.Codebook(eng, codes, labels=clab)
        chunk, ld = E.rslvq_chunk(rows)
        say("%s: %d x %d codebook, %d classes, %d samples, sigma2 %g; chunk %d samples, ld %d" % (name, rows, dim, classes, n, sigma2, chunk, ld))

        def epoch(train, timing):
            best = None
            for rep in range(a.reps + 1):
                cb.upload(codes)
                eng.timing(True)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                train()
                wall = (time.perf_counter() - t0) * 1e3
                t = timing()
                eng.timing(False)
                if rep and (best is None or wall < best[0]):
                    best = (wall, t)
            return best

        wall, t = epoch(lambda: E.rslvq_train(cb, ds, 1, 1.0, sigma2, stats=False), eng.rslvq_timing)
        d_ms, p_ms, s_ms, u_ms = (t[k][1] for k in ("distances", "k_rslvq_posterior", "k_rslvq_sums", "k_rslvq_update"))
        say("  rslvq epoch (best of %d by the host clock): %.3f ms; distances %.3f, posteriors %.3f, sums %.3f, update %.3f ms" %
            (a.reps, wall, d_ms, p_ms, s_ms, u_ms))
        gwall, g = epoch(lambda: E.glvq_train(cb, ds, 1, 1.0, stats=False), eng.glvq_timing)
        say("  glvq  epoch (best of %d by the host clock): %.3f ms; search %.3f, terms + group %.3f, sums %.3f, update %.3f ms" %
            (a.reps, gwall, g["search"][1], g["terms"][1], g["k_glvq_sums"][1], g["k_glvq_update"][1]))
        say("  rslvq / glvq epoch: %.2f; distances / glvq search: %.2f; posteriors + sums add %.3f ms (%.2f of the distances)" %
            (wall / gwall, d_ms / g["search"][1], p_ms + s_ms, (p_ms + s_ms) / d_ms))
        useful = 2.0 * n * rows * (dim + 1)
        blocks = (dim + 63) // 64
        n64 = (n + 63) // 64 * 64                                   # (the last chunk's last tile is padded with zeros)
        issued = 2.0 * n64 * ld * (64.0 * blocks + 16.0)
        say("  sums: useful %.4g FLOP, issued %.4g FLOP in %.3f ms = %.2f useful / %.2f issued TFLOP/s: %.1f %% / %.1f %% of 78.6 TFLOP/s" %
            (useful, issued, s_ms, useful / s_ms / 1e9, issued / s_ms / 1e9, 100 * useful / s_ms / 1e9 / (PEAK_F64_MATRIX / 1e12),
             100 * issued / s_ms / 1e9 / (PEAK_F64_MATRIX / 1e12)))
        moved = float(n) * ld * (3 * 4 + 3 * 8)
        say("  posteriors: %.4g bytes (3 reads of a distance, write + read + write of a coefficient) in %.3f ms = %.2f TB/s; "
            "%.4g exponentials = %.3g per second; %.3g serial fp64 additions per wave" %
            (moved, p_ms, moved / p_ms / 1e9, float(n) * rows, float(n) * rows / p_ms * 1e3, 2.0 * ld))
        cb.close()
        ds.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
