#!/usr/bin/env python3
"""Times batch GMLVQ (somhip_gmlvq_train, K12) per stage on one MI355X beside batch GLVQ's class-wise scan (K9) on the same
data in the same process, at the shapes of the LVQ bench configurations: 10 000 x 256 (c3) and 100 000 x 1024 (c5),
100 000 samples each, at ranks 2, 16 and dim.

Data and codebook are those of tools/glvq_measure.py: the seeded mixture stream of bench.py's LVQ configurations, the data
its first 100 000 rows, the codebook the rows behind them, each row labelled with its mixture id.  Omega is
engine.gmlvq_omega(dim, rank).

Per shape and rank, best of `--reps` after one warm-up call, from HIP events (somhip_gmlvq_timing, somhip_glvq_timing):
  scan     alternating: k_scan_class over all dim columns (somhip_debug_glvq_search on the direct route), then
           somhip_gmlvq_search, whose projection and scan over rank columns are reported apart; the ratio of the two
           scans beside rank / dim
  epoch    one epoch of somhip_gmlvq_train: projection, search, terms + group, sums, the gradient of Omega with its
           reduction, update, the host clock around the call, and the bytes of the gradient's partial sums
--out FILE also writes the lines there."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (codebook rows, dim, classes, seed of the stream)
    "c3": (10000, 256, 100, 2345),
    "c5": (100000, 1024, 1000, 4567),
}
SAMPLES = 100000
BLOCK = 4096


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--ranks", default="2,16,dim")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from som_lvq_pak_amd import engine as E

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    eng = E.Engine(0)
    n = a.samples
    for name in a.shapes.split(","):
        rows, dim, classes, seed = SHAPES[name]
        ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
        src.close()
        cb = E.Codebook(eng, codes, labels=clab)
        say("%s: %d x %d codebook, %d classes, %d samples" % (name, rows, dim, classes, n))
        for rank in (dim if r == "dim" else int(r) for r in a.ranks.split(",")):
            om = E.gmlvq_omega(dim, rank)
            blocks = (n + BLOCK - 1) // BLOCK
            say(" rank %d: the gradient's partial sums [%d blocks][%d][%d] doubles: %.3f GB" % (rank, blocks, rank, dim, 8.0 * blocks * rank * dim / 1e9))
            plain, proj, scan = [], [], []
            for rep in range(a.reps + 1):                           # alternating: the yardstick, then the projected search
                for which in ("plain", "projected"):
                    eng.timing(True)
                    eng.timing_reset()
                    if which == "plain":
                        E.glvq_search(cb, ds, 0, n, E.GLVQ_DIRECT)
                        ms = eng.glvq_timing()["search"][1]
                        if rep:
                            plain.append(ms)
                    else:
                        E.gmlvq_search(cb, ds, om, 0, n)
                        t = eng.gmlvq_timing()
                        if rep:
                            proj.append(t["k_gmlvq_project"][1])
                            scan.append(t["search"][1])
                    eng.timing(False)
            say("  scan k_scan_class, %4d columns  best %9.3f ms  all %s  spread %.2f %%" %
                (dim, min(plain), ["%.3f" % v for v in plain], 100.0 * (max(plain) - min(plain)) / min(plain)))
            say("  scan k_scan_class, %4d columns  best %9.3f ms  all %s  ratio of the bests %.4f (rank / dim: %.4f)" %
                (rank, min(scan), ["%.3f" % v for v in scan], min(scan) / min(plain), rank / dim))
            say("  k_gmlvq_project (samples + rows) best %9.3f ms  all %s" % (min(proj), ["%.3f" % v for v in proj]))
            best = None
            for rep in range(a.reps + 1):
                cb.upload(codes)
                eng.timing(True)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                E.gmlvq_train(cb, ds, 1, 1.0, 0.5, om, stats=False)
                wall = (time.perf_counter() - t0) * 1e3
                t = eng.gmlvq_timing()
                eng.timing(False)
                if rep and (best is None or wall < best[0]):
                    best = (wall, t)
            wall, t = best
            fp64 = t["k_gmlvq_project"][1] + t["k_gmlvq_omega_grad"][1] + t["k_gmlvq_update"][1]
            say("  gmlvq epoch (best of %d by the host clock): %.3f ms; projection %.3f, search %.3f, terms + group %.3f, sums %.3f, "
                "gradient + reduce %.3f, update %.3f ms; the three fp64 stages %.3f ms = %.3f of the full scan" %
                (a.reps, wall, t["k_gmlvq_project"][1], t["search"][1], t["terms"][1], t["sums"][1], t["k_gmlvq_omega_grad"][1],
                 t["k_gmlvq_update"][1], fp64, fp64 / min(plain)))
        cb.close()
        ds.close()
    eng.close()


if __name__ == "__main__":
    main()
