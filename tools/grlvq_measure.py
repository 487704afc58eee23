#!/usr/bin/env python3
"""Times batch GRLVQ (somhip_grlvq_train, K11) per stage on one MI355X beside batch GLVQ (K9) on the same data in the same
process, at the shapes of the LVQ bench configurations: 10 000 x 256 (c3) and 100 000 x 1024 (c5), 100 000 samples each.

Data and codebook are those of tools/glvq_measure.py: the seeded mixture stream of bench.py's LVQ configurations, the data
its first 100 000 rows, the codebook the rows behind them, each row labelled with its mixture id.  lambda is 1 / dim each.

Per shape, best of `--reps` after one warm-up call, from HIP events (somhip_grlvq_timing, somhip_glvq_timing):
  scan     the weighted class-wise scan (somhip_grlvq_search) and, alternating with it, its yardstick k_scan_class
           (somhip_debug_glvq_search on the direct route); the ratio of the two best times, and the spread of the
           yardstick's own repeats
  epoch    one epoch of somhip_grlvq_train: search, terms + group, sums, relevance reduction, update, the host clock around
           the call, and the bytes of the relevance sums R; beside it one epoch of somhip_glvq_train on its planned route,
           for k_glvq_sums and k_glvq_update (the grouping is the same: lambda = 1 / dim scales every distance alike)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
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
        lam = np.full(dim, np.float32(1.0) / np.float32(dim), dtype=np.float32)
        say("%s: %d x %d codebook, %d classes, %d samples; R (relevance sums, both roles): %.3f GB" %
            (name, rows, dim, classes, n, 16.0 * rows * dim / 1e9))
        plain, weighted = [], []
        for rep in range(a.reps + 1):                               # alternating: the yardstick, then the weighted scan
            for which in ("plain", "weighted"):
                eng.timing(True)
                eng.timing_reset()
                if which == "plain":
                    got_plain = E.glvq_search(cb, ds, 0, n, E.GLVQ_DIRECT)
                    ms = eng.glvq_timing()["search"][1]
                else:
                    got = E.grlvq_search(cb, ds, lam, 0, n)
                    ms = eng.grlvq_timing()["search"][1]
                eng.timing(False)
                if rep:
                    (plain if which == "plain" else weighted).append(ms)
        same = (got[1] == got_plain[1]).all() and (got[3] == got_plain[3]).all()
        say("  scan k_scan_class          best %9.3f ms  all %s  spread %.2f %%" %
            (min(plain), ["%.3f" % v for v in plain], 100.0 * (max(plain) - min(plain)) / min(plain)))
        say("  scan k_scan_class_weighted best %9.3f ms  all %s  ratio of the bests %.3f (four vector operations per element against three: 1.333)" %
            (min(weighted), ["%.3f" % v for v in weighted], min(weighted) / min(plain)))
        say("  winners under lambda = 1 / dim equal the unweighted ones (a uniform scale; ties aside): %s" % same)
        best = None
        for rep in range(a.reps + 1):
            cb.upload(codes)
            eng.timing(True)
            eng.timing_reset()
            eng.sync()
            t0 = time.perf_counter()
            E.grlvq_train(cb, ds, 1, 1.0, 0.5, lam, stats=False)
            wall = (time.perf_counter() - t0) * 1e3
            t = eng.grlvq_timing()
            eng.timing(False)
            if rep and (best is None or wall < best[0]):
                best = (wall, t)
        wall, t = best
        say("  grlvq epoch (best of %d by the host clock): %.3f ms; search %.3f, terms + group %.3f, sums %.3f, relevance reduction %.3f, update %.3f ms" %
            (a.reps, wall, t["search"][1], t["terms"][1], t["k_grlvq_sums"][1], t["k_grlvq_relevance"][1], t["k_grlvq_update"][1]))
        best = None
        for rep in range(a.reps + 1):
            cb.upload(codes)
            eng.timing(True)
            eng.timing_reset()
            eng.sync()
            t0 = time.perf_counter()
            E.glvq_train(cb, ds, 1, 1.0, stats=False)
            wall = (time.perf_counter() - t0) * 1e3
            t = eng.glvq_timing()
            eng.timing(False)
            if rep and (best is None or wall < best[0]):
                best = (wall, t)
        wall, t = best
        say("  glvq epoch beside it, planned route (%s): %.3f ms; search %.3f, terms + group %.3f, k_glvq_sums %.3f, k_glvq_update %.3f ms" %
            ("list" if E.glvq_plan(rows, dim, n) == E.GLVQ_LIST else "direct", wall, t["search"][1], t["terms"][1], t["k_glvq_sums"][1],
             t["k_glvq_update"][1]))
        cb.close()
        ds.close()
    eng.close()


if __name__ == "__main__":
    main()
