#!/usr/bin/env python3
"""Times batch GLVQ (somhip_glvq_train, K9) per stage on one MI355X, both routes of its search, at the shapes of the LVQ
bench configurations: 10 000 x 256 (c3) and 100 000 x 1024 (c5), 100 000 samples each.

Data and codebook are the seeded mixture stream of bench.py's LVQ configurations (same seed, classes and dimension): the
data its first 100 000 rows, the codebook the rows behind them, each row labelled with its mixture id.

Per shape, best of `--reps` after one warm-up call, from the HIP events of somhip_glvq_timing:
  search   the class-wise winner search alone (somhip_debug_glvq_search) on the direct route and on the list route, and the
           share of the samples in the list route's remainder
  epoch    one epoch of somhip_glvq_train on the planned route: search, terms + group, sums, update, and the host clock
           around the call
For orientation only, beside them: one pass of the same data through lvq_train OLVQ1 (the exact batched online engine),
host clock.  --out FILE also writes the lines there."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (codebook rows, dim, classes, seed of the stream, alpha of the OLVQ1 line)
    "c3": (10000, 256, 100, 2345, 0.3),
    "c5": (100000, 1024, 1000, 4567, 0.05),
}
SAMPLES = 100000


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--no-olvq1", action="store_true")
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
        rows, dim, classes, seed, alpha = SHAPES[name]
        ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
        src.close()
        cb = E.Codebook(eng, codes, labels=clab)
        say("%s: %d x %d codebook, %d classes, %d samples; planned route: %s" %
            (name, rows, dim, classes, n, "list" if E.glvq_plan(rows, dim, n) == E.GLVQ_LIST else "direct"))
        found = {}
        for route, rname in ((E.GLVQ_DIRECT, "direct"), (E.GLVQ_LIST, "list")):
            ms, rem = [], 0
            for rep in range(a.reps + 1):
                eng.timing(True)
                eng.timing_reset()
                out = E.glvq_search(cb, ds, 0, n, route)
                t = eng.glvq_timing()
                eng.timing(False)
                rem = out[4]
                if rep:
                    ms.append(t["search"][1])
            found[rname] = out[:4]
            elems = float(n if route == E.GLVQ_DIRECT else rem) * rows * dim
            say("  search %-6s best %9.3f ms  all %s  remainder %d of %d (%.2f %%)  class-wise scan: %.3g fp32 elements" %
                (rname, min(ms), ["%.3f" % v for v in ms], rem, n, 100.0 * rem / n, elems))
        same = all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(found["direct"], found["list"]))
        say("  the two routes agree by bit pattern and index: %s" % same)
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
        say("  epoch (best of %d by the host clock): %.3f ms; search %.3f, terms + group %.3f, sums %.3f, update %.3f ms" %
            (a.reps, wall, t["search"][1], t["terms"][1], t["k_glvq_sums"][1], t["k_glvq_update"][1]))
        if not a.no_olvq1:
            walls = []
            for rep in range(a.reps + 1):
                cb.upload(codes)
                talpha = np.full(rows, alpha, dtype=np.float32)
                eng.sync()
                t0 = time.perf_counter()
                E.lvq_train(cb, ds, E.OLVQ1, n, alpha, talpha=talpha, count=n, data_first=0, trace=False)
                eng.sync()
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
            say("  for orientation: lvq_train OLVQ1, one pass of the same %d samples: best %.1f ms  all %s" %
                (n, min(walls), ["%.1f" % v for v in walls]))
        cb.close()
        ds.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
