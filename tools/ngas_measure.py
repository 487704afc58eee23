#!/usr/bin/env python3
"""Times batch neural gas (somhip_ng_train, K10) per stage on one MI355X.

Two shapes, 100 000 samples each, data and codebook from the seeded mixture stream (the data its first rows, the codebook
the rows behind them):
  gas   256 units x dim 128 at K = 256 (what the first epoch of a default run takes) and at K = 1 (the last)
  c3    10 000 x 256 (the LVQ bench configuration c3) at K = 256: neural gas truncated at the 256 nearest units

Per case one epoch of somhip_ng_train with the ranks fixed, best of `--reps` by the host clock after one warm-up call, its
stages from HIP events: search = every launch of the k-NN search (the published kernel table and somhip_knn_timing),
entries + group, sums and update from somhip_ng_timing.  Beside the sums: the bytes of data rows they read,
n * K * dim * 4, and the rate that implies.  --out FILE also writes the lines there."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name: (units, dim, centres of the mixture, seed of the stream, the ranks timed)
    "gas": (256, 128, 16, 1234, (256, 1)),
    "c3": (10000, 256, 100, 2345, (256,)),
}
SAMPLES = 100000


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="gas,c3")
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
    for name in a.cases.split(","):
        units, dim, centres, seed, ranks = CASES[name]
        ds = E.Dataset(eng, generate=(seed, centres, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, centres, dim, n, units))
        codes = src.rows(0, units)
        src.close()
        cb = E.Codebook(eng, codes)
        say("%s: %d x %d codebook, %d samples" % (name, units, dim, n))
        for K in ranks:
            best = None
            for rep in range(a.reps + 1):
                cb.upload(codes)
                eng.timing(True)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                E.ng_train(cb, ds, 1, ranks=K, qerror=False)
                wall = (time.perf_counter() - t0) * 1e3
                t = eng.ng_timing()
                search = sum(ms for _, ms in eng.timing_table().values()) + sum(ms for _, ms in eng.knn_timing().values())
                eng.timing(False)
                if rep and (best is None or wall < best[0]):
                    best = (wall, search, t)
            wall, search, t = best
            moved = float(n) * min(K, units) * dim * 4
            sums_ms = t["k_ng_sums"][1]
            say("  K = %3d  epoch (best of %d by the host clock) %9.3f ms; search %.3f, entries + group %.3f, sums %.3f, update %.3f ms"
                % (K, a.reps, wall, search, t["group"][1], sums_ms, t["k_ng_update"][1]))
            mean_list = float(n) * min(K, units) / units
            say("           sums: %d launches, %.3f GB of data rows read, %.1f GB/s; a unit's list has %.0f entries on average: "
                "%.1f ns per entry if one list were the whole time" % (t["k_ng_sums"][0], moved / 1e9, moved / 1e6 / sums_ms, mean_list,
                                                                      sums_ms * 1e6 / mean_list))
        cb.close()
        ds.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
