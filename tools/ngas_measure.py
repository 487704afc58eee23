#!/usr/bin/env python3
"""Times batch neural gas (somhip_ng_train, K10) per stage on one MI355X, and with --dense its dense form
(somhip_ng_train_dense, K10d) beside it.

Two shapes, 100 000 samples each, data and codebook from the seeded mixture stream (the data its first rows, the codebook
the rows behind them):
  gas   256 units x dim 128 at K = 256 (what the first epoch of a default run takes) and at K = 1 (the last)
  c3    10 000 x 256 (the LVQ bench configuration c3) at K = 256: neural gas truncated at the 256 nearest units
  gas1k, gas4k   1024 and 4096 units x dim 128 at K = 256: the truncated form at the sizes the dense one is for

Per case one epoch of somhip_ng_train with the ranks fixed, best of `--reps` by the host clock after one warm-up call, its
stages from HIP events: search = every launch of the k-NN search (the published kernel table and somhip_knn_timing),
entries + group, sums and update from somhip_ng_timing.  Beside the sums: the bytes of data rows they read,
n * K * dim * 4, and the rate that implies.

--dense: behind every case of at most 4096 units one epoch of somhip_ng_train_dense under the same protocol, its stages
from somhip_ng_dense_timing (distances, the ranking kernel, the sums) and K10's update; beside the ranking kernel the
compare-exchanges of its bitonic network, P / 2 * log2(P) (log2(P) + 1) / 2 per sample over P = the next power of two,
and the LDS bytes they move (two 8-byte loads each, two 8-byte stores where the pair was out of order: half of them on
average), with the rates both imply.  --finding T: what truncation changes on one run -- T epochs of both forms from the
same start on the gas1k case, the quantization error before every epoch and of the codebook each run ends with.
--out FILE also writes the lines there."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name: (units, dim, centres of the mixture, seed of the stream, the ranks timed)
    "gas": (256, 128, 16, 1234, (256, 1)),
    "c3": (10000, 256, 100, 2345, (256,)),
    "gas1k": (1024, 128, 16, 1234, (256,)),
    "gas4k": (4096, 128, 16, 1234, (256,)),
}
SAMPLES = 100000


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="gas,c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--dense", action="store_true", help="time somhip_ng_train_dense beside every case it takes")
    ap.add_argument("--finding", type=int, default=0, metavar="T", help="T epochs of both forms from one start at 1024 x 128")
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
        if a.dense and units <= E.NG_DENSE_MAX:
            best = None
            for rep in range(a.reps + 1):
                cb.upload(codes)
                eng.timing(True)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                E.ng_train_dense(cb, ds, 1, qerror=False)
                wall = (time.perf_counter() - t0) * 1e3
                t, upd = eng.ng_dense_timing(), eng.ng_timing()["k_ng_update"][1]
                eng.timing(False)
                if rep and (best is None or wall < best[0]):
                    best = (wall, t, upd)
            wall, t, upd = best
            rank_ms = t["k_ng_dense_weights"][1]
            say("  dense    epoch (best of %d by the host clock) %9.3f ms; distances %.3f, ranking %.3f, sums %.3f, update %.3f ms"
                % (a.reps, wall, t["distances"][1], rank_ms, t["sums"][1], upd))
            P, lg = 1, 0
            while P < units:
                P, lg = 2 * P, lg + 1
            cex = float(n) * (P // 2) * lg * (lg + 1) / 2
            lds = cex * (16 + 8)
            say("           ranking: %d launches, %d steps of %d compare-exchanges a sample: %.3g compare-exchanges, %.1f G/s; "
                "%.3f TB through LDS, %.2f TB/s" % (t["k_ng_dense_weights"][0], lg * (lg + 1) // 2, P // 2, cex, cex / 1e6 / max(rank_ms, 1e-9),
                                                    lds / 1e12, lds / 1e9 / max(rank_ms, 1e-9)))
            flop = 2.0 * n * units * (dim + 1)
            say("           sums: %.3g useful fp64 flop, %.2f Tflop/s; Q: %.3f GB written and read"
                % (flop, flop / 1e9 / max(t["sums"][1], 1e-9), float(n) * ((units + 63) // 64 * 64) * 8 / 1e9))
        cb.close()
        ds.close()
    if a.finding > 0:
        units, dim, centres, seed, _ = CASES["gas1k"]
        T = a.finding
        ds = E.Dataset(eng, generate=(seed, centres, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, centres, dim, n, units))
        codes = src.rows(0, units)
        src.close()
        cb = E.Codebook(eng, codes)
        say("finding: %d epochs from one start, %d x %d, %d samples of gen:k=%d,dim=%d,seed=%d (default lambda: 128 down to 0.01)"
            % (T, units, dim, n, centres, dim, seed))
        for form, train in (("bng", E.ng_train), ("bng -dense", E.ng_train_dense)):
            cb.upload(codes)
            q = train(cb, ds, T)
            last = train(cb, ds, 1, 0.01, 0.01)[0]                     # (the q of the codebook the run ended with)
            say("  %-10s qerror per sample before epochs 0, %d, %d: %.6f %.6f %.6f; of the final codebook: %.6f"
                % (form, T // 2, T - 1, q[0] / n, q[T // 2] / n, q[T - 1] / n, last / n))
        cb.close()
        ds.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
