#!/usr/bin/env python3
"""Randomised sweep of update mode gemm against the exact kernels (which equal the batch oracle bit for bit): random map
shapes (8x8-patch order and linear), dims in whole 128s, batch lengths that are no multiple of a chunk, bubble and gaussian
neighbourhoods, several batches per run with the rate decaying to zero inside the schedule.  Same winners in the first batch;
the codebooks within fp32 rounding of each other (later batches see slightly different codebooks, so their winners may differ
at ties -- the runs are therefore compared batch by batch from the SAME start).   python tools/fuzz_gemm.py [seconds] [seed]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from som_lvq_pak_amd import engine as E  # noqa: E402
from helpers.som_replay import replay  # noqa: E402


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    rs = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    eng = E.Engine(0)
    t0, n, worst, worst_pair = time.time(), 0, 0.0, 0.0
    while time.time() - t0 < budget:
        xd, yd = [int(v) for v in rs.choice([6, 8, 12, 16, 24, 32, 40, 64], 2)]
        d = int(rs.choice([128, 256, 384, 512]))
        topol, neigh = int(rs.choice([3, 4])), int(rs.choice([1, 2]))
        B = int(rs.choice([17, 100, 255, 256, 600, 1000, 2049, 4096]))
        nvec = int(rs.choice([B, 2 * B + 3, 5000]))
        radius = float(rs.uniform(0.6, max(xd, yd)))
        alpha = float(rs.choice([0.02, 0.05, 0.3, 0.9]))
        length = int(rs.choice([B, 4 * B, 64 * B]))
        ds = E.Dataset(eng, generate=(int(rs.randint(1, 1 << 30)), int(rs.randint(1, 12)), d, 0, nvec))
        lo, hi, cnt = E.column_minmax(ds)
        init = E.randinit_from_bbox(lo, hi, cnt, xd, yd, int(rs.randint(1, 1000)))
        ds_rows = ds.rows(0, nvec)
        it0 = int(rs.randint(0, max(1, length - B + 1)))
        got = {}
        for mode in ("exact", "gemm"):
            eng.set_update_mode(mode)
            cb = E.Codebook(eng, init, topol, neigh, xd, yd)
            ti, _ = E.som_train(cb, ds, length, alpha, radius, batch=B, start_iter=it0, count=min(B - it0 % B, length - it0))
            got[mode] = (cb.download(), ti)
            cb.close()
        eng.set_update_mode("exact")
        ds.close()
        a, b = got["exact"][0], got["gemm"][0]
        case = (xd, yd, d, topol, neigh, B, nvec, radius, alpha, length, it0)
        assert np.array_equal(got["exact"][1], got["gemm"][1]), case
        assert np.isfinite(b).all(), case
        scale = float(np.abs(a).max())
        err = float(np.abs(a - b).max()) / scale
        # the yardstick: a float64 replay of the batch on a few units (tests/helpers/som_replay.py: the reference's own
        # float arithmetic for radii, rates and lattice distances, so no unit on a neighbourhood's rim is decided the
        # other way; the exact kernels' fp32 chain of thousands of hits has an error of its own, as large as the GEMM's)
        units = rs.choice(xd * yd, min(48, xd * yd), replace=False)
        win = got["exact"][1]
        cnt_it = len(win)
        c = replay(init, xd, yd, topol, neigh, ds_rows, length, alpha, radius, win, start_iter=it0, count=cnt_it,
                   dtype=np.float64, units=units).codes
        e_exact = float(np.abs(a[units] - c).max()) / scale
        e_gemm = float(np.abs(b[units] - c).max()) / scale
        worst = max(worst, e_gemm)
        worst_pair = max(worst_pair, err)
        # a sum of k products accumulated in fp32 carries ~ sqrt(k) 2^-24 of the magnitude of the sum (the exact kernels'
        # chain is contractive -- every step damps the earlier roundings by 1 - a -- and stays near 1e-6)
        # (e_gemm is the LARGEST of ~20 000 element errors: about four standard deviations of a random walk of k roundings
        # of a sum a few times the scale -- hence the factor 12)
        allow = max(2.0 * e_exact, 12.0 * np.sqrt(cnt_it) * 5.96e-8, 3e-6)
        assert e_gemm <= allow, (case, e_exact, e_gemm, allow)
        assert err <= max(2.0 * allow, 10.0 * (e_exact + e_gemm), 2e-5), (case, err, e_exact, e_gemm)   # all units: the sample may miss the worst
        n += 1
        if n % 20 == 0:
            print("%d cases, worst error of the gemm result against the float64 replay %.2e of the scale, against the exact kernels %.2e" % (n, worst, worst_pair), flush=True)
    print("fuzz gemm ok: %d cases in %.0f s, worst error of the gemm result against a float64 replay %.2e of the scale (bound per case: 12 sqrt(hits) 2^-24, or twice the exact kernels' own error); largest difference between the gemm and the exact kernels %.2e of the scale" % (n, time.time() - t0, worst, worst_pair))


if __name__ == "__main__":
    main()
