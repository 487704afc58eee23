#!/usr/bin/env python3
"""somhip_umatrix at the headline shape (256 x 256 x 512, hexa and rect, both filters) beside the plain host loop
tools/umatrix_host_loop.c over the same rows: per-kernel times from the engine's HIP-event table, the entry point's wall
time, k_umat_dist's bytes per second against one read of the codebook at HBM speed, and the equality of the two results.

  gcc -O3 -ffp-contract=off -o build/umatrix_host_loop tools/umatrix_host_loop.c -lm
  python tools/umatrix_measure.py [--out profiles/umatrix_vs_host.txt] [--rounds 7]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from som_lvq_pak_amd import engine as E  # noqa: E402

HBM_MEASURED = 6.29e12          # bytes per second, float4 copy on an MI355X
MX, MY, DIM = 256, 256, 512
KERNELS = ["k_umat_dist", "k_umat_units", "k_umat_minmax", "k_umat_scale", "k_umat_average", "k_umat_median"]


def fnv(u):
    h = 1469598103934665603
    for b in u.view(np.uint32).ravel().tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-loop", default=os.path.join(ROOT, "build", "umatrix_host_loop"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rows = np.random.RandomState(1).standard_normal((MX * MY, DIM)).astype(np.float32)
    tile_bytes = MX * MY * DIM * 4
    floor_us = tile_bytes / HBM_MEASURED * 1e6
    say("# somhip_umatrix against a plain host loop; %d x %d x %d, seeded normal rows, filters = average + median" % (MX, MY, DIM))
    say("# one read of the codebook: %d bytes (%.0f MiB); at %.2f TB/s (float4 copy, measured) that is %.1f us: k_umat_dist's floor"
        % (tile_bytes, tile_bytes / 2 ** 20, HBM_MEASURED / 1e12, floor_us))
    eng = E.Engine(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "rows.f32")
    rows.tofile(path)
    for name, topol in (("hexa", E.TOPOL_HEXA), ("rect", E.TOPOL_RECT)):
        cb = E.Codebook(eng, rows, topol, E.NEIGH_BUBBLE, MX, MY)
        u, mm = E.umatrix(cb, True, True)                       # warm-up: code objects, scratch
        say()
        say("## %s: per kernel, HIP events around each launch, %d calls after one warm-up call" % (name, a.rounds))
        eng.timing(True)
        eng.timing_reset()
        for _ in range(a.rounds):
            E.umatrix(cb, True, True)
        table = eng.timing_table()
        eng.timing(False)
        for k in KERNELS:
            n, ms = table[k]
            say("%-16s %3d launches, mean %9.1f us" % (k, n, 1e3 * ms / max(n, 1)))
        dist_us = 1e3 * table["k_umat_dist"][1] / table["k_umat_dist"][0]
        pairs = (4 if name == "rect" else 3) * MX * MY
        say("k_umat_dist: %.1f us = %.2f x the floor; the codebook's bytes once over that time: %.2f TB/s; with both rows of every"
            % (dist_us, dist_us / floor_us, tile_bytes / dist_us / 1e6))
        say("  pair (about %d pairs x 2 rows x %d bytes, most of it served by the caches): %.2f TB/s at the load instructions"
            % (pairs, DIM * 4, pairs * 2 * DIM * 4 / dist_us / 1e6))
        walls = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            E.umatrix(cb, True, True)
            walls.append(1e3 * (time.perf_counter() - t0))
        say("entry point wall time, timing off (launches, the min/max read-back, %d bytes of result back): median %.3f ms, min %.3f ms, max %.3f ms"
            % (u.nbytes, float(np.median(walls)), min(walls), max(walls)))
        if os.path.exists(a.host_loop):
            p = subprocess.run([a.host_loop, path, str(MX), str(MY), str(DIM), name], stdout=subprocess.PIPE, text=True, check=True)
            say(p.stdout.strip())
            same = p.stdout.strip().rsplit(" ", 1)[1] == fnv(u)
            say("engine: min %.9g max %.9g; hash %s -> %s" % (mm[0], mm[1], fnv(u), "the same bits" if same else "DIFFERENT"))
        else:
            say("(host loop %s not built)" % a.host_loop)
        cb.close()
    os.remove(path)
    os.rmdir(tmp)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
