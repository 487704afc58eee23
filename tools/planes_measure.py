#!/usr/bin/env python3
"""somhip_planes at the headline shape (256 x 256 x 512, all planes, and one 64 MiB window of them) beside the plain host
loop tools/planes_host_loop.c over the same rows: the entry point's wall time, the pass's own floor (the rows read twice,
the planes written once, at HBM speed) and the equality of the two results.  The three kernels have no ids in the engine's
HIP-event table (the table is closed); their times come from a kernel trace of this script:

  gcc -O3 -ffp-contract=off -o build/planes_host_loop tools/planes_host_loop.c
  python tools/planes_measure.py [--out profiles/planes_vs_host.txt] [--rounds 7]
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/planes_measure.py --rounds 5
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-loop", default=os.path.join(ROOT, "build", "planes_host_loop"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n = MX * MY
    rs = np.random.RandomState(1)
    rows = (rs.standard_normal((n, DIM)) * 10.0 ** rs.uniform(-2, 2, size=DIM) + rs.uniform(-20, 20, size=DIM)).astype(np.float32)
    tile_bytes = n * DIM * 4
    say("# somhip_planes against a plain host loop; %d x %d x %d, seeded normal rows, per-component scales and offsets" % (MX, MY, DIM))
    say("# the pass's floor: the rows read twice and the planes written once = 3 x %d bytes (%.0f MiB each); at %.2f TB/s"
        % (tile_bytes, tile_bytes / 2 ** 20, HBM_MEASURED / 1e12))
    say("# (float4 copy, measured) that is %.1f us: %.1f us for k_planes_minmax (one read), %.1f us for k_planes_grey (read + write)"
        % (3 * tile_bytes / HBM_MEASURED * 1e6, tile_bytes / HBM_MEASURED * 1e6, 2 * tile_bytes / HBM_MEASURED * 1e6))
    eng = E.Engine(0)
    cb = E.Codebook(eng, rows, E.TOPOL_HEXA, E.NEIGH_BUBBLE, MX, MY)
    window = max(1, (64 << 20) // (4 * n))
    got = None
    for label, first, count in (("all %d planes" % DIM, 0, DIM), ("one window of %d planes (64 MiB)" % window, 0, window)):
        got = E.planes(cb, first, count)                        # warm-up: code objects, scratch
        walls = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            E.planes(cb, first, count)
            walls.append(1e3 * (time.perf_counter() - t0))
        back = got[0].nbytes
        med = float(np.median(walls))
        say("entry point wall time, %s (3 launches, %d bytes of grey levels back to pageable host memory): median %.3f ms, "
            "min %.3f ms, max %.3f ms; the result's bytes over the median: %.1f GB/s"
            % (label, back, med, min(walls), max(walls), back / med / 1e6))
    whole = E.planes(cb)
    if os.path.exists(a.host_loop):
        tmp = tempfile.mkdtemp()
        path, out = os.path.join(tmp, "rows.f32"), os.path.join(tmp, "grey.f32")
        cb.download().tofile(path)
        p = subprocess.run([a.host_loop, path, str(n), str(DIM), out], stdout=subprocess.PIPE, text=True, check=True)
        say(p.stdout.strip())
        host = np.fromfile(out, dtype=np.float32).reshape(DIM, n)
        same = np.array_equal(host.view(np.uint32), whole[0].view(np.uint32))
        say("engine against the host loop, %d grey levels: %s" % (host.size, "the same bits" if same else "DIFFERENT"))
        os.remove(path)
        os.remove(out)
        os.rmdir(tmp)
    else:
        say("(host loop %s not built)" % a.host_loop)
    cb.close()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
