#!/usr/bin/env python3
"""Masked against unmasked data through the command-line tools: LVQ1 and OLVQ1 training and `knntest -knn 5`, the
engine's tools (som_lvq_pak_amd/host/bin) beside the reference's CPU tools built into oracle/_ref, on the same files.

  python tools/masked_lvq_bench.py [--quick]

Shapes: ex1 (200 codes x 20, the masked fixtures of tests/golden) and BASELINE configs[2]'s codebook (10 000 codes x
256, a seeded 100-class mixture, 10 000 data rows; the masked copy has about 10 % of its components set to `x`).
Every figure is a slope between two runs of one tool that differ only in -rlen (or in the number of data rows), so
start-up and file parsing drop out: microseconds per LVQ iteration, per k-NN sample.  Each run is the best of three
(process start-up on the GPU varies by tens of milliseconds).  Run on a GPU box after build()."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
REF = os.path.join(ROOT, "oracle", "_ref")
DATA = os.path.join(ROOT, "tests", "golden", "data")
MASKED = os.path.join(ROOT, "tests", "golden", "masked")


def wall(exe, args, limit=900, repeat=3):
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        p = subprocess.run([exe] + [str(a) for a in args] + ["-v", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=limit)
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            raise SystemExit("%s %s failed (%d): %s" % (exe, " ".join(map(str, args)), p.returncode, p.stderr[-400:]))
        best = dt if best is None else min(best, dt)
    return best


def write_dat(path, x, lab, mask=None):
    with open(path, "w") as f:
        f.write("%d\n" % x.shape[1])
        for r in range(x.shape[0]):
            vals = ["x" if mask is not None and mask[r, i] else "%g" % x[r, i] for i in range(x.shape[1])]
            f.write(" ".join(vals) + " %s\n" % lab[r])


def mask_of(shape, seed, frac=0.10):
    m = np.random.RandomState(seed).random_sample(shape) < frac
    m[m.all(axis=1), 0] = False
    return m


def slope(exe, args_of, n0, n1):
    """seconds per unit between n0 and n1 units (the tool run twice)"""
    return (wall(exe, args_of(n1)) - wall(exe, args_of(n0))) / (n1 - n0)


def case(name, tmp, files, rlen, nknn):
    """files: {"plain": (data, codes, knn data small, knn data big), "masked": (...)}; rlen / nknn: {side: (n0, n1)}"""
    for kind, alpha in (("lvq1", 0.05), ("olvq1", 0.3)):
        for data in ("plain", "masked"):
            din, cin = files[data][0], files[data][1]
            row = []
            for side, root in (("engine", BIN), ("reference CPU", REF)):
                out = os.path.join(tmp, "o.cod")
                n0, n1 = rlen[side]
                s = slope(os.path.join(root, kind), lambda n: ["-din", din, "-cin", cin, "-cout", out, "-rlen", n,
                                                               "-alpha", alpha], n0, n1)
                row.append("%s %.2f us/iter" % (side, 1e6 * s))
            print("%-8s %-6s %-7s %s" % (name, kind, data, "  ".join(row)), flush=True)
    for data in ("plain", "masked"):
        _, cin, small, big = files[data]
        row = []
        for side, root in (("engine", BIN), ("reference CPU", REF)):
            exe = os.path.join(root, "knntest")
            t = (wall(exe, ["-din", big, "-cin", cin, "-knn", 5]) - wall(exe, ["-din", small, "-cin", cin, "-knn", 5])) / nknn
            row.append("%s %.2f us/sample" % (side, 1e6 * t))
        print("%-8s %-6s %-7s %s" % (name, "knn5", data, "  ".join(row)), flush=True)


def main():
    quick = "--quick" in sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        # ---- ex1: the fixtures (masked codes carry `x` of their own: eveninit picked them from the masked data)
        import importlib.util
        from som_lvq_pak_amd import textio
        spec = importlib.util.spec_from_file_location("make_golden_masked", os.path.join(ROOT, "tests", "golden",
                                                                                          "make_golden_masked.py"))
        golden = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(golden)
        golden.write_masked_data(tmp)                       # ex1_masked.dat / ex2_masked.dat, as the fixtures were made
        e2, tab = textio.read_entries(os.path.join(DATA, "ex2.dat"))
        e2m, _ = textio.read_entries(os.path.join(tmp, "ex2_masked.dat"), tab)
        half = e2.points.shape[0] // 2
        files = {}
        for tag, e, din, cin in (("plain", e2, os.path.join(DATA, "ex1.dat"), os.path.join(ROOT, "tests", "golden", "cli", "lvq_init.cod")),
                                 ("masked", e2m, os.path.join(tmp, "ex1_masked.dat"), os.path.join(MASKED, "eveninit_knn5.cod"))):
            lab = [tab.to_label(int(v)) for v in e.first_label]
            small, big = os.path.join(tmp, "k%s_s.dat" % tag), os.path.join(tmp, "k%s_b.dat" % tag)
            write_dat(small, e.points[:half], lab[:half], None if e.mask is None else e.mask[:half])
            write_dat(big, e.points, lab, e.mask)
            files[tag] = (din, cin, small, big)
        n = 5000 if quick else 20000
        case("ex1", tmp, files, {"engine": (n, 10 * n), "reference CPU": (n, 3 * n)}, e2.points.shape[0] - half)
        # ---- configs[2]'s codebook: 10 000 x 256
        rs = np.random.RandomState(2345)
        k, dim, nvec, ncodes = 100, 256, 10000, 10000
        cent = (4.0 * rs.standard_normal((k, dim))).astype(np.float32)
        lab = ["c%d" % v for v in rs.randint(0, k, nvec)]
        x = (cent[[int(v[1:]) for v in lab]] + rs.standard_normal((nvec, dim)).astype(np.float32)).astype(np.float32)
        codes, clab = x[:ncodes], lab[:ncodes]
        m = mask_of(x.shape, 7)
        cod = os.path.join(tmp, "c2.cod")
        write_dat(cod, codes, clab)
        nk0, nk1 = (200, 400) if quick else (1000, 5000)
        files = {}
        for tag, mask in (("plain", None), ("masked", m)):
            din = os.path.join(tmp, "c2_%s.dat" % tag)
            write_dat(din, x, lab, mask)
            small, big = os.path.join(tmp, "c2k_%s_s.dat" % tag), os.path.join(tmp, "c2k_%s_b.dat" % tag)
            write_dat(small, x[:nk0], lab[:nk0], None if mask is None else mask[:nk0])
            write_dat(big, x[:nk1], lab[:nk1], None if mask is None else mask[:nk1])
            files[tag] = (din, cod, small, big)
        g, r = (1000, 3000) if quick else (5000, 45000), (100, 300) if quick else (500, 1500)
        case("10000x256", tmp, files, {"engine": g, "reference CPU": r}, nk1 - nk0)


if __name__ == "__main__":
    main()
