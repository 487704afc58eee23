#!/usr/bin/env python3
"""Generate the fixtures of tests/test_masked_lvq_batched.py from the REAL reference (oracle/_ref).

Run in the build container only:   python tests/golden/make_golden_masked_batch.py

A size the ex1 fixtures of tests/golden/masked do not reach: a seeded 100-class mixture, 5 000 data rows x 64
components with about 10 % of the components `x`, a codebook of 2 000 rows (the first 2 000 data rows, unmasked),
20 000 iterations of lvq1 / olvq1 / lvq2 / lvq3.  Nothing but masked_batch/expected.json is stored: write_case() makes
the two input files again from the seed (the tests check their md5), and only the md5 of what the reference wrote for
each run is recorded.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "masked_batch")

CLASSES, DIM, ROWS, CODES, RLEN = 100, 64, 5000, 2000, 20000
RUNS = {
    "lvq1": ["-rlen", RLEN, "-alpha", 0.05],
    "olvq1": ["-rlen", RLEN, "-alpha", 0.3],
    "lvq2": ["-rlen", RLEN, "-alpha", 0.05, "-win", 0.3],
    "lvq3": ["-rlen", RLEN, "-alpha", 0.05, "-win", 0.3, "-epsilon", 0.1],
}


def case_arrays():
    """x [ROWS][DIM], labels, mask (about 10 %, no row fully masked), codes = the first CODES rows as they are"""
    rs = np.random.RandomState(4242)
    cent = (4.0 * rs.standard_normal((CLASSES, DIM))).astype(np.float32)
    which = rs.randint(0, CLASSES, ROWS)
    x = (cent[which] + rs.standard_normal((ROWS, DIM)).astype(np.float32)).astype(np.float32)
    mask = rs.random_sample((ROWS, DIM)) < 0.10
    mask[mask.all(axis=1), 0] = False
    return x, ["c%d" % v for v in which], mask


def write_entries(path, x, lab, mask=None):
    with open(path, "w") as f:
        f.write("%d\n" % x.shape[1])
        for r in range(x.shape[0]):
            f.write(" ".join("x" if mask is not None and mask[r, i] else "%g" % x[r, i] for i in range(x.shape[1])))
            f.write(" %s\n" % lab[r])


def write_case(dst):
    """mix_masked.dat and mix.cod into directory dst"""
    x, lab, mask = case_arrays()
    write_entries(os.path.join(dst, "mix_masked.dat"), x, lab, mask)
    write_entries(os.path.join(dst, "mix.cod"), x[:CODES], lab[:CODES])


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def main():
    sys.path.insert(0, ROOT)
    from oracle import build, ref_tool
    build()
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    write_case(tmp)
    exp = {"data": {f: md5(os.path.join(tmp, f)) for f in ("mix_masked.dat", "mix.cod")}, "runs": {}}
    for tag, args in RUNS.items():
        out = os.path.join(tmp, tag + ".cod")
        cmd = [ref_tool(tag), "-din", os.path.join(tmp, "mix_masked.dat"), "-cin", os.path.join(tmp, "mix.cod"), "-cout", out]
        p = subprocess.run(cmd + [str(a) for a in args] + ["-v", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise RuntimeError("%s failed: %s" % (cmd, p.stderr))
        exp["runs"][tag] = {"tool": tag, "args": [str(a) for a in args], "md5": md5(out)}
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
