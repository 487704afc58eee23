#!/usr/bin/env python3
"""Record what the REAL reference's knntest (oracle/_ref, built from /root/reference) prints for more than 8 neighbours.

Run in the build container only:   python tests/golden/make_golden_knn_wide.py

  knn_wide/expected.json   knntest's stdout for -knn 9 and -knn 21
                           "ex2":        data/ex2.dat against cli/lvq_olvq1.cod
                           "ex2_masked": ex2_masked.dat (not stored: make_golden_masked.write_masked_data() makes it
                                         again, and masked/expected.json holds its md5) against masked/olvq1.cod

No other fixture is touched.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import build, ref_tool  # noqa: E402
from make_golden_masked import write_masked_data  # noqa: E402

OUT = os.path.join(HERE, "knn_wide")
KNNS = (9, 21)


def cases(masked_dir):
    """name -> (data file, codebook)"""
    return {"ex2": (os.path.join(HERE, "data", "ex2.dat"), os.path.join(HERE, "cli", "lvq_olvq1.cod")),
            "ex2_masked": (os.path.join(masked_dir, "ex2_masked.dat"), os.path.join(HERE, "masked", "olvq1.cod"))}


def knntest(exe, din, cin, knn, *extra):
    return subprocess.run([exe, "-din", din, "-cin", cin, "-knn", str(knn)] + [str(a) for a in extra],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def main():
    build()
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    write_masked_data(tmp)
    exp = {}
    for name, (din, cin) in cases(tmp).items():
        exp[name] = {}
        for knn in KNNS:
            p = knntest(ref_tool("knntest"), din, cin, knn, "-v", 0)
            if p.returncode != 0:
                raise RuntimeError("knntest -knn %d on %s failed: %s" % (knn, name, p.stderr))
            exp[name][str(knn)] = p.stdout
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
