#!/usr/bin/env python3
"""Generate the masked-data LVQ / k-NN fixtures from the REAL reference (oracle/_ref, built from /root/reference).

Run in the build container only:   python tests/golden/make_golden_masked.py

  ex1_masked.dat, ex2_masked.dat (NOT stored: write_masked_data() makes them again, the tests check their md5)
                  data/ex1.dat / ex2.dat with about 10 % of the components replaced by `x` (seeded; comment lines
                  kept; no row has every component masked, so the reference's readers keep every row)
  masked/eveninit_knn5.cod, masked/olvq1.cod
                  the two codebooks later runs start from ("%g" text, `x` where a code row carries a mask)
  masked/expected.json   md5 of the masked data and of every codebook the runs wrote, and what the tools printed

make_golden.py and the fixtures it writes are not touched.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import build, ref_tool  # noqa: E402

DATA = os.path.join(HERE, "data")
OUT = os.path.join(HERE, "masked")

# the recorded runs: tag -> (tool, data file, extra arguments)
INIT = {
    "eveninit_knn5": ("eveninit", "ex1_masked.dat", ["-noc", 200, "-knn", 5]),
    "eveninit_knn3": ("eveninit", "ex1_masked.dat", ["-noc", 200, "-knn", 3]),
    "propinit_knn5": ("propinit", "ex1_masked.dat", ["-noc", 200, "-knn", 5]),
    "propinit_knn3": ("propinit", "ex1_masked.dat", ["-noc", 200, "-knn", 3]),
    "elimin_knn5": ("elimin", "ex1_masked.dat", ["-knn", 5]),
}
TRAIN = {      # all from eveninit_knn5.cod (its rows are data rows, `x` included)
    "lvq1": ("lvq1", ["-rlen", 5000, "-alpha", 0.05]),
    "olvq1": ("olvq1", ["-rlen", 5000, "-alpha", 0.3]),
    "lvq2": ("lvq2", ["-rlen", 5000, "-alpha", 0.05, "-win", 0.3]),
    "lvq3": ("lvq3", ["-rlen", 5000, "-alpha", 0.05, "-win", 0.3, "-epsilon", 0.1]),
}


def mask_file(src, dst, seed, frac=0.10):
    """Replace about `frac` of the numeric components of every data line by `x`; header, comment lines and labels are
    kept as they are.  A row that would lose every component keeps its first one."""
    rs = np.random.RandomState(seed)
    lines = open(src).read().split("\n")
    dim = int(lines[0].split()[0])
    out = [lines[0]]
    for ln in lines[1:]:
        tok = ln.split()
        if not tok or ln.lstrip().startswith("#"):
            out.append(ln)
            continue
        m = rs.random_sample(dim) < frac
        if m.all():
            m[0] = False
        out.append(" ".join(("x" if m[i] else t) if i < dim else t for i, t in enumerate(tok)))
    open(dst, "w").write("\n".join(out))


MASKED_DATA = {"ex1_masked.dat": ("ex1.dat", 101), "ex2_masked.dat": ("ex2.dat", 202)}


def write_masked_data(dst):
    """ex1_masked.dat and ex2_masked.dat into directory dst"""
    for name, (src, seed) in MASKED_DATA.items():
        mask_file(os.path.join(DATA, src), os.path.join(dst, name), seed)


def run(tool, *args, env=None):
    cmd = [ref_tool(tool)] + [str(a) for a in args] + ["-v", "0"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=OUT,
                       env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        raise RuntimeError("%s failed: %s" % (cmd, p.stderr))
    return p.stdout


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def main():
    build()
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    write_masked_data(tmp)
    d = lambda f: os.path.join(tmp, f)  # noqa: E731
    exp = {"data": {f: md5(d(f)) for f in MASKED_DATA}, "runs": {}}
    runs = exp["runs"]
    for tag, (tool, data, args) in INIT.items():
        run(tool, "-din", d(data), "-cout", tag + ".cod", *args)
        runs[tag] = {"tool": tool, "din": data, "args": [str(a) for a in args], "out": tag + ".cod",
                     "md5": md5(os.path.join(OUT, tag + ".cod"))}
    for tag, (tool, args) in TRAIN.items():
        out = tag + ".cod"
        run(tool, "-din", d("ex1_masked.dat"), "-cin", "eveninit_knn5.cod", "-cout", out, *args)
        runs[tag] = {"tool": tool, "din": "ex1_masked.dat", "cin": "eveninit_knn5.cod", "args": [str(a) for a in args],
                     "out": out, "md5": md5(os.path.join(OUT, out)),
                     "accuracy_stdout": run("accuracy", "-din", d("ex2_masked.dat"), "-cin", out)}
        assert not os.path.exists(os.path.join(OUT, tag + ".lra"))      # olvq1 writes it, lvqtrain.c:249 removes it
    # balance is not recorded: on every masked input tried it appends codes, and the reference then reads and writes
    # OLVQ1 rates past the end of its array for them (balance.c:188) -- its bytes depend on the heap, or it aborts
    # the scanners on ex2_masked.dat against the masked olvq1 codebook
    t = {}
    t["accuracy"] = run("accuracy", "-din", d("ex2_masked.dat"), "-cin", "olvq1.cod")
    for knn in (1, 3, 5, 8):
        t["knntest_%d" % knn] = run("knntest", "-din", d("ex2_masked.dat"), "-cin", "olvq1.cod", "-knn", knn)
    run("classify", "-din", d("ex2_masked.dat"), "-cin", "olvq1.cod", "-dout", "classify.dat", "-cfout", "classify.cfo")
    t["classify_dout_md5"] = md5(os.path.join(OUT, "classify.dat"))
    t["classify_cfout_md5"] = md5(os.path.join(OUT, "classify.cfo"))
    t["cmatr"] = run("cmatr", "-din", d("ex2_masked.dat"), "-cin", "olvq1.cod", "-cfout", "cmatr.cfo")
    t["cmatr_cfout_md5"] = md5(os.path.join(OUT, "cmatr.cfo"))
    for knn in (3, 5):
        run("setlabel", "-din", d("ex2_masked.dat"), "-cin", "olvq1.cod", "-cout", "setlabel_%d.cod" % knn, "-knn", knn)
        t["setlabel_%d_md5" % knn] = md5(os.path.join(OUT, "setlabel_%d.cod" % knn))
    exp["scan"] = t
    # only the two input codebooks are kept; the rest is in expected.json
    keep = {"eveninit_knn5.cod", "olvq1.cod"}
    shutil.rmtree(tmp)
    for f in os.listdir(OUT):
        if f not in keep and f != "expected.json":
            os.remove(os.path.join(OUT, f))
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
