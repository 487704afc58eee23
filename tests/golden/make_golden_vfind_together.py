#!/usr/bin/env python3
"""Generate tests/golden/vfind_together/ from the REAL reference's vfind (oracle/_ref, built from the reference by
oracle/Makefile): nine trials each of two of the cases tests/test_vfind_together.py runs.

Run in the build container only:   python tests/golden/make_golden_vfind_together.py

  expected.json    per case: the arguments, the answers given on stdin (file names relative to the run's directory),
                   the per-trial error lines of stderr, the last line of stdout
  <case>.cod       the map the reference saved

Only answers and results are kept; the inputs are tests/golden/data.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_tool  # noqa: E402

DATA = os.path.join(HERE, "data")
OUT = os.path.join(HERE, "vfind_together")

# trials, data, test, out, topology, neighbourhood, xdim, ydim, length / alpha / radius of the two parts
CASES = {
    "hexa_bubble": {"args": [], "data": "ex.dat",
                    "answers": ["9", "{data}", "{data}", "{out}", "hexa", "bubble", "6", "5", "300", "0.05", "5", "700", "0.02", "2"]},
    "fixed_weights": {"args": ["-fixed", "1", "-weights", "1"], "data": "ex_fts.dat",
                      "answers": ["9", "{data}", "{data}", "{out}", "hexa", "bubble", "6", "5", "300", "0.05", "5", "700", "0.02", "2"]},
}


def main():
    os.makedirs(OUT, exist_ok=True)
    exp = {}
    for tag, case in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(os.path.join(DATA, case["data"]), os.path.join(tmp, case["data"]))
            ans = "\n".join(a.format(data=case["data"], out="out.cod") for a in case["answers"]) + "\n"
            p = subprocess.run([ref_tool("vfind")] + case["args"], input=ans, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, cwd=tmp)
            assert p.returncode == 0, p.stderr
            shutil.copy(os.path.join(tmp, "out.cod"), os.path.join(OUT, tag + ".cod"))
            exp[tag] = {"args": case["args"], "data": case["data"], "answers": case["answers"],
                        "trials_stderr": [ln for ln in p.stderr.splitlines() if ": " in ln and ln.strip()[:1].isdigit()],
                        "last_stdout_line": p.stdout.strip().splitlines()[-1]}
            assert len(exp[tag]["trials_stderr"]) == 9, p.stderr
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(exp, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
