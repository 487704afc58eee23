#!/usr/bin/env python3
"""Generate the mindist / stddev fixtures from the REAL reference (its mindist.c and stddev.c, compiled where they lie
with oracle/Makefile's flags into a temporary directory; nothing of them is kept).

Run in the build container only:   python tests/golden/make_golden_classdist.py

  classdist/expected.json   md5 of every input, and per run: tool, arguments, stdout, return code

Inputs are fixtures of tests/golden/cli and tests/golden/data or are made by tests/classdist_replay.py write_generated()
(NOT stored: the tests make them again and check their md5).  Runs use file names relative to their working directory.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import classdist_replay  # noqa: E402

REF = os.environ.get("SOM_PAK_REFERENCE", "/root/reference")
CLI = os.path.join(HERE, "cli")
DATA = os.path.join(HERE, "data")
OUT = os.path.join(HERE, "classdist")
OBJECTS = ["lvq_rout", "lvq_pak", "fileio", "labels", "datafile", "version"]
REFFLAGS = ["-O3", "-w", "-ffp-contract=off"]          # oracle/Makefile
STORED = {"lvq_olvq1.cod": CLI, "ex1.dat": DATA}


def cases():
    """tag -> (tool, arguments)"""
    return {
        "mindist_cod": ("mindist", ["-cin", "lvq_olvq1.cod"]),
        "mindist_cod_din": ("mindist", ["-cin", "lvq_olvq1.cod", "-din", "ex1_noF.dat"]),
        "mindist_cod_din_buffer": ("mindist", ["-cin", "lvq_olvq1.cod", "-din", "ex1_noF.dat", "-buffer", "10"]),
        "mindist_ex1_self": ("mindist", ["-cin", "ex1.dat", "-din", "ex1.dat"]),
        "mindist_scaled": ("mindist", ["-cin", "scaled.dat"]),
        "mindist_masked_self": ("mindist", ["-cin", "masked.dat", "-din", "masked.dat"]),
        "stddev_ex1": ("stddev", ["-din", "ex1.dat"]),
        "stddev_scaled": ("stddev", ["-din", "scaled.dat"]),
        "stddev_masked": ("stddev", ["-din", "masked.dat"]),
    }


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def build_reference(tmp, tool):
    exe = os.path.join(tmp, "ref_" + tool)
    subprocess.check_call(["gcc"] + REFFLAGS + ["-I", REF] + [os.path.join(REF, o + ".c") for o in [tool] + OBJECTS] +
                          ["-o", exe, "-lm"])
    return exe


def main():
    tmp = tempfile.mkdtemp()
    exe = {tool: build_reference(tmp, tool) for tool in ("mindist", "stddev")}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    classdist_replay.write_generated(work, DATA)
    for name, src in STORED.items():
        shutil.copy(os.path.join(src, name), os.path.join(work, name))
    os.makedirs(OUT, exist_ok=True)
    names = sorted(list(STORED) + list(classdist_replay.GENERATED))
    exp = {"inputs": {name: md5(os.path.join(work, name)) for name in names}, "runs": {}}
    for tag, (tool, args) in cases().items():
        p = subprocess.run([exe[tool]] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=work)
        if p.returncode != 0:
            raise RuntimeError("%s %s failed: %s" % (tool, args, p.stderr))
        assert "nan" not in p.stdout.lower() and "inf" not in p.stdout.lower().replace("in class", ""), tag
        exp["runs"][tag] = {"tool": tool, "args": args, "stdout": p.stdout, "returncode": p.returncode}
    shutil.rmtree(tmp)
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
