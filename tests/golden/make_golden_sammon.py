#!/usr/bin/env python3
"""Generate the sammon fixtures from the REAL reference (its sammon.c, compiled where it lies with oracle/Makefile's
flags into a temporary directory; nothing of it is kept).

Run in the build container only:   python tests/golden/make_golden_sammon.py

  sammon/<tag>.cod       what `sammon -cin <input> -cout <tag>.cod -rlen R -rand S ...` wrote (two numbers and the labels
                         of every row)
  sammon/expected.json   md5 of every input, and per run: arguments, stdout (the `-v 2` mapping-error lines), stderr, md5
                         of the .cod and of <tag>_sa.eps / <tag>_sa.ps

Inputs are fixtures of tests/golden/cli or are made by tests/sammon_replay.py write_generated() (NOT stored: the tests
make them again and check their md5).  Runs use file names relative to their working directory, so the recorded stderr
of `-v 2` names no directory.  No recorded output may hold a NaN or an infinity.
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

import sammon_replay  # noqa: E402

REF = os.environ.get("SOM_PAK_REFERENCE", "/root/reference")
CLI = os.path.join(HERE, "cli")
OUT = os.path.join(HERE, "sammon")
OBJECTS = ["sammon", "lvq_pak", "fileio", "labels", "datafile", "version"]
REFFLAGS = ["-O3", "-w", "-ffp-contract=off"]          # oracle/Makefile


def cases():
    """tag -> (input, rlen, seed, extra arguments)"""
    out = {}
    for short, cin in (("hexa", "som_hexa_gaussian.cod"), ("rect", "som_rect_bubble.cod"), ("lvq", "lvq_olvq1.cod")):
        for rlen in (1, 100, 1000):
            for seed in (7, 1234):
                out["%s_r%d_s%d" % (short, rlen, seed)] = (cin, rlen, seed, ["-v", "0"])
    out["seeded_r200_s7"] = ("seeded_35x31x16.cod", 200, 7, ["-v", "0"])
    out["dup_r100_s7_eps"] = ("som_hexa_gaussian_dup.cod", 100, 7, ["-eps", "-v", "0"])
    out["hexa_r100_s7_eps"] = ("som_hexa_gaussian.cod", 100, 7, ["-eps", "-v", "0"])
    out["rect_r100_s1234_ps"] = ("som_rect_bubble.cod", 100, 1234, ["-ps", "-v", "0"])
    out["vcal_r100_s7_eps"] = ("somexample_vcal.cod", 100, 7, ["-eps", "-v", "0"])
    out["lvq_r100_s7_eps"] = ("lvq_olvq1.cod", 100, 7, ["-eps", "-v", "0"])
    out["lvq_r100_s1234_ps"] = ("lvq_olvq1.cod", 100, 1234, ["-ps", "-buffer", "10", "-v", "0"])
    out["hexa_r100_s7_v2"] = ("som_hexa_gaussian.cod", 100, 7, ["-v", "2"])
    # -v 2 prints the mapping error, a sequential fp32 sum over n = noc (noc - 1) / 2 pairs that the engine cannot follow
    # bit for bit; the runs recorded for it keep (n - 1) 2^-24 e below 0.0014 on every line (see tests/test_sammon.py)
    out["vcal_r100_s1234_v2"] = ("somexample_vcal.cod", 100, 1234, ["-v", "2"])
    return out


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def build_reference(tmp):
    exe = os.path.join(tmp, "ref_sammon")
    subprocess.check_call(["gcc"] + REFFLAGS + ["-I", REF] + [os.path.join(REF, o + ".c") for o in OBJECTS] +
                          ["-o", exe, "-lm"])
    return exe


def main():
    tmp = tempfile.mkdtemp()
    exe = build_reference(tmp)
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    all_cases = cases()
    inputs = sorted({c[0] for c in all_cases.values()})
    sammon_replay.write_generated(work, CLI)
    for name in inputs:
        if name not in sammon_replay.GENERATED:
            shutil.copy(os.path.join(CLI, name), os.path.join(work, name))
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    exp = {"inputs": {name: md5(os.path.join(work, name)) for name in inputs}, "runs": {}}
    for tag, (cin, rlen, seed, extra) in all_cases.items():
        args = ["-cin", cin, "-cout", tag + ".cod", "-rlen", str(rlen), "-rand", str(seed)] + extra
        p = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=work)
        if p.returncode != 0:
            raise RuntimeError("%s failed: %s" % (args, p.stderr))
        run = {"cin": cin, "rlen": rlen, "seed": seed, "args": args, "stdout": p.stdout, "stderr": p.stderr,
               "md5": md5(os.path.join(work, tag + ".cod"))}
        texts = [open(os.path.join(work, tag + ".cod")).read()]
        for kind in ("eps", "ps"):
            pic = os.path.join(work, "%s_sa.%s" % (tag, kind))
            if os.path.exists(pic):
                run[kind + "_md5"] = md5(pic)
                texts.append(open(pic).read())
        for t in texts:
            low = t.lower()
            assert "nan" not in low.replace("gaussian", "") and "inf" not in low.replace("findfont", ""), tag
        if "-v 2" in " ".join(args):
            noc = len(texts[0].strip().split("\n")) - 1
            worst = max(float(ln.split(":")[1]) for ln in p.stdout.split("\n") if ln)
            assert noc <= 300 and (noc * (noc - 1) // 2 - 1) * 2.0 ** -24 * worst < 0.0014, (tag, noc, worst)
        shutil.copy(os.path.join(work, tag + ".cod"), os.path.join(OUT, tag + ".cod"))
        exp["runs"][tag] = run
    shutil.rmtree(tmp)
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
