#!/usr/bin/env python3
"""Generate the umat fixtures from the REAL reference (its umat.c, map.c, median.c and header.c, compiled where they lie
with oracle/Makefile's flags into a temporary directory; nothing of them is kept).

Run in the build container only:   python tests/golden/make_golden_umat.py

  umat/expected.json   md5 of every input, and per run: arguments, return code, stderr at -v 2, the md5 of the
                       NORMALISED output and its parsed content (block rows, unit rows, the numbers of the size lines)

Normalised = without the %%CreationDate: lines and without the PostScript prologue (every line after %%EndComments and
before the first line that begins "/radius "): the prologue is program text of the reference and is not recorded, and
neither is any output text that holds it.  Inputs are fixtures of tests/golden/cli or are made by tests/umat_replay.py
write_generated() (NOT stored: the tests make them again and check their md5).  Runs use file names relative to their
working directory.
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

import umat_replay  # noqa: E402

REF = os.environ.get("SOM_PAK_REFERENCE", "/root/reference")
CLI = os.path.join(HERE, "cli")
OUT = os.path.join(HERE, "umat")
SOURCES = ["umat", "map", "median", "header", "som_rout", "lvq_pak", "fileio", "labels", "datafile", "version"]
REFFLAGS = ["-O3", "-w", "-ffp-contract=off"]          # oracle/Makefile
STORED = ["som_hexa_gaussian.cod", "som_hexa_bubble.cod", "som_rect_gaussian.cod", "som_rect_bubble.cod",
          "somexample_vcal.cod"]


def cases():
    """tag -> arguments (-v 2 is added to every run)"""
    c = {}
    for t in ("hexa", "rect"):
        for n in ("gaussian", "bubble"):
            c["plain_%s_%s" % (t, n)] = ["-cin", "som_%s_%s.cod" % (t, n)]
        for tag, flags in (("average", ["-average"]), ("median", ["-median"]), ("both", ["-average", "-median"])):
            c["%s_%s" % (tag, t)] = ["-cin", "som_%s_gaussian.cod" % t] + flags
    c["labels_vcal"] = ["-cin", "somexample_vcal.cod"]
    c["labels_several"] = ["-cin", "labelled.cod"]
    c["labels_several_ps"] = ["-cin", "labelled.cod", "-ps", "-title", "a (b) \\ c"]
    c["ps_default"] = ["-cin", "som_hexa_gaussian.cod", "-ps"]
    c["ps_portrait_a3"] = ["-cin", "som_rect_bubble.cod", "-ps", "-portrait", "-paper", "A3"]
    c["ps_landscape_tall"] = ["-cin", "gen_hexa_4x5x5.cod", "-ps", "-landscape", "-notitle"]
    c["ps_best_tall"] = ["-cin", "gen_rect_4x5x5.cod", "-ps"]
    c["border_thresholds"] = ["-cin", "som_hexa_bubble.cod", "-border", "-W", "0.9", "-B", "0.1"]
    c["onlylabs"] = ["-cin", "somexample_vcal.cod", "-onlylabs"]
    c["nolabs_notitle"] = ["-cin", "somexample_vcal.cod", "-nolabs", "-notitle"]
    c["title_font"] = ["-cin", "som_rect_gaussian.cod", "-title", "my map", "-font", "Courier", "-fontsize", "0.8"]
    c["swap"] = ["-cin", "som_hexa_gaussian.cod", "-swapx", "-swapy"]
    c["guess_ps"] = ["-cin", "som_rect_bubble.cod", "-o", "x.ps"]
    c["guess_eps"] = ["-cin", "som_hexa_bubble.cod", "-o", "x.eps"]
    for mx, my, d in umat_replay.SHAPES:
        for t in ("hexa", "rect"):
            name = "gen_%s_%dx%dx%d.cod" % (t, mx, my, d)
            c["gen_%s_%dx%dx%d" % (t, mx, my, d)] = ["-cin", name]
            c["gen_%s_%dx%dx%d_both" % (t, mx, my, d)] = ["-cin", name, "-average", "-median"]
    for t in ("hexa", "rect"):
        c["round_%s" % t] = ["-cin", "round_%s.cod" % t]
        c["round_%s_both" % t] = ["-cin", "round_%s.cod" % t, "-average", "-median"]
    return c


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def main():
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "ref_umat")
    subprocess.check_call(["gcc"] + REFFLAGS + ["-I", REF] + [os.path.join(REF, s + ".c") for s in SOURCES] +
                          ["-o", exe, "-lm"])
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    umat_replay.write_generated(work)
    for name in STORED:
        shutil.copy(os.path.join(CLI, name), os.path.join(work, name))
    os.makedirs(OUT, exist_ok=True)
    names = sorted(STORED + umat_replay.generated_names())
    exp = {"inputs": {name: md5(os.path.join(work, name)) for name in names}, "runs": {}}
    env = {k: v for k, v in os.environ.items() if k != "UMAT_HEADERFILE"}
    for tag, args in sorted(cases().items()):
        p = subprocess.run([exe] + args + ["-v", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=work, env=env)
        if p.returncode != 0:
            raise RuntimeError("umat %s failed: %s" % (args, p.stderr))
        text = p.stdout.decode("latin-1")
        if "-o" in args:
            assert text == ""
            text = open(os.path.join(work, args[args.index("-o") + 1]), encoding="latin-1").read()
        norm = umat_replay.normalise(text)
        assert "nan" not in norm.lower() and norm.count("%%EndComments\n/radius ") == 1, tag
        exp["runs"][tag] = {"args": args, "returncode": p.returncode, "stderr": p.stderr.decode(),
                            "md5": umat_replay.md5_text(norm), "content": umat_replay.parse_text(norm)}
    shutil.rmtree(tmp)
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=None, sort_keys=True, separators=(",", ":"))
    print("wrote", OUT, "(%d runs)" % len(exp["runs"]))


if __name__ == "__main__":
    main()
