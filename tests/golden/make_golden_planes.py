#!/usr/bin/env python3
"""Generate the planes fixtures from the REAL reference (its planes.c, compiled where it lies with oracle/Makefile's
flags into a temporary directory; nothing of it is kept).

Run in the build container only:   python tests/golden/make_golden_planes.py

  planes/expected.json   md5 of every input, and per run: arguments, return code, stdout, stderr, and per file the run
                         wrote its name, the md5 of its NORMALISED text and its parsed content (discs with their grey
                         strings, labels, circles, path segments, sizes)

Normalised = without the bodies of the procedure definitions (every line from a line "/LN" or "/LP" through the next line
that ends in "} def"): they are program text of the reference and are not recorded, and neither is any output text that
holds them.  Inputs are fixtures of tests/golden/cli and tests/golden/data or are made by tests/planes_replay.py
write_generated() (NOT stored: the tests make them again and check their md5).  Every run happens in the directory that
holds its inputs, because the output lands beside -cin.
"""
import glob
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

import planes_replay  # noqa: E402

REF = os.environ.get("SOM_PAK_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "planes")
SOURCES = ["planes", "som_rout", "lvq_pak", "fileio", "labels", "datafile", "version"]
REFFLAGS = ["-O3", "-w", "-ffp-contract=off"]          # oracle/Makefile
STORED = {"cli": ["som_hexa_gaussian.cod", "som_hexa_bubble.cod", "som_rect_gaussian.cod", "som_rect_bubble.cod",
                  "somexample_vcal.cod", "lvq_olvq1.cod"],
          "data": ["ex.dat", "ex_masked.dat"]}


def cases():
    """tag -> arguments"""
    c = {}
    c["all_hexa"] = ["-cin", "som_hexa_gaussian.cod", "-plane", "0"]
    c["all_rect"] = ["-cin", "som_rect_bubble.cod", "-plane", "0"]
    c["default_plane"] = ["-cin", "som_rect_gaussian.cod"]
    c["single_plane"] = ["-cin", "som_hexa_bubble.cod", "-plane", "3"]
    c["ps_plane"] = ["-cin", "som_hexa_bubble.cod", "-plane", "2", "-ps", "1"]
    c["ps_all_rect"] = ["-cin", "som_rect_gaussian.cod", "-plane", "0", "-ps", "1"]
    c["labels_vcal"] = ["-cin", "somexample_vcal.cod", "-plane", "0"]
    c["labels_parens"] = ["-cin", "parens.cod", "-plane", "0"]
    c["constant"] = ["-cin", "constant.cod", "-plane", "0"]
    c["traj_ex_hexa"] = ["-cin", "som_hexa_gaussian.cod", "-din", "ex.dat"]
    c["traj_ex_rect_ps"] = ["-cin", "som_rect_bubble.cod", "-din", "ex.dat", "-plane", "5", "-ps", "1"]
    c["traj_masked"] = ["-cin", "som_hexa_gaussian.cod", "-din", "ex_masked.dat", "-plane", "0"]
    c["traj_masked_buffer"] = ["-cin", "som_hexa_gaussian.cod", "-din", "ex_masked.dat", "-plane", "0", "-buffer", "100"]
    c["traj_breaks"] = ["-cin", "som_hexa_gaussian.cod", "-din", "breaks.dat"]
    c["traj_breaks_buffer"] = ["-cin", "som_hexa_gaussian.cod", "-din", "breaks.dat", "-buffer", "16"]
    c["traj_breaks_rect"] = ["-cin", "som_rect_bubble.cod", "-din", "breaks.dat", "-buffer", "7"]
    c["err_not_a_map"] = ["-cin", "lvq_olvq1.cod"]
    c["err_plane_too_high"] = ["-cin", "som_hexa_gaussian.cod", "-plane", "6"]
    c["err_data_wider"] = ["-cin", "som_hexa_gaussian.cod", "-din", "wide.dat"]
    c["round"] = ["-cin", "round.cod", "-plane", "0"]
    return c


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def pictures(work):
    return sorted(glob.glob(os.path.join(work, "*.eps")) + glob.glob(os.path.join(work, "*.ps")))


def main():
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "ref_planes")
    subprocess.check_call(["gcc"] + REFFLAGS + ["-I", REF] + [os.path.join(REF, s + ".c") for s in SOURCES] +
                          ["-o", exe, "-lm"])
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    planes_replay.write_generated(work)
    names = list(planes_replay.generated_names())
    for sub, files in STORED.items():
        for name in files:
            shutil.copy(os.path.join(HERE, sub, name), os.path.join(work, name))
            names.append(name)
    os.makedirs(OUT, exist_ok=True)
    exp = {"inputs": {name: md5(os.path.join(work, name)) for name in sorted(names)}, "runs": {}}
    for tag, args in sorted(cases().items()):
        for path in pictures(work):
            os.remove(path)
        p = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=work)
        files = {}
        for path in pictures(work):
            norm = planes_replay.normalise(open(path, encoding="latin-1").read())
            assert "nan" not in norm.lower() and "} def" not in norm, (tag, path)
            files[os.path.basename(path)] = {"md5": planes_replay.md5_text(norm), "content": planes_replay.parse_text(norm)}
        if tag.startswith("err_") != (p.returncode != 0) or tag.startswith("err_") != (not files):
            raise RuntimeError("planes %s: status %d, %d files: %s" % (args, p.returncode, len(files), p.stderr))
        exp["runs"][tag] = {"args": args, "returncode": p.returncode, "stdout": p.stdout.decode(), "stderr": p.stderr.decode(),
                            "files": files}
    shutil.rmtree(tmp)
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=None, sort_keys=True, separators=(",", ":"))
    print("wrote", OUT, "(%d runs)" % len(exp["runs"]))


if __name__ == "__main__":
    main()
