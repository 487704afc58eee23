#!/usr/bin/env python3
"""Record what the REAL reference's k-NN vote consumers (oracle/_ref, built from /root/reference) write for more than 8
neighbours.

Run in the build container only:   python tests/golden/make_golden_knn_vote.py

  knn_vote/expected.json   per run: the command (tool, data, codebook, arguments), the exit code, the stdout and the md5 of
                           every file it wrote -- setlabel -knn 9 / 21, eveninit -knn 9, propinit -knn 11, balance -knn 9,
                           elimin -knn 9 / 10 / 12 (the reference caps 12 to its own 10, with a message) on data/ex1.dat
                           and data/ex2.dat, and on ex1_masked.dat / ex2_masked.dat (not stored:
                           make_golden_masked.write_masked_data() makes them again, masked/expected.json holds their md5).
                           Masked balance stays out (the reference reads and writes past the end of its
                           rate array there).  Only runs the reference ends with exit code 0 are kept.

balance's OLVQ1 pass reads the rates of the codes it has just appended past the end of its rate array (balance.c:188,
lvq_rout.c:661-670), so its bytes mean something only where those codes win no sample but the data row they are copies
of (an update by any rate then changes nothing).  appended_codes_win() replays the pass from the reference's own files and
counts the other wins; a balance run with any is left out.  cli/lvq_init.cod at -knn 9 is one: the appended copy of
data row 735 wins rows 1497 and 1912, and the reference's file is the replay's with a rate of 0 for that code, not with
the 0.3 the reference intends (balance.c:203) and this project uses.  So balance -knn 9 starts from the reference's
`eveninit -noc 400` (as balance_even400_knn3 in cli/expected.json does), where the replay finds no such win; "made"
holds that codebook's md5 and the tests make it again with this project's eveninit.

No other fixture is touched.
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
sys.path.insert(0, HERE)

from oracle import build, ref_tool  # noqa: E402
from make_golden_masked import write_masked_data  # noqa: E402

OUT = os.path.join(HERE, "knn_vote")

# codebooks the runs below start from, made first: file -> (tool, data, arguments)
MADE = {"even400.cod": ("eveninit", "data/ex1.dat", ["-noc", "400"])}
# tag -> (tool, data, codebook or None, arguments); data and codebook relative to tests/golden, "masked:" = the directory
# write_masked_data() fills, "made:" = the directory of the MADE codebooks
RUNS = {
    "setlabel_9": ("setlabel", "data/ex2.dat", "cli/lvq_olvq1.cod", ["-knn", "9"]),
    "setlabel_21": ("setlabel", "data/ex2.dat", "cli/lvq_olvq1.cod", ["-knn", "21"]),
    "eveninit_9": ("eveninit", "data/ex1.dat", None, ["-noc", "200", "-knn", "9"]),
    "propinit_11": ("propinit", "data/ex1.dat", None, ["-noc", "200", "-knn", "11"]),
    "balance_9": ("balance", "data/ex1.dat", "made:even400.cod", ["-knn", "9"]),
    "elimin_9": ("elimin", "data/ex1.dat", None, ["-knn", "9"]),
    "elimin_10": ("elimin", "data/ex1.dat", None, ["-knn", "10"]),
    "elimin_12": ("elimin", "data/ex1.dat", None, ["-knn", "12"]),
    "masked_setlabel_9": ("setlabel", "masked:ex2_masked.dat", "masked/olvq1.cod", ["-knn", "9"]),
    "masked_setlabel_21": ("setlabel", "masked:ex2_masked.dat", "masked/olvq1.cod", ["-knn", "21"]),
    "masked_eveninit_9": ("eveninit", "masked:ex1_masked.dat", None, ["-noc", "200", "-knn", "9"]),
    "masked_propinit_11": ("propinit", "masked:ex1_masked.dat", None, ["-noc", "200", "-knn", "11"]),
    "masked_elimin_9": ("elimin", "masked:ex1_masked.dat", None, ["-knn", "9"]),
    "masked_elimin_10": ("elimin", "masked:ex1_masked.dat", None, ["-knn", "10"]),
    "masked_elimin_12": ("elimin", "masked:ex1_masked.dat", None, ["-knn", "12"]),
}


def locate(name, dirs):
    """dirs: {"masked": directory, "made": directory}"""
    for kind, directory in dirs.items():
        if name.startswith(kind + ":"):
            return os.path.join(directory, name[len(kind) + 1:])
    return os.path.join(HERE, name)


def command(exe, run, dirs, out):
    """the command line of a recorded run writing to `out` (the tests run this project's tools with it)"""
    tool, din, cin, args = run
    cmd = [exe, "-din", locate(din, dirs)]
    if cin:
        cmd += ["-cin", locate(cin, dirs)]
    return cmd + ["-cout", out] + list(args) + ["-v", "0"]


def make_codebooks(exe_of, directory):
    """the MADE codebooks into `directory`, by the tools exe_of(name) names"""
    for name, (tool, din, args) in MADE.items():
        subprocess.check_call([exe_of(tool), "-din", os.path.join(HERE, din), "-cout", os.path.join(directory, name)] +
                              list(args) + ["-v", "0"])


def appended_codes_win(din, cin, cout, lra):
    """Replay of balance's OLVQ1 pass (lvq_rout.c:637-673) from the files of one of its runs: how often a code that
    balance appended (the rows of cout behind the len(lra) kept ones; copies of data rows) wins a sample at a distance
    above 0.  The appended codes get the rate 0; the kept ones start at 0.3."""
    from som_lvq_pak_amd import textio
    tab = textio.LabelTable()
    data, init, out = (textio.read_entries(f, tab)[0] for f in (din, cin, cout))
    first = lambda e: np.array([l[0] if len(l) else 0 for l in e.labels])  # noqa: E731
    dl, il, ol = first(data), first(init), first(out)
    x, c0, res = (e.points.astype(np.float32) for e in (data, init, out))
    nkeep = len(open(lra).read().split())
    picked = [int(np.nonzero((x == res[r]).all(axis=1))[0][0]) for r in range(nkeep, res.shape[0])]
    lose = {}                                     # removed: the first codes of the classes that lost some (balance.c:140-167)
    for lab in il:
        lose[int(lab)] = lose.get(int(lab), 0) + 1
    for lab in ol[:nkeep]:
        lose[int(lab)] -= 1
    keep = []
    for r, lab in enumerate(il):
        if lose[int(lab)] > 0:
            lose[int(lab)] -= 1
        else:
            keep.append(r)
    assert len(keep) == nkeep and (il[keep] == ol[:nkeep]).all()
    c = np.concatenate([c0[keep], x[picked]]).astype(np.float32)
    lab = np.concatenate([il[keep], ol[nkeep:]])
    ta = np.full(c.shape[0], 0.3, np.float32)
    ta[nkeep:] = 0.0
    wins = 0
    for s in range(x.shape[0]):
        acc = np.zeros(c.shape[0], np.float32)
        for i in range(x.shape[1]):
            d = c[:, i] - x[s, i]
            acc = acc + d * d
        w = int(np.argmin(acc))
        wins += w >= nkeep and acc[w] > 0
        a = ta[w]
        if lab[w] == dl[s]:
            c[w] = c[w] + a * (x[s] - c[w])
            ta[w] = a / (np.float32(1) + a)
        else:
            c[w] = c[w] - a * (x[s] - c[w])
            ta[w] = min(a / (np.float32(1) - a), np.float32(0.3))
    assert np.abs(c - res).max() < 1e-3, "the replay is not the reference's pass"
    return int(wins)


def md5s(directory):
    return {f: hashlib.md5(open(os.path.join(directory, f), "rb").read()).hexdigest() for f in sorted(os.listdir(directory))}


def main():
    build()
    os.makedirs(OUT, exist_ok=True)
    dirs = {"masked": tempfile.mkdtemp(), "made": tempfile.mkdtemp()}
    write_masked_data(dirs["masked"])
    make_codebooks(ref_tool, dirs["made"])
    exp = {"made": md5s(dirs["made"]), "runs": {}}
    for tag, run in RUNS.items():
        work = tempfile.mkdtemp()
        cout = os.path.join(work, "out.cod")
        p = subprocess.run(command(ref_tool(run[0]), run, dirs, cout), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, cwd=work)
        if p.returncode != 0:
            print("left out: %s ended with exit code %d: %s" % (tag, p.returncode, p.stderr.strip()))
        elif run[0] == "balance" and appended_codes_win(locate(run[1], dirs), locate(run[2], dirs), cout,
                                                         os.path.join(work, "out.lra")):
            print("left out: %s: appended codes win other samples, the bytes come from rates read past the array" % tag)
        else:
            exp["runs"][tag] = {"tool": run[0], "din": run[1], "cin": run[2], "args": run[3], "exit": p.returncode,
                                "stdout": p.stdout, "md5": md5s(work)}
        shutil.rmtree(work)
    for d in dirs.values():
        shutil.rmtree(d)
    json.dump(exp, open(os.path.join(OUT, "expected.json"), "w"), indent=1, sort_keys=True)
    print("wrote", OUT, "with", len(exp["runs"]), "runs")


if __name__ == "__main__":
    main()
