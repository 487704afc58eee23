#!/usr/bin/env python3
"""Times batch GLVQ (somhip_glvq_train, K9) per stage on one MI355X, both routes of its search, at the shapes of the LVQ
bench configurations: 10 000 x 256 (c3) and 100 000 x 1024 (c5), 100 000 samples each.

Data and codebook are the seeded mixture stream of bench.py's LVQ configurations (same seed, classes and dimension): the
data its first 100 000 rows, the codebook the rows behind them, each row labelled with its mixture id.

Per shape, best of `--reps` after one warm-up call, from the HIP events of somhip_glvq_timing:
  search   the class-wise winner search alone (somhip_debug_glvq_search) on the direct route and on the list route, and the
           share of the samples in the list route's remainder
  epoch    one epoch of somhip_glvq_train on the planned route: search, terms + group, sums, update, and the host clock
           around the call
For orientation only, beside them: one pass of the same data through lvq_train OLVQ1 (the exact batched online engine),
host clock.  --out FILE also writes the lines there.

--pieces measures the epoch over data in pieces (somhip_glvq_begin / _accumulate / _finish) instead:
  (a) one call of somhip_glvq_train per shape on this tree's libsomhip.so and on --parent-lib (a libsomhip.so built from the
      parent commit), in alternating child processes: HIP-event stage totals, best of --reps, and the spread of each
      library's own runs
  (b) the same epoch in 1, 4 and 16 pieces: HIP-event totals per stage and per piece, and the host clock per piece; what
      the host clock holds beyond the events is the piece's host side (the label check, the tail copy, the syncs)
  (c) the glvq tool by the host clock, plain against -buffer n/4, on a labelled gen: source"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (codebook rows, dim, classes, seed of the stream, alpha of the OLVQ1 line)
    "c3": (10000, 256, 100, 2345, 0.3),
    "c5": (100000, 1024, 1000, 4567, 0.05),
}
SAMPLES = 100000


def one_call_child(lib_path, name, n, reps):
    """in a child process: `reps` timed epochs of somhip_glvq_train after a warm-up on the library at lib_path; prints one
    line of stage totals per epoch"""
    from som_lvq_pak_amd import _lib
    _lib.LIB_PATH = lib_path
    import ctypes
    probe = ctypes.CDLL(lib_path)
    if not hasattr(probe, "somhip_glvq_begin"):                      # a parent library: it has no pieces to declare
        _lib.GLVQ_PIECES_SIGNATURES.clear()
    from som_lvq_pak_amd import engine as E
    eng = E.Engine(0)
    rows, dim, classes, seed, _ = SHAPES[name]
    ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
    src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
    codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
    src.close()
    cb = E.Codebook(eng, codes, labels=clab)
    for rep in range(reps + 1):
        cb.upload(codes)
        eng.timing(True)
        eng.timing_reset()
        E.glvq_train(cb, ds, 1, 1.0, stats=False)
        t = eng.glvq_timing()
        eng.timing(False)
        if rep:
            print("STAGES %.4f %.4f %.4f %.4f" % (t["search"][1], t["terms"][1], t["k_glvq_sums"][1], t["k_glvq_update"][1]), flush=True)
    eng.close()


def pieces(a, say):
    import subprocess
    from som_lvq_pak_amd import _lib, engine as E
    n = a.samples
    # (a) alternating child processes: this, parent, this, parent, ...
    libs = [("this", _lib.LIB_PATH)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    if not a.parent_lib:
        say("(a) no --parent-lib given: only this tree's library is timed")
    for name in a.shapes.split(","):
        runs = {k: [] for k, _ in libs}
        for turn in range(a.turns):
            for k, path in libs:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--shapes", name, "--samples", str(n),
                                      "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True, check=True).stdout
                runs[k] += [[float(v) for v in ln.split()[1:]] for ln in out.splitlines() if ln.startswith("STAGES")]
        rows, dim = SHAPES[name][:2]
        say("(a) %s: %d x %d, %d samples, one call of somhip_glvq_train, %d child processes a library, %d epochs each" %
            (name, rows, dim, n, a.turns, a.reps))
        for k, _ in libs:
            tot = sorted(sum(r) for r in runs[k])
            best = min(runs[k], key=sum)
            say("  %-6s best %9.3f ms (search %.3f, terms + group %.3f, sums %.3f, update %.3f); its own runs %.3f .. %.3f ms (spread %.2f %%)" %
                (k, sum(best), best[0], best[1], best[2], best[3], tot[0], tot[-1], 100.0 * (tot[-1] - tot[0]) / tot[0]))
        if len(libs) == 2:
            t, p = min(sum(r) for r in runs["this"]), min(sum(r) for r in runs["parent"])
            say("  this / parent, best against best: %.4f" % (t / p))
    # (b) the epoch in 1, 4, 16 pieces
    eng = E.Engine(0)
    for name in a.shapes.split(","):
        rows, dim, classes, seed, _ = SHAPES[name]
        ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
        src.close()
        cb = E.Codebook(eng, codes, labels=clab)
        E.glvq_train(cb, ds, 1, 1.0, stats=False)
        want = cb.download()
        say("(b) %s: the epoch in pieces; state blob %.1f MB" % (name, (8 * (2 * rows * (dim + 1) + rows) + 8 * rows + 16) / 1e6))
        for k in (1, 4, 16):
            best = None
            for rep in range(a.reps + 1):
                cb.upload(codes)
                eng.timing(True)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                E.glvq_begin(cb)
                per = (n + k - 1) // k
                for first in range(0, n, per):
                    E.glvq_accumulate(cb, ds, first, min(per, n - first))
                E.glvq_finish(cb, 1.0)
                wall = (time.perf_counter() - t0) * 1e3
                t = eng.glvq_timing()
                eng.timing(False)
                if rep and (best is None or wall < best[0]):
                    best = (wall, t)
            same = (cb.download().view(np.uint32) == want.view(np.uint32)).all()
            wall, t = best
            ev = sum(v[1] for v in t.values())
            say("  %2d pieces: host clock %9.3f ms (%.3f a piece); events: search %.3f, terms + group %.3f, sums + counts %.3f "
                "(%.3f a piece, %d launches), update %.3f; beyond the events (label check, tail copy, syncs) %.3f ms (%.3f a piece); "
                "rows equal the one call's: %s" % (k, wall, wall / k, t["search"][1], t["terms"][1], t["k_glvq_sums"][1], t["k_glvq_sums"][1] / k,
                                                   t["k_glvq_sums"][0], t["k_glvq_update"][1], wall - ev, (wall - ev) / k, same))
        E.glvq_end(cb)
        cb.close()
        ds.close()
    eng.close()
    # (c) the tool
    import tempfile
    tool = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "glvq")
    rows, dim, classes, seed = 1000, 256, 100, 2345
    with tempfile.TemporaryDirectory() as tmp:
        eng = E.Engine(0)
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres
        src.close()
        eng.close()
        cod = os.path.join(tmp, "c.cod")
        with open(cod, "w") as fh:
            fh.write("%d\n" % dim)
            for row, l in zip(codes, clab):
                fh.write(" ".join("%.9g" % v for v in row) + " c%d\n" % int(l))
        base = [tool, "-cin", cod, "-din", "gen:k=%d,dim=%d,n=%d,seed=%d,labels=1" % (classes, dim, n, seed), "-epochs", "3", "-alpha", "1"]
        say("(c) glvq, %d x %d codebook file, labelled gen: source of %d rows, 3 epochs, host clock of the whole process" % (rows, dim, n))
        outs = {}
        for label, extra in (("plain", []), ("-buffer %d" % (n // 4), ["-buffer", str(n // 4)])):
            walls = []
            for rep in range(a.reps):
                out = os.path.join(tmp, "o_%d.cod" % len(outs))
                t0 = time.perf_counter()
                subprocess.run(base + ["-cout", out] + extra, check=True, stdout=subprocess.DEVNULL)
                walls.append(time.perf_counter() - t0)
            outs[label] = open(out, "rb").read()
            say("  %-14s best %.3f s  all %s" % (label, min(walls), ["%.3f" % v for v in walls]))
        say("  the two files are equal byte for byte: %s" % (len(set(outs.values())) == 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=SAMPLES)
    ap.add_argument("--no-olvq1", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pieces", action="store_true", help="measure the epoch over data in pieces (see above)")
    ap.add_argument("--parent-lib", default=None, help="--pieces (a): a libsomhip.so built from the parent commit")
    ap.add_argument("--turns", type=int, default=3, help="--pieces (a): child processes per library, alternating")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return one_call_child(a.child, a.shapes, a.samples, a.reps)
    from som_lvq_pak_amd import engine as E

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.pieces:
        pieces(a, say)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return

    eng = E.Engine(0)
    n = a.samples
    for name in a.shapes.split(","):
        rows, dim, classes, seed, alpha = SHAPES[name]
        ds = E.Dataset(eng, generate=(seed, classes, dim, 0, n))
        src = E.Dataset(eng, generate=(seed, classes, dim, n, rows))
        codes, clab = src.rows(0, rows), src.centres.astype(np.int32)
        src.close()
        cb = E.Codebook(eng, codes, labels=clab)
        say("%s: %d x %d codebook, %d classes, %d samples; planned route: %s" %
            (name, rows, dim, classes, n, "list" if E.glvq_plan(rows, dim, n) == E.GLVQ_LIST else "direct"))
        found = {}
        for route, rname in ((E.GLVQ_DIRECT, "direct"), (E.GLVQ_LIST, "list")):
            ms, rem = [], 0
            for rep in range(a.reps + 1):
                eng.timing(True)
                eng.timing_reset()
                out = E.glvq_search(cb, ds, 0, n, route)
                t = eng.glvq_timing()
                eng.timing(False)
                rem = out[4]
                if rep:
                    ms.append(t["search"][1])
            found[rname] = out[:4]
            elems = float(n if route == E.GLVQ_DIRECT else rem) * rows * dim
            say("  search %-6s best %9.3f ms  all %s  remainder %d of %d (%.2f %%)  class-wise scan: %.3g fp32 elements" %
                (rname, min(ms), ["%.3f" % v for v in ms], rem, n, 100.0 * rem / n, elems))
        same = all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(found["direct"], found["list"]))
        say("  the two routes agree by bit pattern and index: %s" % same)
        best = None
        for rep in range(a.reps + 1):
            cb.upload(codes)
            eng.timing(True)
            eng.timing_reset()
            eng.sync()
            t0 = time.perf_counter()
            E.glvq_train(cb, ds, 1, 1.0, stats=False)
            wall = (time.perf_counter() - t0) * 1e3
            t = eng.glvq_timing()
            eng.timing(False)
            if rep and (best is None or wall < best[0]):
                best = (wall, t)
        wall, t = best
        say("  epoch (best of %d by the host clock): %.3f ms; search %.3f, terms + group %.3f, sums %.3f, update %.3f ms" %
            (a.reps, wall, t["search"][1], t["terms"][1], t["k_glvq_sums"][1], t["k_glvq_update"][1]))
        if not a.no_olvq1:
            walls = []
            for rep in range(a.reps + 1):
                cb.upload(codes)
                talpha = np.full(rows, alpha, dtype=np.float32)
                eng.sync()
                t0 = time.perf_counter()
                E.lvq_train(cb, ds, E.OLVQ1, n, alpha, talpha=talpha, count=n, data_first=0, trace=False)
                eng.sync()
                if rep:
                    walls.append((time.perf_counter() - t0) * 1e3)
            say("  for orientation: lvq_train OLVQ1, one pass of the same %d samples: best %.1f ms  all %s" %
                (n, min(walls), ["%.1f" % v for v in walls]))
        cb.close()
        ds.close()
    eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
