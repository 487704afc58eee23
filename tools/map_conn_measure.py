#!/usr/bin/env python3
"""Times map connectivity (somhip_map_connectivity, K1c) on one MI355X beside somhip_map_quality, and somhip_map_quality
beside the parent commit's.

Shapes: those of profiles/map_quality_vs_parent.txt -- 256 x 256 x 512 over 1 M generated vectors, 32 x 32 x 128 over
100 k -- data gen:k=16,seed=9 made in HBM, the map the next xdim * ydim rows of the same stream.

  map_quality   child processes that alternate between the library under --parent-lib and this commit's, `--rounds` of
                each: per child a warm-up call, then `--reps` calls on the host clock from an engine synchronise to the
                return of the call (the call ends in a device synchronise), events off.  Reported: every child's median, the
                spread of the parent's children among themselves (largest less smallest median), and this commit's median of
                medians less the parent's.
  the pairs     this commit's children also time the fused call (quality and pairs from one search) and the pairs-only
                call the same way, and then the fused call with the LaunchTimer on: the stage totals of somhip_conn_timing
                and somhip_map_quality_timing, the pairs found and the table's bytes (16 per pair).  The fused call's table
                is compared with the pairs-only call's, and its totals with map_quality's, before any time is printed.
  the tool      `somqual` with and without -conn, process start to exit on this script's host clock, -v 0, a raw fp32 code
                file: four runs each, the first dropped, the two alternating."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 256, 512, 1000000), (32, 32, 128, 100000)]   # xdim, ydim, dim, vectors
NEW = ["somhip_conn_create", "somhip_conn_destroy", "somhip_conn_clear", "somhip_conn_size", "somhip_conn_read",
       "somhip_map_connectivity", "somhip_conn_timing"]


def med(v):
    return statistics.median(v)


def fmt(v):
    return "[" + ", ".join("%.3f" % x for x in v) + "]"


def child(E, eng, who, reps, shapes):
    for xdim, ydim, dim, n in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)

        def timed(call):
            eng.sync()
            t0 = time.perf_counter()
            r = call()
            return (time.perf_counter() - t0) * 1e3, r
        timed(lambda: E.map_quality(cb, ds))
        r = {"who": who, "shape": [xdim, ydim, dim, n], "quality": [timed(lambda: E.map_quality(cb, ds))[0] for _ in range(reps)]}
        if who == "this":
            conn = E.Conn(eng)

            def fused():
                conn.clear()
                return E.map_connectivity(cb, ds, conn, quality=True)

            def pairs_only():
                conn.clear()
                return E.map_connectivity(cb, ds, conn)
            want = E.map_quality(cb, ds)
            pairs_only()
            table = conn.read()
            got = fused()
            assert all(np.array_equal(a, b) for a, b in zip(conn.read(), table)), "the fused call's table differs"
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
            r["fused"] = [timed(fused)[0] for _ in range(reps)]
            r["pairs_only"] = [timed(pairs_only)[0] for _ in range(reps)]
            ev = []
            for _ in range(reps):
                eng.timing(True)
                eng.timing_reset()
                wall = timed(fused)[0]
                st = dict(eng.conn_timing())
                st.update(eng.map_quality_timing())
                eng.timing(False)
                ev.append({"wall": wall, "stages": {k: list(v) for k, v in st.items()}})
            r["events"] = ev
            r["pairs"], r["samples"] = conn.size()
            conn.close()
        print("JSON " + json.dumps(r), flush=True)
        cb.close(); ds.close()


def write_raw_map(E, path, xdim, ydim, dim, n):
    rows = np.ascontiguousarray(E.gen_rows(9, 16, dim, n, xdim * ydim)[0], dtype="<f4")
    with open(path, "wb") as f:
        f.write(("#!somf32 %d 0\n%d hexa %d %d bubble\n" % (xdim * ydim, dim, xdim, ydim)).encode())
        f.write(rows.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None, help="(a child process) 'parent' or 'this': the library under SOMHIP_LIB")
    ap.add_argument("--small", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--shape", type=int, default=None, help="only this entry of the shapes (0: the large one, 1: the small one)")
    ap.add_argument("--no-tool", action="store_true", help="leave the somqual runs out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [(24, 16, 40, 9000)] if a.small else SHAPES if a.shape is None else [SHAPES[a.shape]]
    from som_lvq_pak_amd import _lib, engine as E
    if a.child:
        if a.child == "parent":                             # the parent's library has no pair table: bind what it has
            for name in NEW:
                del _lib.SIGNATURES[name]
        eng = E.Engine(0)
        child(E, eng, a.child, a.reps, shapes)
        eng.close()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    me = os.path.abspath(__file__)
    runs = {}
    for who in (["parent", "this"] if a.parent_lib else ["this"]) * a.rounds:
        env = dict(os.environ)
        if who == "parent":
            env["SOMHIP_LIB"] = os.path.abspath(a.parent_lib)
        pick = (["--small"] if a.small else []) + (["--shape", str(a.shape)] if a.shape is not None else [])
        p = subprocess.run([sys.executable, me, "--child", who, "--reps", str(a.reps)] + pick, env=env,
                           stdout=subprocess.PIPE, text=True, check=True, timeout=900)
        for s in p.stdout.split("\n"):
            if s.startswith("JSON "):
                r = json.loads(s[5:])
                runs.setdefault(tuple(r["shape"]), []).append(r)
    for shape, rs in runs.items():
        out("== %d x %d x %d over %d generated vectors" % shape)
        meds = {"parent": [], "this": []}
        for r in rs:
            meds[r["who"]].append(med(r["quality"]))
            out("  %-6s somhip_map_quality wall ms: median %.3f of %s" % (r["who"], med(r["quality"]), fmt(r["quality"])))
        if meds["parent"]:
            diff = med(meds["this"]) - med(meds["parent"])
            out("  map_quality: the parent's children among themselves: spread %.3f ms (this commit's: %.3f ms); this commit less the "
                "parent, medians of medians: %+.3f ms (%+.2f %%)"
                % (max(meds["parent"]) - min(meds["parent"]), max(meds["this"]) - min(meds["this"]), diff, 100 * diff / med(meds["parent"])))
        else:
            out("  map_quality against the parent: not measured (no --parent-lib)")
        for r in rs:
            if r["who"] != "this":
                continue
            out("  this   fused call wall ms: median %.3f of %s | pairs alone: median %.3f of %s | map_quality: median %.3f"
                % (med(r["fused"]), fmt(r["fused"]), med(r["pairs_only"]), fmt(r["pairs_only"]), med(r["quality"])))
            names = list(r["events"][0]["stages"])
            tot = {k: med([e["stages"][k][1] for e in r["events"]]) for k in names}
            wall = med([e["wall"] for e in r["events"]])
            out("         with events on: wall median %.3f ms; " % wall
                + "; ".join("%s %d launches %.3f ms" % (k, r["events"][0]["stages"][k][0], tot[k]) for k in names))
            pair_pass = sum(tot[k] for k in ("k_conn_keys", "sort", "runs", "merge"))
            out("         the pair pass (keys, sort, runs, merge): %.3f ms by events = %.2f %% of the fused call's %.3f ms (events off); "
                "the fused call less map_quality on the host clock: %+.3f ms (%+.2f %%)"
                % (pair_pass, 100 * pair_pass / med(r["fused"]), med(r["fused"]), med(r["fused"]) - med(r["quality"]),
                   100 * (med(r["fused"]) - med(r["quality"])) / med(r["quality"])))
            out("         %d pairs of %d samples; the table holds %d bytes" % (r["pairs"], r["samples"], 16 * r["pairs"]))
    somqual = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "somqual")
    with tempfile.TemporaryDirectory() as tmp:
        for xdim, ydim, dim, n in ([] if a.no_tool else shapes):
            cod = os.path.join(tmp, "m.f32")
            write_raw_map(E, cod, xdim, ydim, dim, n)
            src = "gen:k=16,dim=%d,n=%d,seed=9" % (dim, n)
            walls, text = {"plain": [], "-conn": []}, {}
            for rep in range(4):
                for name, extra in (("plain", []), ("-conn", ["-conn", os.path.join(tmp, "pairs.txt")])):
                    t0 = time.perf_counter()
                    p = subprocess.run([somqual, "-cin", cod, "-din", src, "-v", "0"] + extra, check=True, stdout=subprocess.PIPE, text=True,
                                       timeout=600)
                    walls[name].append((time.perf_counter() - t0) * 1e3)
                    text[name] = p.stdout.rstrip("\n").split("\n")
            assert text["-conn"][:3] == text["plain"], "somqual -conn changes the first three lines"
            out("== somqual, %d x %d x %d, -din %s (process start to exit)" % (xdim, ydim, dim, src))
            for name in ("plain", "-conn"):
                out("  %-6s wall ms: median %.1f of %s after a first run of %.1f" % (name, med(walls[name][1:]), fmt(walls[name][1:]), walls[name][0]))
            out("  " + " | ".join(text["-conn"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"lines": len(lines)}))


if __name__ == "__main__":
    main()
