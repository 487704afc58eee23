#!/usr/bin/env python3
"""Times the batch map (somhip_som_batchmap, K8) per stage on one MI355X and sets it beside the online engine.

Per shape, neighbourhood and radius: one epoch (epochs = 1, so r_0 is the radius given) from the same codebook every time
(re-uploaded outside the timed window).  One warm-up call, then `--reps` calls with the host clock from an engine
synchronise to the return of the call (the call ends in a device synchronise), events off; then `--reps` calls with the
LaunchTimer on for the stage totals (somhip_batchmap_timing) and the winner search's kernels (the published table).

Derived figures, computed here from the shapes:
  sums     bytes = n * dim * 4 (every row once) + n * 4 (the list) + units * (dim + 1) * 8 (S written), over the sums' time,
           against the HBM figures of MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured)
  combine  useful FLOP = 2 * units^2 * (dim + 1) (H dense); issued FLOP = 2 * 64 * 64 * 80 per (destination group, source
           group, column block) that the kernel does not skip, counted here by the kernel's own box rule; over the combine's
           time, against the fp64 matrix rate: MI355X_MICROARCH.md lists none, so AMD's published 78.6 TFLOP/s for the MI355X
           is used (half the guide's 157.3 TFLOP/s fp32 matrix rate)

--parent-lib PATH: also times somhip_som_train at batch auto over the same number of vectors with that library (the parent
commit's, built from a clean checkout of it), in a child process that loads it through SOMHIP_LIB.

--pieces: the report on the epoch over data in pieces (somhip_batchmap_begin / _accumulate / _finish).
  one call   somhip_som_batchmap, one bubble epoch per shape at the first radius, in child processes that alternate between
             the library under --parent-lib and this commit's, `--rounds` of each: per child a warm-up call, `--reps` calls
             on the host clock with events off, `--reps` with the stage events on.  Reported: every child's medians, the
             spread of the parent's children among themselves (largest less smallest median) and this commit's median
             of medians less the parent's.
  pieces     this commit, the same epoch through begin / accumulate x k / finish for k = 1, 4, 16 equal pieces, timed the
             same way; the rows are compared with the one call's by bit pattern before any time is printed.
  the tool   `bsom` end to end (process start to exit, the host clock of this script) on a gen: source, without -buffer and
             with -buffer at a quarter and a sixteenth of the rows; with two or more devices also -gpus 2 and -gpus <all>.
  ranks      the bytes one epoch broadcasts, computed from the shapes: G times the state.

--missing: the report on the batch map over data with missing values (somhip_som_batchmap_missing, K8m).
  plain paths   somhip_som_batchmap per shape at bubble radius 1, bubble and gaussian at the first radius, in child processes
                that alternate between the library under --parent-lib and this commit's, `--rounds` of each, timed as under
                --pieces; and `bsom` end to end with the tool under --parent-bsom and this commit's, alternating.  Reported:
                every child's medians, the parent's spread among its own children, this commit less the parent.
  new stages    this commit's children also run somhip_som_batchmap_missing on the same unmasked data: the sums and the
                combine of the missing form beside the parent's plain stages, as ratios of the medians of medians.
  masked epoch  this commit, 30 % of the components masked at random (host data, uploaded), one epoch per stage; the
                winner search is the masked direct scan, one sample per launch column, so the large shape runs over
                --masked-large vectors only and its search time per vector is what carries to a larger run."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12
FP64_MATRIX = 78.6e12
SHAPES = [  # xdim, ydim, dim, vectors, radii
    (256, 256, 512, 1000000, (128.0, 16.0, 1.0)),
    (32, 32, 128, 1000000, (16.0, 4.0, 1.0)),
]


def group_boxes(xdim, ydim):
    """the lattice boxes of the 64-row groups, as bm_group_box (kernels/batchmap.hpp) forms them"""
    units = xdim * ydim
    ng = (units + 63) // 64
    g = np.arange(ng)
    if xdim % 8 == 0 and ydim % 8 == 0:
        pw = xdim // 8
        x0, y0 = (g % pw) * 8, (g // pw) * 8
        return x0, x0 + 7, y0, y0 + 7
    u0, u1 = g * 64, np.minimum(g * 64 + 63, units - 1)
    y0, y1 = u0 // xdim, u1 // xdim
    one = y0 == y1
    return np.where(one, u0 % xdim, 0), np.where(one, u1 % xdim, xdim - 1), y0, y1


def issued_tiles(xdim, ydim, topol, gauss, thresh):
    """(destination group, source group) pairs the combine stages and multiplies"""
    x0, x1, y0, y1 = group_boxes(xdim, ydim)
    ng = len(x0)
    if gauss:
        return ng * ng
    gx = np.maximum(0, np.maximum(x0[None, :] - x1[:, None], x0[:, None] - x1[None, :])).astype(np.float64)
    gy = np.maximum(0, np.maximum(y0[None, :] - y1[:, None], y0[:, None] - y1[None, :])).astype(np.float64)
    hx = gx if topol == 4 else np.maximum(0.0, gx - 0.5)
    least = hx * hx + (1.0 if topol == 4 else 0.75) * gy * gy
    return int((least <= thresh * 1.000001).sum())


def med(v):
    return statistics.median(v)


def fmt(v):
    return "[" + ", ".join("%.3f" % x for x in v) + "]"


def measure_batchmap(E, eng, reps, shapes, out):
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]                # the next rows of the stream: spread like the data, unordered
        for neigh, nname in ((E.NEIGH_BUBBLE, "bubble"), (E.NEIGH_GAUSSIAN, "gaussian")):
            cb = E.Codebook(eng, codes, E.TOPOL_HEXA, neigh, xdim, ydim)
            for radius in radii:
                def epoch(events):
                    cb.upload(codes)
                    eng.timing(events)
                    eng.timing_reset()
                    eng.sync()
                    t0 = time.perf_counter()
                    E.som_batchmap(cb, ds, 1, radius, qerror=False)
                    wall = (time.perf_counter() - t0) * 1e3
                    st = eng.batchmap_timing() if events else None
                    tab = eng.timing_table() if events else None
                    eng.timing(False)
                    return wall, st, tab
                epoch(False)
                walls = [epoch(False)[0] for _ in range(reps)]
                timed = [epoch(True) for _ in range(reps)]
                grp = [t[1]["group"][1] for t in timed]
                sums = [t[1]["k_batchmap_sums"][1] for t in timed]
                comb = [t[1]["k_batchmap_combine"][1] for t in timed]
                search = [sum(ms for _, ms in t[2].values()) for t in timed]
                wall_ev = [t[0] for t in timed]
                sum_bytes = n * dim * 4 + n * 4 + units * (dim + 1) * 8
                useful = 2.0 * units * units * (dim + 1)
                thresh = radius * radius                          # (the box rule against the squared radius, as the kernel's thresh)
                tiles = issued_tiles(xdim, ydim, E.TOPOL_HEXA, neigh == E.NEIGH_GAUSSIAN, thresh)
                issued = 2.0 * 64 * 64 * 80 * tiles * ((dim + 63) // 64)
                out("== %d x %d x %d hexa %s, radius %g, %d generated vectors, one epoch" % (xdim, ydim, dim, nname, radius, n))
                out("  wall ms, events off: median %.3f of %s" % (med(walls), fmt(walls)))
                out("  wall ms, events on:  median %.3f of %s" % (med(wall_ev), fmt(wall_ev)))
                out("  stage ms (events): group %.3f %s | sums %.3f %s | combine %.3f %s | winner-search kernels %.3f %s"
                    % (med(grp), fmt(grp), med(sums), fmt(sums), med(comb), fmt(comb), med(search), fmt(search)))
                w = med(wall_ev)
                out("  shares of the events-on wall: search %.1f %%, group %.1f %%, sums %.1f %%, combine %.1f %%, rest (copies, gaps) %.1f %%"
                    % (100 * med(search) / w, 100 * med(grp) / w, 100 * med(sums) / w, 100 * med(comb) / w,
                       100 * (w - med(search) - med(grp) - med(sums) - med(comb)) / w))
                bps = sum_bytes / (med(sums) * 1e-3)
                out("  sums: %.1f MB in %.3f ms = %.3f TB/s: %.1f %% of 8.0 TB/s spec, %.1f %% of 6.29 TB/s measured"
                    % (sum_bytes / 1e6, med(sums), bps / 1e12, 100 * bps / HBM_SPEC, 100 * bps / HBM_MEASURED))
                out("  combine: useful %.3f TFLOP (dense H), issued %.3f TFLOP (%d of %d group pairs) in %.3f ms = %.2f useful / %.2f issued "
                    "TFLOP/s: %.1f %% / %.1f %% of 78.6 TFLOP/s"
                    % (useful / 1e12, issued / 1e12, tiles, ((units + 63) // 64) ** 2, med(comb), useful / med(comb) / 1e9,
                       issued / med(comb) / 1e9, 100 * useful / (med(comb) * 1e-3) / FP64_MATRIX,
                       100 * issued / (med(comb) * 1e-3) / FP64_MATRIX))
            cb.close()
        ds.close()


def measure_online(E, eng, reps, shapes, out, who):
    """somhip_som_train at batch auto over as many vectors as an epoch reads"""
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
        walls = []
        for rep in range(min(reps, 2) + 1):
            cb.upload(codes)
            eng.sync()
            t0 = time.perf_counter()
            E.som_train(cb, ds, n, 0.05, radii[0], batch=-1, trace=False)
            eng.sync()
            walls.append((time.perf_counter() - t0) * 1e3)
        out("== %s: somhip_som_train, batch auto, %d x %d x %d hexa bubble, radius %g -> 1, alpha 0.05, %d iterations over %d generated vectors"
            % (who, xdim, ydim, dim, radii[0], n, n))
        out("  wall ms: median %.3f of %s after a warm-up run of %.3f" % (med(walls[1:]), fmt(walls[1:]), walls[0]))
        cb.close(); ds.close()


def onecall_child(E, eng, reps, shapes, who):
    """one bubble epoch per shape at its first radius: a JSON line per shape"""
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)

        def epoch(events):
            cb.upload(codes)
            eng.timing(events)
            eng.timing_reset()
            eng.sync()
            t0 = time.perf_counter()
            E.som_batchmap(cb, ds, 1, radii[0], qerror=False)
            wall = (time.perf_counter() - t0) * 1e3
            st = eng.batchmap_timing() if events else None
            eng.timing(False)
            return wall, st
        epoch(False)
        walls = [epoch(False)[0] for _ in range(reps)]
        timed = [epoch(True)[1] for _ in range(reps)]
        print("JSON " + json.dumps({"who": who, "shape": [xdim, ydim, dim, n], "walls": walls,
                                    "group": [t["group"][1] for t in timed], "sums": [t["k_batchmap_sums"][1] for t in timed],
                                    "combine": [t["k_batchmap_combine"][1] for t in timed]}), flush=True)
        cb.close(); ds.close()


def pieces_report(E, a, shapes, out):
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    runs = {}
    order = (["parent", "this"] if a.parent_lib else ["this"]) * a.rounds
    for who in order:
        env = dict(os.environ)
        if who == "parent":
            env["SOMHIP_LIB"] = os.path.abspath(a.parent_lib)
        p = subprocess.run([sys.executable, me, "--onecall-only", who, "--reps", str(a.reps)] + small, env=env, stdout=subprocess.PIPE,
                           text=True, check=True, timeout=600)
        for s in p.stdout.split("\n"):
            if s.startswith("JSON "):
                r = json.loads(s[5:])
                runs.setdefault(tuple(r["shape"]), []).append(r)
    out("== one call (somhip_som_batchmap, one bubble epoch, events off for the wall, on for the stages), children alternating")
    for shape, rs in runs.items():
        out("  %d x %d x %d over %d vectors" % shape)
        meds = {"parent": [], "this": []}
        for r in rs:
            meds[r["who"]].append(med(r["walls"]))
            out("    %-6s wall ms median %.3f of %s | group %.3f sums %.3f combine %.3f"
                % (r["who"], med(r["walls"]), fmt(r["walls"]), med(r["group"]), med(r["sums"]), med(r["combine"])))
        if meds["parent"]:
            spread = max(meds["parent"]) - min(meds["parent"])
            diff = med(meds["this"]) - med(meds["parent"])
            out("    parent's children among themselves: spread %.3f ms; this commit less the parent: %+.3f ms (%+.2f %%)"
                % (spread, diff, 100 * diff / med(meds["parent"])))
    eng = E.Engine(0)
    out("== this commit: the same epoch through begin / accumulate x k / finish")
    for xdim, ydim, dim, n, radii in shapes:
        units = xdim * ydim
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, units)[0]
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
        E.som_batchmap(cb, ds, 1, radii[0], qerror=False)
        want = cb.download()
        r0 = E.batchmap_radius(radii[0], 1, 0)
        out("  %d x %d x %d over %d vectors, radius %g" % (xdim, ydim, dim, n, radii[0]))
        for k in (1, 4, 16):
            per = (n + k - 1) // k

            def epoch(events):
                cb.upload(codes)
                eng.timing(events)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                E.batchmap_begin(cb)
                for first in range(0, n, per):
                    E.batchmap_accumulate(cb, ds, first, min(per, n - first), qerror=False)
                E.batchmap_finish(cb, r0, qerror=False)
                wall = (time.perf_counter() - t0) * 1e3
                st = eng.batchmap_timing() if events else None
                eng.timing(False)
                return wall, st
            epoch(False)
            assert np.array_equal(cb.download().view(np.uint32), want.view(np.uint32)), "pieces differ from the one call"
            walls = [epoch(False)[0] for _ in range(a.reps)]
            timed = [epoch(True)[1] for _ in range(a.reps)]
            out("    %2d pieces: wall ms median %.3f of %s | group %.3f (%d launches) sums %.3f combine %.3f"
                % (k, med(walls), fmt(walls), med([t["group"][1] for t in timed]), timed[0]["group"][0],
                   med([t["k_batchmap_sums"][1] for t in timed]), med([t["k_batchmap_combine"][1] for t in timed])))
        E.batchmap_end(cb)
        cb.close(); ds.close()
    eng.close()
    # the tool, end to end
    import tempfile
    from som_lvq_pak_amd import _lib, textio
    bsom = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "bsom")
    xdim, ydim, dim, n, radii = shapes[-1]
    ndev = C.c_int(0)
    _lib.load().somhip_device_count(C.byref(ndev))
    with tempfile.TemporaryDirectory() as tmp:
        m = textio.Entries()
        m.dim, m.topol, m.neigh, m.xdim, m.ydim = dim, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim
        m.points = E.gen_rows(9, 16, dim, n, xdim * ydim)[0]
        cod = os.path.join(tmp, "m.cod")
        textio.write_entries(cod, m)
        src = "gen:k=16,dim=%d,n=%d,seed=9" % (dim, n)
        out("== bsom end to end, %d x %d x %d, -din %s, 4 epochs from radius %g (process start to exit)" % (xdim, ydim, dim, src, radii[0]))
        variants = [[], ["-buffer", str((n + 3) // 4)], ["-buffer", str((n + 15) // 16)]]
        if ndev.value >= 2:
            variants += [["-gpus", "2"]] + ([["-gpus", str(ndev.value)]] if ndev.value > 2 else [])
        ref = None
        for extra in variants:
            walls = []
            for rep in range(a.reps):
                o = os.path.join(tmp, "o.cod")
                t0 = time.perf_counter()
                subprocess.run([bsom, "-cin", cod, "-din", src, "-cout", o, "-epochs", "4", "-radius", str(radii[0])] + extra, check=True,
                               stdout=subprocess.DEVNULL, timeout=600)
                walls.append((time.perf_counter() - t0) * 1e3)
                data = open(o, "rb").read()
                ref = ref or data
                assert data == ref, "bsom %s writes another file" % " ".join(extra)
            out("    %-16s wall ms median %.1f of %s (the plain run's file, byte for byte)" % (" ".join(extra) or "(plain)", med(walls), fmt(walls)))
        if ndev.value < 2:
            out("    one device visible: -gpus not timed (ranks that share a GPU say nothing about speed)")
    out("== ranks: bytes broadcast per epoch = G x the state (units x (dim + 1) x 8 + 16)")
    for units, dim in ((65536, 512), (1024, 128)):
        out("    %d x %d: state %.1f MB per rank's turn" % (units, dim + 1, (units * (dim + 1) * 8 + 16) / 1e6))


MISSING_CASES = lambda E, radii: (("bubble", E.NEIGH_BUBBLE, 1.0), ("bubble", E.NEIGH_BUBBLE, radii[0]), ("gaussian", E.NEIGH_GAUSSIAN, radii[0]))  # noqa: E731


def timed_epochs(E, eng, cb, ds, codes, radius, reps, train):
    """one warm-up epoch, `reps` on the host clock with events off, `reps` with the stage events on: (walls, group, sums, combine)"""
    def epoch(events):
        cb.upload(codes)
        eng.timing(events)
        eng.timing_reset()
        eng.sync()
        t0 = time.perf_counter()
        train(cb, ds, 1, radius, qerror=False)
        wall = (time.perf_counter() - t0) * 1e3
        st = eng.batchmap_timing() if events else None
        eng.timing(False)
        return wall, st
    epoch(False)
    walls = [epoch(False)[0] for _ in range(reps)]
    timed = [epoch(True)[1] for _ in range(reps)]
    return (walls, [t["group"][1] for t in timed], [t["k_batchmap_sums"][1] for t in timed], [t["k_batchmap_combine"][1] for t in timed])


def missing_child(E, eng, reps, shapes, who):
    """per shape and case the plain epoch, and with this commit's library the missing form on the same unmasked data: a JSON
    line each"""
    for xdim, ydim, dim, n, radii in shapes:
        ds = E.Dataset(eng, generate=(9, 16, dim, 0, n))
        codes = E.gen_rows(9, 16, dim, n, xdim * ydim)[0]
        for nname, neigh, radius in MISSING_CASES(E, radii):
            cb = E.Codebook(eng, codes, E.TOPOL_HEXA, neigh, xdim, ydim)
            forms = [("plain", E.som_batchmap)] + ([("missing", E.som_batchmap_missing)] if who == "this" else [])
            rows = {}
            for form, train in forms:
                walls, grp, sums, comb = timed_epochs(E, eng, cb, ds, codes, radius, reps, train)
                rows[form] = cb.download()
                print("JSON " + json.dumps({"who": who, "form": form, "shape": [xdim, ydim, dim, n], "case": "%s radius %g" % (nname, radius),
                                            "walls": walls, "group": grp, "sums": sums, "combine": comb}), flush=True)
            if "missing" in rows:
                assert np.array_equal(rows["plain"].view(np.uint32), rows["missing"].view(np.uint32)), "the missing form differs on unmasked data"
            cb.close()
        ds.close()


def missing_report(E, a, shapes, out):
    me = os.path.abspath(__file__)
    small = ["--small"] if a.small else []
    runs = {}
    order = (["parent", "this"] if a.parent_lib else ["this"]) * a.rounds
    for who in order:
        env = dict(os.environ)
        if who == "parent":
            env["SOMHIP_LIB"] = os.path.abspath(a.parent_lib)
        p = subprocess.run([sys.executable, me, "--missing-child", who, "--reps", str(a.reps)] + small, env=env, stdout=subprocess.PIPE,
                           text=True, check=True, timeout=900)
        for s in p.stdout.split("\n"):
            if s.startswith("JSON "):
                r = json.loads(s[5:])
                runs.setdefault((tuple(r["shape"]), r["case"]), []).append(r)
    out("== one epoch on unmasked generated vectors, hexa; children alternating between the parent's library and this commit's;")
    out("   per child: medians of %d calls (wall: events off; stages: events on)" % a.reps)
    for (shape, case), rs in runs.items():
        out("  %d x %d x %d over %d vectors, %s" % (shape + (case,)))
        m = {}
        for r in rs:
            key = (r["who"], r["form"])
            m.setdefault(key, {"wall": [], "sums": [], "combine": []})
            m[key]["wall"].append(med(r["walls"])); m[key]["sums"].append(med(r["sums"])); m[key]["combine"].append(med(r["combine"]))
            out("    %-6s %-7s wall ms median %.3f of %s | group %.3f sums %.3f combine %.3f"
                % (r["who"], r["form"], med(r["walls"]), fmt(r["walls"]), med(r["group"]), med(r["sums"]), med(r["combine"])))
        base = m.get(("parent", "plain")) or m[("this", "plain")]
        if ("parent", "plain") in m:
            for what in ("wall", "sums", "combine"):
                pv, tv = m[("parent", "plain")][what], m[("this", "plain")][what]
                out("    plain %-7s parent's children among themselves: spread %.3f ms (%.2f %%); this commit less the parent: %+.3f ms (%+.2f %%)"
                    % (what, max(pv) - min(pv), 100 * (max(pv) - min(pv)) / med(pv), med(tv) - med(pv), 100 * (med(tv) - med(pv)) / med(pv)))
        if ("this", "missing") in m:
            for what in ("sums", "combine"):
                bv, mv = base[what], m[("this", "missing")][what]
                out("    missing %-7s %.3f ms against the %s plain %.3f ms: ratio %.3f (plain spread %.2f %%, missing spread %.2f %%)"
                    % (what, med(mv), "parent's" if ("parent", "plain") in m else "this commit's", med(bv), med(mv) / med(bv),
                       100 * (max(bv) - min(bv)) / med(bv), 100 * (max(mv) - min(mv)) / med(mv)))
    # the tool, end to end, the parent's beside this commit's
    import tempfile
    from som_lvq_pak_amd import textio
    bsom = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin", "bsom")
    xdim, ydim, dim, n, radii = shapes[-1]
    with tempfile.TemporaryDirectory() as tmp:
        m = textio.Entries()
        m.dim, m.topol, m.neigh, m.xdim, m.ydim = dim, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim
        m.points = E.gen_rows(9, 16, dim, n, xdim * ydim)[0]
        cod = os.path.join(tmp, "m.cod")
        textio.write_entries(cod, m)
        src = "gen:k=16,dim=%d,n=%d,seed=9" % (dim, n)
        out("== bsom end to end, %d x %d x %d, -din %s, 4 epochs from radius %g (process start to exit), runs alternating" % (xdim, ydim, dim, src, radii[0]))
        variants = ([("parent", a.parent_bsom, [])] if a.parent_bsom else []) + [("this", bsom, []), ("this", bsom, ["-missing"])]
        walls, ref = {}, None
        for rnd in range(a.rounds):
            for who, exe, extra in variants:
                o = os.path.join(tmp, "o.cod")
                t0 = time.perf_counter()
                subprocess.run([exe, "-cin", cod, "-din", src, "-cout", o, "-epochs", "4", "-radius", str(radii[0])] + extra, check=True,
                               stdout=subprocess.DEVNULL, timeout=600)
                walls.setdefault((who, " ".join(extra)), []).append((time.perf_counter() - t0) * 1e3)
                data = open(o, "rb").read()
                ref = ref or data
                assert data == ref, "bsom %s %s writes another file" % (who, " ".join(extra))
        for (who, extra), w in walls.items():
            out("    %-6s bsom %-9s wall ms median %.1f of %s, spread %.1f (one file, byte for byte)" % (who, extra, med(w), fmt(w), max(w) - min(w)))
    # a masked epoch, per stage
    eng = E.Engine(0)
    out("== this commit: one epoch of somhip_som_batchmap_missing, 30 % of the components masked at random, hexa bubble (events on)")
    for i, (xdim, ydim, dim, n, radii) in enumerate(shapes):
        if i == 0 and not a.small:
            n = a.masked_large
        rs = np.random.RandomState(5)
        x = rs.standard_normal((n, dim)).astype(np.float32)
        mask = (rs.uniform(size=(n, dim)) < 0.3).astype(np.uint8)
        ds = E.Dataset(eng, x, mask=mask)
        codes = rs.standard_normal((xdim * ydim, dim)).astype(np.float32)
        cb = E.Codebook(eng, codes, E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim)
        walls, grp, sums, comb = timed_epochs(E, eng, cb, ds, codes, radii[0], a.reps, E.som_batchmap_missing)
        rest = med(walls) - med(grp) - med(sums) - med(comb)
        out("  %d x %d x %d over %d vectors, radius %g: wall ms (events off) median %.3f of %s | group %.3f sums %.3f combine %.3f | the rest, "
            "the masked search with the copies: %.3f ms = %.3f us a vector"
            % (xdim, ydim, dim, n, radii[0], med(walls), fmt(walls), med(grp), med(sums), med(comb), rest, 1e3 * rest / n))
        cb.close(); ds.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--online-only", default=None, help="(the child process) label of the library under SOMHIP_LIB")
    ap.add_argument("--batchmap-only", action="store_true", help="leave the online runs out")
    ap.add_argument("--small", action="store_true", help="one small shape: a rehearsal of the script, not a measurement")
    ap.add_argument("--pieces", action="store_true", help="the report on the epoch over data in pieces (see the top)")
    ap.add_argument("--rounds", type=int, default=3, help="--pieces: child processes per library")
    ap.add_argument("--onecall-only", default=None, help="(a --pieces child process) label of the library under SOMHIP_LIB")
    ap.add_argument("--missing", action="store_true", help="the report on the batch map over data with missing values (see the top)")
    ap.add_argument("--missing-child", default=None, help="(a --missing child process) label of the library under SOMHIP_LIB")
    ap.add_argument("--parent-bsom", default=None, help="--missing: the parent commit's bsom, beside its own library")
    ap.add_argument("--masked-large", type=int, default=16384, help="--missing: vectors of the masked epoch at the first shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [(24, 16, 40, 5000, (6.0, 1.0))] if a.small else SHAPES
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    from som_lvq_pak_amd import _lib, engine as E
    if a.online_only:                                   # the parent's library has no batch map: bind what it has
        for name in [k for k in _lib.SIGNATURES if "batchmap" in k]:
            del _lib.SIGNATURES[name]
    if a.missing_child or a.missing:
        if a.missing_child == "parent":                 # the parent's library has no missing form
            _lib.BATCHMAP_MISSING_SIGNATURES.clear()
        if a.missing_child:
            eng = E.Engine(0)
            missing_child(E, eng, a.reps, shapes, a.missing_child)
            eng.close()
        else:
            missing_report(E, a, shapes, out)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
        print(json.dumps({"lines": len(lines)}))
        return
    if a.onecall_only or a.pieces:
        if a.onecall_only == "parent":                  # ... nor the pieces' entry points
            for name in [k for k in _lib.SIGNATURES if k.startswith("somhip_batchmap_") and k != "somhip_batchmap_timing"] + \
                    ["somhip_som_batchmap_ranks", "somhip_comm_broadcast"]:
                del _lib.SIGNATURES[name]
        if a.onecall_only:
            eng = E.Engine(0)
            onecall_child(E, eng, a.reps, shapes, a.onecall_only)
            eng.close()
        else:
            pieces_report(E, a, shapes, out)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
        print(json.dumps({"lines": len(lines)}))
        return
    eng = E.Engine(0)
    if a.online_only:
        measure_online(E, eng, a.reps, shapes, out, a.online_only)
    else:
        measure_batchmap(E, eng, a.reps, shapes, out)
        if not a.batchmap_only:
            measure_online(E, eng, a.reps, shapes, out, "this commit")
    eng.close()
    if a.parent_lib and not a.online_only and not a.batchmap_only:
        cmd = [sys.executable, os.path.abspath(__file__), "--online-only", "parent", "--reps", str(a.reps)] + (["--small"] if a.small else [])
        p = subprocess.run(cmd, env=dict(os.environ, SOMHIP_LIB=os.path.abspath(a.parent_lib)), stdout=subprocess.PIPE, text=True, check=True)
        for s in p.stdout.rstrip("\n").split("\n"):
            out(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"lines": len(lines)}))


if __name__ == "__main__":
    main()
