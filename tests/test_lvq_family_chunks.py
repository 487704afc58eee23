"""The GLVQ family (K9 glvq, K11 grlvq, K12 gmlvq) on runs longer than one launch of the class-wise scan.

GLVQ_CHUNK = 16384 (csrc/host_proto.inc) cuts the scan in one loop, class_scan_walk, which glvq_search_stage,
grlvq_search_stage (host_grlvq.inc) and gmlvq_search_stage (host_gmlvq.inc) walk with their own tiles -- and the list route
is cut again, at 4096 samples, by knn_chunk_keys (csrc/host_scan.inc), after which k_glvq_pick adds the chunk's offset and the
remainder goes through class_scan_walk with its own list.  A wrong offset in any of them reads in bounds and returns plausible winners, so
the runs here cross every one of those edges over a data set of 5000 rows whose labels and values differ between run
sample s and run sample s - 16384 for every s (test_samples_a_chunk_apart_differ), and the winners and distance bits are
compared with the replays.  Neither constant is exposed by the library: test_the_chunk_sizes_are_the_sources checks them
against the source, so the shapes here have to follow a change.  The second part of test_lvq_family_layouts.py's issue."""
import os
import re

import numpy as np
import pytest

import glvq_replay as G
import gmlvq_replay as M
import grlvq_replay as R
import test_glvq as TG
from conftest import ROOT
from test_glvq import built                                            # noqa: F401  (fixture)

f32, f64 = np.float32, np.float64
bits32, bits64 = TG.bits32, TG.bits64

GLVQ_CHUNK = 16384                                                     # csrc/host_proto.inc
KNN_CHUNK = 4096                                                       # csrc/host_scan.inc:762, knn_chunk_keys at knn <= 8
N_ROWS = 5000                                                          # data rows: every long run wraps several times
CLASSES = 4
DIRECT_SHAPES = [(70, 5), (1030, 3)]
# one sample below the chunk, the chunk, one sample into the second; two chunks and a sample, wrapping after two rows
RUNS = [(0, GLVQ_CHUNK - 1), (0, GLVQ_CHUNK), (0, GLVQ_CHUNK + 1), (N_ROWS - 2, 2 * GLVQ_CHUNK + 1)]
SUMS_SHAPE = (6, 5)
ALPHA, EPS = 5.0, 0.5


def cycle_labels(n_rows, shift):
    """labels in [0, 4) with label[r] != label[(r + shift) % n_rows] for every r: along every orbit of r -> r + shift the
    labels alternate, the orbit's last row (orbits may be odd) takes a third one"""
    lab = np.full(n_rows, -1, dtype=np.int32)
    orbit = 0
    for start in range(n_rows):
        if lab[start] >= 0:
            continue
        r, i, walk = start, 0, []
        while lab[r] < 0:
            lab[r] = i % 2 + 2 * (orbit % 2)
            walk.append(r)
            r, i = (r + shift) % n_rows, i + 1
        if len(walk) % 2:
            lab[walk[-1]] = (2 + 2 * (orbit % 2)) % 4
        orbit += 1
    return lab


_cases = {}


def chunk_case(rows, dim):
    """(codes, code labels, data, data labels): Gaussian rows and data, code labels r % 4, data labels cycle_labels; built
    once per shape and left unchanged"""
    if (rows, dim) not in _cases:
        rs = np.random.RandomState(9000 + rows + dim)
        c = rs.standard_normal((rows, dim)).astype(f32)
        cl = (np.arange(rows) % CLASSES).astype(np.int32)
        x = (rs.standard_normal((N_ROWS, dim)) * 1.2).astype(f32)
        dl = cycle_labels(N_ROWS, GLVQ_CHUNK % N_ROWS)
        for a in (c, cl, x, dl):
            a.setflags(write=False)
        _cases[(rows, dim)] = (c, cl, x, dl)
    return _cases[(rows, dim)]


_winners = {}


def winners(key, search):
    """the replay's search over the 5000 data rows, once per case: a sample's winners depend on its data row alone, so run
    sample s of any range has those of row (first + s) % 5000"""
    if key not in _winners:
        _winners[key] = search()
    return _winners[key]


def of_run(per_row, first, n):
    r = (first + np.arange(n)) % N_ROWS
    return tuple(a[r] for a in per_row)


def same_search(got, want, what):
    dp, ip, dm, im = got[:4]
    assert (ip == want[1]).all() and (im == want[3]).all(), (what, np.flatnonzero((ip != want[1]) | (im != want[3]))[:5])
    assert (bits32(dp) == bits32(want[0])).all() and (bits32(dm) == bits32(want[2])).all(), what


# ------------------------------------------------------------------------------------------------ without a GPU
def test_the_chunk_sizes_are_the_sources():
    src = os.path.join(ROOT, "som_lvq_pak_amd", "csrc")
    proto = open(os.path.join(src, "host_proto.inc")).read()
    assert int(re.search(r"constexpr int64_t GLVQ_CHUNK = (\d+);", proto).group(1)) == GLVQ_CHUNK
    scan = open(os.path.join(src, "host_scan.inc")).read()
    body = scan[scan.index("static int knn_chunk_keys("):]
    assert int(re.search(r"const int64_t CH = std::min<int64_t>\((\d+), count\);", body).group(1)) == KNN_CHUNK
    assert proto.count("off += GLVQ_CHUNK") == 1                        # one loop, class_scan_walk, and all three searches walk it
    for name in ("host_glvq.inc", "host_grlvq.inc", "host_gmlvq.inc"):
        text = open(os.path.join(src, name)).read()
        assert "class_scan_walk(" in text and "GLVQ_CHUNK" not in text, name
    assert GLVQ_CHUNK % N_ROWS != 0 and GLVQ_CHUNK % 32 == 0


def test_samples_a_chunk_apart_differ(built):
    """no run sample s shares its data row, its label or its values with run sample s - 16384, from either first row the
    tests use: a dropped `+ off` cannot return the right answer by coincidence.  And every shape below takes the direct
    route by the plan, so sums and training run the chunked scan."""
    from som_lvq_pak_amd import engine as E
    for rows, dim in DIRECT_SHAPES + [SUMS_SHAPE]:
        c, cl, x, dl = chunk_case(rows, dim)
        assert set(dl.tolist()) == set(range(CLASSES)) == set(cl.tolist())
        for first, n in RUNS + [(N_ROWS - 2, GLVQ_CHUNK + 1), (3, 20000)]:
            if n <= GLVQ_CHUNK:
                continue
            s = np.arange(GLVQ_CHUNK, n)
            a, b = (first + s) % N_ROWS, (first + s - GLVQ_CHUNK) % N_ROWS
            assert (a != b).all() and (dl[a] != dl[b]).all() and (x[a] != x[b]).any(axis=1).all()
        assert all(E.glvq_plan(rows, dim, n) == E.GLVQ_DIRECT for _, n in RUNS)
    assert len(np.unique(chunk_case(*SUMS_SHAPE)[2], axis=0)) == N_ROWS


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", DIRECT_SHAPES)
def test_direct_searches_across_the_scan_chunk(E, eng, rows, dim):
    """glvq_search on the direct route, grlvq_search and gmlvq_search at rank 2 over 16383, 16384, 16385 and 32769 samples:
    winners and distance bits of every sample"""
    c, cl, x, dl = chunk_case(rows, dim)
    rs = np.random.RandomState(rows)
    lam = rs.uniform(0.05, 2.0, size=dim).astype(f32)
    om = (0.5 * rs.standard_normal((2, dim))).astype(f32)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    want = winners(("glvq", rows, dim), lambda: G.search(c, cl, x, dl))
    wantl = winners(("grlvq", rows, dim), lambda: R.search(c, cl, x, dl, lam))
    wantm = winners(("gmlvq", rows, dim), lambda: M.search(c, cl, x, dl, om))
    assert RUNS[-1] == (4998, 32769)
    for first, n in RUNS:
        got = E.glvq_search(cb, ds, first, n, E.GLVQ_DIRECT)
        assert got[4] == n
        same_search(got, of_run(want, first, n), ("glvq", first, n))
        same_search(E.grlvq_search(cb, ds, lam, first, n), of_run(wantl, first, n), ("grlvq", first, n))
        same_search(E.gmlvq_search(cb, ds, om, first, n), of_run(wantm, first, n), ("gmlvq", first, n))
    cb.close(); ds.close()


@pytest.mark.gpu
def test_list_route_across_its_chunks_with_a_partial_remainder(E, eng):
    """4095, 4096, 4097 and 8193 samples on 70 Gaussian rows of four classes: most top-8 lists hold both roles, the others
    go through the remainder, 0 < rem < n.  The remainder's order is not defined: the keys alone are compared."""
    c, cl, x, dl = chunk_case(70, 5)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    want = winners(("glvq", 70, 5), lambda: G.search(c, cl, x, dl))
    for first, n in ((0, KNN_CHUNK - 1), (0, KNN_CHUNK), (0, KNN_CHUNK + 1), (N_ROWS - 2, 2 * KNN_CHUNK + 1)):
        got = E.glvq_search(cb, ds, first, n, E.GLVQ_LIST)
        same_search(got, of_run(want, first, n), ("list", first, n))
        assert 0 < got[4] < n, (n, got[4])
    cb.close(); ds.close()


def remainder_case(mixed):
    """test_glvq's test_list_route_without_the_other_role_goes_through_the_remainder over 5000 data rows: forty rows of
    class 0 beside every sample, thirty rows of the other classes far away -- no top-8 list holds both roles.  mixed: every
    second data row moved next to the far rows, where the lists of classes 1 .. 3 hold both."""
    rs = np.random.RandomState(40)
    c = (50.0 + rs.standard_normal((70, 5))).astype(f32)
    c[:40] = (0.01 * rs.standard_normal((40, 5))).astype(f32)
    cl = (1 + np.arange(70) % 3).astype(np.int32)
    cl[:40] = 0
    x = (0.01 * rs.standard_normal((N_ROWS, 5))).astype(f32)
    if mixed:
        x[::2] += 50.0
    return c, cl, x, cycle_labels(N_ROWS, GLVQ_CHUNK % N_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True])
def test_list_route_with_a_remainder_longer_than_a_scan_chunk(E, eng, mixed):
    """the remainder is the whole run (16385 and 20000 samples: rem == n, two launches of the listed scan, the only place
    where k_glvq_pack_listed and the scan see sel + off), or about half of 20000 samples (n / 2 <= rem < n)"""
    c, cl, x, dl = remainder_case(mixed)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    want = G.search(c, cl, x, dl)
    for first, n in ((3, 20000),) if mixed else ((3, GLVQ_CHUNK + 1), (N_ROWS - 2, 20000)):
        got = E.glvq_search(cb, ds, first, n, E.GLVQ_LIST)
        same_search(got, of_run(want, first, n), ("list", mixed, first, n))
        if mixed:
            assert n // 2 <= got[4] < n, got[4]
        else:
            assert got[4] == n > GLVQ_CHUNK
    cb.close(); ds.close()


_stages = {}


def sums_replays(trainer):
    """one replayed epoch of a trainer at n = 16385 over 6 rows of dim 5 from first row 4998: (rows, metric, cost, correct,
    the stage results), shared by the sums and the training test.  (About a second each: the replays' sums are Python loops
    over the samples.)"""
    if trainer not in _stages:
        c, cl, x, dl = chunk_case(*SUMS_SHAPE)
        first, n = N_ROWS - 2, GLVQ_CHUNK + 1
        lam, om = metrics_of_sums()
        a_t, e_t = R.rate_at(ALPHA, 1, 0), R.rate_at(EPS, 1, 0)
        if trainer == "glvq":
            rows, cost, correct, S = G.epoch(c, cl, x, dl, a_t, 0.0, first, n)
            out = (rows, None, cost, correct, S)
        elif trainer == "grlvq":
            out = R.epoch(c, cl, x, dl, lam, a_t, e_t, 0.0, first, n)
        else:
            out = M.epoch(c, cl, x, dl, om, a_t, e_t, 0.0, first, n)
        _stages[trainer] = out
    return _stages[trainer]


def metrics_of_sums():
    rs = np.random.RandomState(65)
    return rs.uniform(0.05, 0.5, size=SUMS_SHAPE[1]).astype(f32), rs.uniform(-0.3, 0.3, size=(2, SUMS_SHAPE[1])).astype(f32)


@pytest.mark.gpu
@pytest.mark.parametrize("trainer", ["glvq", "grlvq", "gmlvq"])
def test_sums_and_an_epoch_past_the_scan_chunk(E, eng, trainer):
    """n = 16385 = GLVQ_CHUNK + 1 = 4 * GMLVQ_BLOCK + 1 from first row 4998, 6 rows, dim 5: the counts, S+, S-, cost, correct
    and the relevance gradient or Gm -- five 4096-sample blocks, the last of one sample, beside the second scan chunk -- and
    one epoch of the trainer, all by bit pattern"""
    c, cl, x, dl = chunk_case(*SUMS_SHAPE)
    first, n = N_ROWS - 2, GLVQ_CHUNK + 1
    assert n == 4 * M.BLOCK + 1 and E.glvq_plan(*SUMS_SHAPE, n) == E.GLVQ_DIRECT
    lam, om = metrics_of_sums()
    rows, metric, cost, correct, S = sums_replays(trainer)
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    if trainer == "glvq":
        got, keys = E.glvq_sums(cb, ds, first, n), ()
        gcost, gcorrect = E.glvq_train(cb, ds, 1, ALPHA, first=first, n=n)
    elif trainer == "grlvq":
        got, keys = E.grlvq_sums(cb, ds, lam, first, n), ("rel_plus", "rel_minus", "grad")
        gmetric, gcost, gcorrect = E.grlvq_train(cb, ds, 1, ALPHA, EPS, lam, first=first, n=n)
    else:
        got, keys = E.gmlvq_sums(cb, ds, om, first, n), ("grad",)
        gmetric, gcost, gcorrect = E.gmlvq_train(cb, ds, 1, ALPHA, EPS, om, first=first, n=n)
    assert (got["n_plus"] == S["n_plus"]).all() and (got["n_minus"] == S["n_minus"]).all() and got["n_plus"].sum() == n
    for key in ("sums_plus", "sums_minus", "cost") + keys:
        assert (bits64(got[key]) == bits64(S[key])).all(), (key, np.argwhere(bits64(got[key]) != bits64(S[key]))[:5])
    assert got["correct"] == correct == gcorrect[0] and bits64(gcost)[0] == bits64(cost)[0]
    assert (bits32(cb.download()) == bits32(rows)).all() and (bits32(rows) != bits32(c)).any()
    if metric is not None:
        assert (bits32(gmetric) == bits32(metric)).all() and (bits32(gmetric) != bits32(lam if trainer == "grlvq" else om)).any()
    cb.close(); ds.close()
