"""Batch Robust Soft LVQ (K13) on runs longer than one chunk of its production walk, and at the shortened chunk.

somhip_rslvq_train and somhip_rslvq_search walk a run in chunks of rslvq_chunk(row groups) samples (host_rslvq.inc,
rslvq_walk): 4096 for every codebook up to 8192 rows, 4032 from 8193 rows on (ld = 8256), so that the Q chunk stays within
256 MiB.  The longest run of test_rslvq.py is 1500 samples, so rslvq_walk has never gone round with off > 0: neither
k_rslvq_sums<true> behind it, nor smp = off + i in the posterior, nor (first % n + off) % n in the distance and sums stages;
the stage entries at chunk 64 have loops of their own.  A wrong offset in any of them reads in bounds and returns plausible
figures, so the runs here cross the chunk's edge over a data set whose labels and values differ between run sample s and
run sample s - chunk for every s (test_samples_a_chunk_apart_differ), and every sample is compared with the numpy replay
(rslvq_replay) within the bounds it derives; what the definition promises bit for bit -- the chunk is invisible, an epoch
equals its stages -- is compared by bit pattern.  The chunk is read from engine.rslvq_chunk, which is host arithmetic; the
shapes follow it.  The second part of test_rslvq_layouts.py's issue."""
import math

import numpy as np
import pytest

import rslvq_replay as R
import test_rslvq as TR
from test_lvq_family_chunks import cycle_labels
from test_rslvq import built                                           # noqa: F401  (fixture)

f32, f64 = np.float32, np.float64
bits32, bits64 = TR.bits32, TR.bits64

ROWS, DIM, CLASSES, N_ROWS = 12, 5, 4, 1000                            # the rule's chunk: one row group, every long run wraps
SIGMA2, ALPHA = 2.0, 5.0
RUNS = ["a sample short", "the chunk", "a sample more", "two chunks and a sample, wrapped"]
SHORT_ROWS, SHORT_DIM, SHORT_N_ROWS = 8193, 2, 61                      # the first codebook that shortens the chunk
SHORT_FIRST = SHORT_N_ROWS - 2


def rule_chunk(rows):
    from som_lvq_pak_amd import engine
    return engine.rslvq_chunk(rows)[0]


def runs():
    """(first, n) per entry of RUNS: one sample below the chunk, the chunk, one sample into the second; two chunks and a
    sample, wrapping after two rows"""
    ch = rule_chunk(ROWS)
    return [(0, ch - 1), (0, ch), (0, ch + 1), (N_ROWS - 2, 2 * ch + 1)]


_cases = {}


def chunk_case(rows, dim, n_rows):
    """(codes, code labels, data, data labels, the replay's posteriors by data row): Gaussian rows and data, code labels
    r % 4, data labels that differ a chunk apart; built once per shape and left unchanged"""
    if rows not in _cases:
        rs = np.random.RandomState(9300 + rows + dim)
        c = rs.standard_normal((rows, dim)).astype(f32)
        cl = (np.arange(rows) % CLASSES).astype(np.int32)
        x = (rs.standard_normal((n_rows, dim)) * 1.2).astype(f32)
        dl = cycle_labels(n_rows, rule_chunk(rows) % n_rows)
        for a in (c, cl, x, dl):
            a.setflags(write=False)
        _cases[rows] = (c, cl, x, dl, R.posterior_by_row(c, cl, x, dl, SIGMA2))
    return _cases[rows]


def chain(values):
    s = f64(0.0)
    for v in values:
        s = s + v
    return s


# ------------------------------------------------------------------------------------------------ without a GPU
def test_samples_a_chunk_apart_differ(built):
    """no run sample s shares its data row, its label or its values with run sample s - chunk: a dropped `+ off` cannot
    return the right figures by coincidence.  The shapes are what the rule makes of them."""
    from som_lvq_pak_amd import engine as E
    assert E.rslvq_chunk(ROWS) == (4096, 64) and runs() == [(0, 4095), (0, 4096), (0, 4097), (998, 8193)]
    c, cl, x, dl, by_row = chunk_case(ROWS, DIM, N_ROWS)
    ch = rule_chunk(ROWS)
    assert set(dl.tolist()) == set(range(CLASSES)) == set(cl.tolist()) and np.bincount(dl).tolist() == [252, 248, 252, 248]
    assert (dl != dl[(np.arange(N_ROWS) + ch) % N_ROWS]).all() and len(np.unique(x, axis=0)) == N_ROWS
    for first, n in runs():
        s = np.arange(ch, n)
        a, b = (first + s) % N_ROWS, (first + s - ch) % N_ROWS
        assert (a != b).all() and (dl[a] != dl[b]).all() and (x[a] != x[b]).any(axis=1).all()
        assert (by_row["pown"][a] != by_row["pown"][b]).all()
    assert 1e-6 < by_row["pown"].min() and by_row["pown"].max() < 1 - 1e-6 and 0 < by_row["correct"].sum() < N_ROWS

    assert E.rslvq_chunk(SHORT_ROWS) == (4032, 8256) and E.rslvq_chunk(SHORT_ROWS - 1) == (4096, 8192)
    c, cl, x, dl, by_row = chunk_case(SHORT_ROWS, SHORT_DIM, SHORT_N_ROWS)
    ch = rule_chunk(SHORT_ROWS)
    assert set(dl.tolist()) == {0, 1, 2} <= set(cl.tolist())
    a, b = (SHORT_FIRST + ch) % SHORT_N_ROWS, SHORT_FIRST                # the second chunk's one sample and the first's first
    assert a != b and dl[a] != dl[b] and (x[a] != x[b]).any() and by_row["pown"][a] != by_row["pown"][b]
    assert 0.2 < by_row["pown"].min() and by_row["pown"].max() < 0.3    # four classes of equal size over the same cloud
    assert 0 < by_row["correct"].sum() < SHORT_N_ROWS


def test_the_by_row_helpers_equal_the_replay_of_the_run():
    """posterior_of_run of posterior_by_row is posterior over the run, and sums_by_row_longdouble is sums_longdouble of
    it: the same sums (np.longdouble adds in another order: within its own rounding) and the same bound"""
    c, cl, x, dl = TR.clusters(3, 40, 7, 5, sep=1.0)
    first, n = 38, 130                                                 # wraps three times
    p = R.posterior(c, cl, x, dl, 2.0, first, n)
    by_row = R.posterior_by_row(c, cl, x, dl, 2.0)
    q = R.posterior_of_run(by_row, first, n)
    assert set(p) == set(q)
    for key in p:
        assert p[key].dtype == q[key].dtype and (p[key].view(np.uint8) == q[key].view(np.uint8)).all(), key
    G, cc, bG, bc = R.sums_longdouble(p["q"], x, first)
    G2, cc2, bG2, bc2 = R.sums_by_row_longdouble(by_row["q"], x, first, n)
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63                      # n additions at 2^-63 against (2 n + 16) 2^-52: 2^-12
    assert (np.abs(G - G2) <= bG * 2.0 ** -11).all() and (np.abs(cc - cc2) <= bc * 2.0 ** -11).all()
    assert np.allclose(bG, bG2, rtol=1e-12, atol=0) and np.allclose(bc, bc2, rtol=1e-12, atol=0)


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


def within(what, err, tol):
    ratio = float((err / tol).max())
    print("rslvq chunks", what, "largest difference / bound: %.6g" % ratio)
    assert (err <= tol).all(), (what, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(RUNS)), ids=[r.replace(" ", "_").replace(",", "") for r in RUNS])
def test_a_run_across_the_rules_chunk(E, eng, which):
    """4095, 4096, 4097 and 8193 samples on 12 rows: the posteriors at the rule's chunk equal those at chunk 64 and follow
    the replay sample by sample; rslvq_search (rslvq_walk without sums) reports them; the sums of that Q do not know the
    chunk; one epoch of rslvq_train (rslvq_walk with sums) equals its stages at chunk 64 and follows the replay"""
    c, cl, x, dl, by_row = chunk_case(ROWS, DIM, N_ROWS)
    first, n = runs()[which]
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    p = R.posterior_of_run(by_row, first, n)
    bq, bc, bp, _ = R.posterior_bounds(p)
    got = E.rslvq_posterior(cb, ds, SIGMA2, first, n)
    small = E.rslvq_posterior(cb, ds, SIGMA2, first, n, chunk=64)
    for key in ("q", "cost", "pown"):
        assert (bits64(got[key]) == bits64(small[key])).all(), key
    assert (got["correct"] == small["correct"]).all()
    for g in (got, small):
        assert (g["correct"] == p["correct"]).all(), np.flatnonzero(g["correct"] != p["correct"])[:5]
        within((n, "q"), np.abs(g["q"][:, :ROWS] - p["q"]), bq)
        within((n, "cost"), np.abs(g["cost"] - p["cost"]), bc)
        within((n, "pown"), np.abs(g["pown"] - p["pown"]), bp)
        assert (bits64(g["q"][:, ROWS:]) == 0).all()

    scost, scorrect, spown = E.rslvq_search(cb, ds, SIGMA2, first, n)
    assert (bits64(spown) == bits64(got["pown"])).all() and scorrect == int(got["correct"].sum())
    assert bits64(scost) == bits64(chain(got["cost"]) / f64(n))

    G, cc = E.rslvq_sums(cb, ds, got["q"], first, n)
    G2, cc2 = E.rslvq_sums(cb, ds, got["q"], first, n, chunk=64)
    assert (bits64(G) == bits64(G2)).all() and (bits64(cc) == bits64(cc2)).all()
    wG, wc, bG, bcc = R.sums_longdouble(got["q"][:, :ROWS], x, first)
    within((n, "G of the device's Q"), np.abs(G - wG).astype(f64), bG)
    within((n, "c of the device's Q"), np.abs(cc - wc).astype(f64), bcc)

    tcost, tcorrect = E.rslvq_train(cb, ds, 1, ALPHA, SIGMA2, first=first, n=n)
    walked = cb.download()
    cb.upload(c)
    ecost, ecorrect = TR.stage_epoch(E, cb, ds, E.glvq_alpha(ALPHA, 1, 0), SIGMA2, first, n, 64)
    assert (bits32(cb.download()) == bits32(walked)).all() and bits64(tcost)[0] == bits64(ecost) and tcorrect[0] == ecorrect
    assert bits64(tcost)[0] == bits64(scost) and tcorrect[0] == scorrect and (bits32(walked) != bits32(c)).any(axis=1).all()
    # the replay's sums of the replay's q; the device's lie within the combine bound of sums of a Q that lies within bq
    wG, wc, bG, bcc = R.sums_longdouble(p["q"], x, first)
    ax = np.abs(x[R.run_rows(N_ROWS, first, n)]).astype(f64)
    want, bound = R.update_longdouble(c, wG, wc, R.alpha_at(ALPHA, 1, 0), SIGMA2, n, bG + bq.T @ ax, bcc + bq.sum(axis=0))
    within((n, "rows after an epoch"), np.abs(walked.astype(np.longdouble) - want), bound)
    cb.close(); ds.close()


@pytest.mark.gpu
def test_an_epoch_of_two_chunks_and_a_sample_launches_three_of_each(E, eng):
    c, cl, x, dl, _ = chunk_case(ROWS, DIM, N_ROWS)
    first, n = runs()[-1]
    assert n == 2 * rule_chunk(ROWS) + 1
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    eng.timing(True); eng.timing_reset()
    E.rslvq_train(cb, ds, 1, ALPHA, SIGMA2, first=first, n=n, stats=False)
    t = eng.rslvq_timing()
    eng.timing(False)
    assert t["distances"][0] == 3 and t["k_rslvq_posterior"][0] == 3 and t["k_rslvq_sums"][0] == 3 and t["k_rslvq_update"][0] == 1
    cb.close(); ds.close()


@pytest.mark.gpu
def test_the_shortened_chunk(E, eng):
    """8193 rows (129 row groups, ld = 8256, a chunk of 4032 samples) and 4033 samples from row 59 of 61: two chunks, the
    second of one sample.  Q is not downloaded (266 MB).  rslvq_search's pown, correct and cost against the replay by data
    row; an epoch of rslvq_train reports that cost and correct and leaves rows within update_longdouble's allowance of
    the replay's, whose [G | c] is formed from the 61 distinct rows weighted by how often the run takes each; twice"""
    c, cl, x, dl, by_row = chunk_case(SHORT_ROWS, SHORT_DIM, SHORT_N_ROWS)
    ch = rule_chunk(SHORT_ROWS)
    first, n = SHORT_FIRST, ch + 1
    assert E.rslvq_chunk(SHORT_ROWS) == (4032, 8256) and (first, n) == (59, 4033)
    r = R.run_rows(SHORT_N_ROWS, first, n)
    bq, bc, bp, _ = R.posterior_bounds(by_row)                          # by data row
    cb, ds = E.Codebook(eng, c, labels=cl), E.Dataset(eng, x, labels=dl)
    scost, scorrect, spown = E.rslvq_search(cb, ds, SIGMA2, first, n)
    within(("short", "pown"), np.abs(spown - by_row["pown"][r]), bp[r])
    assert scorrect == int(by_row["correct"][r].sum())
    wcost = math.fsum(by_row["cost"][r]) / n
    within(("short", "cost"), np.abs(f64(scost - wcost))[None], np.array([bc[r].sum() / n + n * R.U * abs(wcost)]))

    w = np.bincount(r, minlength=SHORT_N_ROWS).astype(f64)
    assert w.sum() == n and w.min() >= n // SHORT_N_ROWS
    wG, wc, bG, bcc = R.sums_by_row_longdouble(by_row["q"], x, first, n)
    bqw = bq * w[:, None]
    want, bound = R.update_longdouble(c, wG, wc, R.alpha_at(ALPHA, 1, 0), SIGMA2, n, bG + bqw.T @ np.abs(x).astype(f64), bcc + bqw.sum(axis=0))
    for again in range(2):
        cb.upload(c)
        tcost, tcorrect = E.rslvq_train(cb, ds, 1, ALPHA, SIGMA2, first=first, n=n)
        assert bits64(tcost)[0] == bits64(scost) and tcorrect[0] == scorrect
        rows = cb.download()
        if again:
            assert (bits32(rows) == bits32(before)).all()
        before = rows
    within(("short", "rows after an epoch"), np.abs(rows.astype(np.longdouble) - want), bound)
    assert (bits32(rows) != bits32(c)).any(axis=1).all()
    cb.close(); ds.close()
