"""sammon past the first chunk of its centre kernel, on the capped grid of its error kernel, and at whole dimension chunks.

The reference is tests/sammon_replay.py (pinned against the recorded reference runs by tests/test_sammon.py); x and y are
compared by bit pattern.  The shapes are chosen against these constants of kernels/sammon.hpp and host_sammon.inc, read
from the source by test_the_constants_are_what_the_shapes_assume:

    SAMMON_CENTRE_CHUNK = 2048   k_sammon_centre carries its two ordered float sums from one chunk of rows to the next:
                                 2048 rows are one whole chunk, 2049 and 2050 a second chunk of one and of two rows, 4097
                                 three chunks, the last of one row
    min(noc - 1, 2048)           workgroups of k_sammon_error, workgroup b takes j = 1 + b, 1 + b + 2048, ...: at 2049 rows
                                 every workgroup has one j, at 2050 workgroup 0 takes j = 1 and j = 2049
    SAMMON_DCHUNK = 32           components per staging round of k_sammon_dist: 32 and 64 are whole rounds, 65 one over

The mapping error is not the reference's fp32 running sum (the engine does not claim that one): it is the same float32
terms per pair, ee * ee / d and d, summed exactly and divided in float64.  The engine adds these non-negative terms in
float64 in some order, n - 1 additions per sum with n = noc (noc - 1) / 2, each off by at most 2^-53 relative, and
divides once: the relative difference is at most (2 (n - 1) + 1) 2^-53."""
import functools
import math
import os
import re

import numpy as np
import pytest

import sammon_replay as R
import test_sammon as TS
from test_sammon import _case_rows, eng  # noqa: F401  (eng: the module's engine fixture)

CENTRE_CHUNK, ERROR_BLOCKS, DCHUNK = 2048, 2048, 32
LARGE_RLENS = (0, 1, 3)


@functools.lru_cache(maxsize=None)
def replayed(noc, dim, rlens):
    """(rows, x0, y0, D, {rlen: (x, y)}) of one replay run: made once per session and never written to"""
    rows = _case_rows(noc, dim)
    D = R.distances(rows)
    assert len(R.zero_pairs(D)) == 0
    x0, y0 = R.initial_table(noc, 11 + noc)
    _, _, snap = R.iterate(x0, y0, D, max(rlens), snapshots=rlens)
    for a in (rows, x0, y0, D) + tuple(v for xy in snap.values() for v in xy):
        a.setflags(write=False)
    return rows, x0, y0, D, snap


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def exact_error(x, y, D):
    """sum of the float32 terms ee * ee / d over sum of the float32 d, pairs k < j: exact sums, one float64 division"""
    n = x.shape[0]
    j, k = np.nonzero(np.tril(np.ones((n, n), dtype=bool), -1))
    with np.errstate(all="ignore"):
        d = D[j, k]
        xd, yd = x[j] - x[k], y[j] - y[k]
        ee = d - np.sqrt(xd.astype(np.float64) * xd.astype(np.float64) + (yd * yd).astype(np.float64)).astype(np.float32)
        terms = ee * ee / d
    assert terms.dtype == np.float32 and d.dtype == np.float32 and (terms >= 0).all() and (d > 0).all()
    return math.fsum(terms.astype(np.float64).tolist()) / math.fsum(d.astype(np.float64).tolist())


# ------------------------------------------------------------------ without a GPU
def test_the_constants_are_what_the_shapes_assume():
    src = os.path.join(TS.ROOT, "som_lvq_pak_amd", "csrc")
    kern = open(os.path.join(src, "kernels", "sammon.hpp")).read()
    assert int(re.search(r"constexpr int SAMMON_CENTRE_CHUNK = (\d+);", kern).group(1)) == CENTRE_CHUNK
    assert int(re.search(r"constexpr int SAMMON_TILE = \d+, SAMMON_DCHUNK = (\d+);", kern).group(1)) == DCHUNK
    assert re.search(r"for \(int j = 1 \+ blockIdx\.x; j < noc; j \+= gridDim\.x\)", kern)
    host = open(os.path.join(src, "host_sammon.inc")).read()
    assert int(re.search(r"err_blocks = \(unsigned\)std::min<int>\(noc - 1, (\d+)\);", host).group(1)) == ERROR_BLOCKS


def test_the_exact_error_is_near_the_reference_number():
    """the reference of the mapping-error test against the replay's fp32 running sum, at a size where that sum is good"""
    rows, x0, y0, D, snap = replayed(65, 3, (1, 2, 3))
    want = R.iterate(x0, y0, D, 3, errors=True)[2]
    for it in (1, 2, 3):
        got = exact_error(snap[it][0], snap[it][1], D)
        assert abs(got - float(want[it - 1])) <= (2 * (65 * 64 // 2) + 1) * 2.0 ** -24 * got   # two fp32 running sums, one division


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("noc", [CENTRE_CHUNK, CENTRE_CHUNK + 1, CENTRE_CHUNK + 2])
def test_the_centre_sum_crosses_its_chunk(noc, eng):
    from som_lvq_pak_amd import engine as E
    rows, x0, y0, _, snap = replayed(noc, 3, LARGE_RLENS)
    cb = E.Codebook(eng, rows)
    for rlen in LARGE_RLENS:
        x, y = E.sammon(cb, x0, y0, rlen)
        assert same_bits(x, snap[rlen][0]), (rlen, "x")
        assert same_bits(y, snap[rlen][1]), (rlen, "y")
    cb.close()


@pytest.mark.gpu
def test_three_centre_chunks_the_last_of_one_row(eng):
    from som_lvq_pak_amd import engine as E
    noc = 2 * CENTRE_CHUNK + 1
    rows, x0, y0, _, snap = replayed(noc, 2, (1,))
    cb = E.Codebook(eng, rows)
    x, y = E.sammon(cb, x0, y0, 1)
    cb.close()
    assert same_bits(x, snap[1][0]) and same_bits(y, snap[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [DCHUNK, 2 * DCHUNK, 2 * DCHUNK + 1])
def test_whole_dimension_chunks(dim, eng):
    from som_lvq_pak_amd import engine as E
    rows, x0, y0, _, snap = replayed(65, dim, (1, 7))
    cb = E.Codebook(eng, rows)
    assert len(E.sammon_zero_pairs(cb)) == 0
    for rlen in (1, 7):
        x, y = E.sammon(cb, x0, y0, rlen)
        assert same_bits(x, snap[rlen][0]) and same_bits(y, snap[rlen][1]), rlen
    cb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("noc", [2, 65, ERROR_BLOCKS + 1, ERROR_BLOCKS + 2])
def test_mapping_error_within_its_summation_bound(noc, eng):
    """every iteration's error against the exact sum of the same float32 terms (see the module's docstring for the
    bound); asking for the error changes no bit of x and y"""
    from som_lvq_pak_amd import engine as E
    rlens = LARGE_RLENS if noc > CENTRE_CHUNK else (1, 2, 3)
    rows, x0, y0, D, snap = replayed(noc, 3, rlens)
    cb = E.Codebook(eng, rows)
    plain = E.sammon(cb, x0, y0, 3)
    x, y, err = E.sammon(cb, x0, y0, 3, want_error=True)
    cb.close()
    assert same_bits(x, plain[0]) and same_bits(y, plain[1])
    assert same_bits(x, snap[3][0]) and same_bits(y, snap[3][1])
    assert err.shape == (3,) and err.dtype == np.float64
    pairs = noc * (noc - 1) // 2
    bound = (2 * (pairs - 1) + 1) * 2.0 ** -53
    worst = 0.0
    for it in sorted(k for k in snap if k >= 1):        # (the large replays keep no snapshot of the second sweep)
        want = exact_error(snap[it][0], snap[it][1], D)
        assert want > 0
        worst = max(worst, abs(float(err[it - 1]) - want) / want / bound)
    print("mapping error, noc %d: %d pairs, bound %.3e relative, largest observed fraction of it %.3e" % (noc, pairs, bound, worst))
    assert worst <= 1.0
