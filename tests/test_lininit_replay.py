"""tests/lininit_replay.py against the LIVE reference, on the CPU: its in-order fp32 reading of lininit's two data passes
and its port of the iteration give the bits of the reference's own find_eigenvectors (oracle/_ref/libref_harness.so
over the unmodified som_rout.o) at every shape of the GPU edge tests -- in memory, not through "%g".  Skipped where
oracle/_ref is not built.  Also here, and needing no reference: the replay stays inside its float64 bounds, and the
inputs discriminate an in-order fp32 chain from a sum formed any more accurately."""
import hashlib
import json
import os

import numpy as np
import pytest

import lininit_replay as R
from conftest import GOLDEN

EDGES = json.load(open(os.path.join(GOLDEN, "cli", "expected.json")))["som"]["lininit_edges"]

CASES = [(d, n, m) for d, n in R.SHAPES for m in (False, True)]
IDS = ["%dx%d%s" % (d, n, "_masked" if m else "") for d, n, m in CASES]


@pytest.fixture(scope="module")
def ref_eig(ref):
    """the live reference with the find_eigenvectors entry of oracle/ref_harness.c; a prebuilt oracle/_ref from before
    that entry, where the reference's sources are not there to rebuild it, is as good as none for these tests"""
    if not ref.has_find_eigenvectors:
        pytest.skip("oracle/_ref/libref_harness.so predates ref_find_eigenvectors and cannot be rebuilt here")
    return ref


def same_bits_nan_aware(a, b):
    """equal bit patterns, except that a NaN only has to meet a NaN: which sign and payload 0 / 0 or inf * 0 gets is
    the compiler's and the processor's business (constant folding gives +NaN, SSE gives -NaN), not the reference's"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(R.bits(a)[~nan], R.bits(b)[~nan])


@pytest.mark.parametrize("dim,rows,masked", CASES, ids=IDS)
def test_replay_equals_the_reference_in_memory(ref_eig, dim, rows, masked):
    """mean and both axes from the replay's own sums and its own R == find_eigenvectors of the reference, two seeds"""
    c = R.replayed(dim, rows, masked)
    for seed in (11, 4242):
        want = ref_eig.find_eigenvectors(c["x"], seed, mask=c["mask"])
        got = R.eigenvectors(c["s"], c["cnt"], c["R"], rows, seed)
        assert want is not None and got is not None
        assert same_bits_nan_aware(got[0], want[0]), "mean"
        assert same_bits_nan_aware(got[1:], want[1:]), "axes"
    if dim >= 15 and not (masked and (dim, rows) == (33, 130)):
        assert np.isfinite(want).all()              # the comparison above was one of numbers


def test_reference_gives_up_like_the_replay(ref_eig):
    """fewer than three rows: NULL from the reference (som_rout.c:256), None from the replay"""
    x = R.case(17, 65, False)["x"][:2]
    assert ref_eig.find_eigenvectors(x, 5) is None and R.find_eigenvectors(x, None, 5) is None
    assert R.lininit_codes(x, None, 4, 3, 5) is None


def test_plane_of_codes_uses_the_axes_as_the_reference_does():
    """lininit_codes = mean + xf * axis1 + yf * axis2 in float with double xf, yf (som_rout.c:413-418): the corners of
    the map are mean -+ 2 axis1 -+ 2 axis2, and the whole function runs from data to codes"""
    c = R.replayed(17, 65, True)
    eig = R.find_eigenvectors(c["x"], c["mask"], 9)
    codes = R.lininit_codes(c["x"], c["mask"], 5, 3, 9)
    assert codes.shape == (15, 17) and codes.dtype == np.float32
    two = np.float32(2.0)
    assert np.array_equal(R.bits(codes[0]), R.bits((eig[0] + -two * eig[1]) + -two * eig[2]))
    assert np.array_equal(R.bits(codes[14]), R.bits((eig[0] + two * eig[1]) + two * eig[2]))
    assert np.array_equal(R.bits(codes[7]), R.bits((eig[0] + np.float32(0.0) * eig[1]) + np.float32(0.0) * eig[2]))


@pytest.mark.parametrize("dim,rows,masked", CASES, ids=IDS)
def test_replay_stays_inside_the_float64_bounds(dim, rows, masked):
    c = R.replayed(dim, rows, masked)
    for x, s in ((c["x"], c["s"]), (c["xs"], c["ss"])):
        s64, bound = R.column_sums64(x, c["mask"])
        assert (np.abs(s.astype(np.float64) - s64) <= bound).all()
    iu = np.triu_indices(dim)
    for mean, r32 in ((c["mean"], c["R"]), (np.zeros(dim, dtype=np.float32), c["R0"])):
        r64, bound = R.centered_products64(c["x"], c["mask"], mean)
        assert (np.abs(r32.astype(np.float64) - r64)[iu] <= bound[iu]).all()


@pytest.mark.parametrize("dim,rows,masked", [k for k in CASES if k[1] >= 63], ids=[i for i, k in zip(IDS, CASES) if k[1] >= 63])
def test_inputs_tell_an_in_order_chain_from_a_better_sum(dim, rows, masked):
    """at least half of the upper-triangle elements of R, and half of the column sums of the scaled rows, differ from
    the correctly rounded float64 result: a re-associated or fused sum cannot pass the bit tests by luck"""
    c = R.replayed(dim, rows, masked)
    iu = np.triu_indices(dim)
    r64, _ = R.centered_products64(c["x"], c["mask"], c["mean"])
    frac_r = float((R.bits(c["R"])[iu] != R.bits(r64.astype(np.float32))[iu]).mean())
    s64, _ = R.column_sums64(c["xs"], c["mask"])
    frac_s = float((R.bits(c["ss"]) != R.bits(s64.astype(np.float32))).mean())
    print("dim %d rows %d masked %d: R differs in %.3f, sums in %.3f" % (dim, rows, masked, frac_r, frac_s))
    assert frac_r >= 0.5 and frac_s >= 0.5


@pytest.mark.parametrize("tag", sorted(EDGES["data"]))
def test_replayed_codes_give_the_bytes_the_reference_wrote(tag):
    """the whole of lininit_codes in the replay, from the regenerated data to the "%g" text: the md5 the real
    reference's lininit left for the same data and command line (both topologies, two seeds)"""
    ex = EDGES["data"][tag]
    x, mask = R.rows_of(ex)
    assert (tag.startswith("masked")) == (mask is not None and mask.any())
    for run in ex["runs"]:
        a = dict(zip(run["args"][0::2], run["args"][1::2]))
        codes = R.lininit_codes(x, mask, int(a["-xdim"]), int(a["-ydim"]), int(a["-rand"]))
        assert hashlib.md5(R.cod_text(codes, run["args"])).hexdigest() == run["md5"], run["args"]


def test_recorded_edge_runs_are_the_ones_asked_for():
    assert sorted(EDGES["data"]) == sorted(["gen_%dx%d" % c for c in R.GEN_CASES] + ["masked_%dx%d" % c for c in R.TEXT_CASES])
    for ex in EDGES["data"].values():
        assert {r["args"][5] for r in ex["runs"]} == {"hexa", "rect"} and len({r["args"][9] for r in ex["runs"]}) == 2
    for tool in ("lininit", "mapinit"):
        two = EDGES["two_rows"][tool]
        assert two["returncode"] == 1 and not two["wrote_file"] and "lininit_codes: Can't find eigenvectors" in two["stderr_lines"]
