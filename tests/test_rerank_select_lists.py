"""The selection of the exact re-rank's (sample, row) pairs by its two kernels (somhip_debug_rerank_pairs):
k_rerank_select_lists, which walks level 2's lists, against k_rerank_select, which reads the whole matrix of group
minima, and both against a numpy replay of the rule on the arrays the search itself read:

    pairs = the rows of wmask[g, b] for every (g, b) with wmin[g, b] <= gmin[b] + tau[b], padding rows removed,
    bit 32 h + 16 i + r of a mask being row 64 g + 32 i + (r & 3) + 8 (r >> 2) + 4 h  (k_rerank_select).

A pair outside level 2's lists cannot pass that rule, so the two kernels must give the SAME set,
the same per-column counters, the same overflow word and the same statistics; the order inside a column's segment is
free.  The keys behind either selection are the oracle's.  Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

from test_scan_routes import TOPOL_HEXA, Case, decode, make_codebook, make_data, oracle_winners

pytestmark = pytest.mark.gpu

CAP_COL = 16384                                         # pairs per 32-sample column (pf_rerank)
TWO = ("two_level", 1, False, False, False)
RING = ("two_level", 1, True, False, False)

CASES = [
    Case("rows64", 64, 32, 256, TWO, cls="dups"),                                   # one group
    Case("rows65", 65, 32, 256, TWO, cls="dups"),                                   # ragged last group, row order
    Case("som13x9", 117, 32, 256, TWO, som=(13, 9, TOPOL_HEXA), cls="zeros"),       # ... of a map, zero samples
    Case("som64x64", 4096, 64, 3841, RING, som=(64, 64, TOPOL_HEXA), cls="dups"),   # patch order, ring kernel
    Case("count65504_wrap", 512, 32, 65504, TWO, wrap=True, ndata=70001),           # last 16-bit sample index
] + [Case("two_%s" % cls, 1024, 32, 256, TWO, cls=cls) for cls in ("dups", "tiny", "huge", "allinf", "nan", "zeros")] + [
    Case("same448", 448, 32, 256, TWO, cls="same"),     # every group listed for every sample: 14336 pairs a column
    Case("same576", 576, 32, 256, TWO, cls="same"),     # 18432 > 16384: the segments overflow, k_rerank decides
]


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    e.set_scan_mode("mfma_bf16")
    yield e
    e.close()


def data_of(c):
    if c.cls != "same":
        return make_data(c)
    rs = np.random.RandomState(c.n)
    v = rs.standard_normal(c.d).astype(np.float32)
    codes = np.tile(v, (c.n, 1))
    x = (v + 0.1 * rs.standard_normal((c.ndata, c.d))).astype(np.float32)
    return codes, x, None


def ordered_to_float(u):
    u = u.astype(np.uint32)
    return np.where(u & 0x80000000, u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(np.float32)


# bit t = 32 h + 16 i + r of a mask -> row of the group
BIT_ROW = np.array([32 * ((t >> 4) & 1) + ((t & 15) & 3) + 8 * ((t & 15) >> 2) + 4 * (t >> 5) for t in range(64)])


def replay(out, n, count):
    """(sorted pair keys sample << 32 | row, colcount [4, ncols]) of the rule on the arrays the selection read"""
    ncols = out["wmin"].shape[1] // 32
    with np.errstate(invalid="ignore", over="ignore"):
        thr = ordered_to_float(out["gmin"][:count]) + out["tau"]
        g, b = np.nonzero(out["wmin"][:, :count] <= thr[None, :])
    bits = ((out["wmask"][g, b][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    rows = g[:, None] * 64 + BIT_ROW[None, :]
    keep = bits & (rows < n)                            # padding rows of a ragged last group removed
    e, t = np.nonzero(keep)
    pair_keys = np.sort((b[e].astype(np.uint64) << np.uint64(32)) | rows[e, t].astype(np.uint64))
    per = keep.sum(axis=1)
    b, per = b[per > 0], per[per > 0]                   # a group without a row left is not counted
    cc = np.zeros((4, ncols), dtype=np.uint32)
    np.add.at(cc[0], b // 32, per)
    np.add.at(cc[1], b // 32, 1)
    np.add.at(cc[2], b // 32, per)
    cc[3] = np.bincount(b, minlength=32 * ncols).reshape(ncols, 32).max(axis=1)
    return pair_keys, cc


def search(E, eng, cb, ds, c, from_lists):
    before = eng.scan_stats()
    out = E.debug_rerank_pairs(cb, ds, c.first, c.count, from_lists)
    after = eng.scan_stats()
    out["delta"] = {k: after[k] - before[k] for k in ("groups", "rows", "samples")}
    out["max"] = after["max_groups_per_sample"]
    return out


def check_selection(out, c, n):
    want_keys, want_cc = replay(out, n, c.count)
    assert np.array_equal(out["colcount"], want_cc), ("counters differ from the replay in columns",
                                                      np.unique(np.nonzero(out["colcount"] != want_cc)[1])[:8])
    cap = (out["wmin"].shape[1] // 32) * CAP_COL
    overflowed = bool((want_cc[0] > CAP_COL).any())
    assert (out["overflow"] > cap) == overflowed
    if not overflowed:
        got = np.sort((out["pairs"][:, 0].astype(np.uint64) << np.uint64(32)) | out["pairs"][:, 1].astype(np.uint64))
        assert got.size == want_keys.size and np.array_equal(got, want_keys)
    return overflowed


def check_keys(oracle, out, codes, x, c):
    win = (c.first + np.arange(c.count)) % c.ndata
    idx, diff = decode(out["keys"].reshape(-1, 1), False)
    widx, wdiff, _ = oracle_winners(oracle, codes, x[win], 1, False)
    wdiff = np.where(widx == -1, np.float32(-1.0), wdiff)
    bad = np.nonzero((idx != widx).any(axis=1) | (diff.view(np.uint32) != wdiff.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%d of %d samples differ from the oracle; first at %d" % (bad.size, c.count, bad[0])


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_both_selectors_give_the_replayed_pairs(eng, oracle, c):
    from som_lvq_pak_amd import engine as E
    codes, x, _ = data_of(c)
    cb, ds = make_codebook(E, eng, c, codes), E.Dataset(eng, x)
    try:
        plan = E.scan_plan(cb, ds, c.count, 1)
        assert (plan["route"], plan["kth"], plan["l1_ring"], plan["by_group"], plan["l2_global"]) == c.plan
        dense = search(E, eng, cb, ds, c, False)
        lists = search(E, eng, cb, ds, c, True)
    finally:
        cb.close()
        ds.close()
    # the pre-filter is the same computation in both runs: the selections read the same arrays
    for k in ("gmin", "tau"):
        assert np.array_equal(dense[k].view(np.uint32), lists[k].view(np.uint32)), k
    overflowed = check_selection(dense, c, c.n)
    assert check_selection(lists, c, c.n) == overflowed
    if c.cls == "same":                                 # (allinf overflows too: every row passes for every sample)
        assert overflowed == (c.n == 576)
    assert np.array_equal(dense["colcount"], lists["colcount"]) and dense["overflow"] == lists["overflow"]
    assert dense["delta"] == lists["delta"] and dense["delta"]["samples"] == c.count
    assert lists["max"] == dense["max"]                 # (a maximum since the engine's creation: the second run adds nothing)
    if c.name == "same448":
        assert (dense["colcount"][0] == 32 * 448).all()
    assert np.array_equal(dense["keys"], lists["keys"])
    check_keys(oracle, lists, codes, x, c)


def test_a_shorter_search_after_a_longer_one(eng, oracle):
    """stale lists, counts and counters of the longer search lie in scratch beyond what the shorter one writes"""
    from som_lvq_pak_amd import engine as E
    long_c = Case("long", 1024, 32, 1000, TWO, cls="dups")
    short_c = Case("short", 1024, 32, 225, TWO, cls="dups", ndata=long_c.ndata)
    codes, x, _ = make_data(long_c)
    cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
    try:
        search(E, eng, cb, ds, long_c, True)
        lists = search(E, eng, cb, ds, short_c, True)
        dense = search(E, eng, cb, ds, short_c, False)
    finally:
        cb.close()
        ds.close()
    assert not check_selection(lists, short_c, 1024) and not check_selection(dense, short_c, 1024)
    assert np.array_equal(dense["colcount"], lists["colcount"]) and dense["delta"] == lists["delta"]
    check_keys(oracle, lists, codes, x, short_c)


def test_lists_need_two_levels(eng):
    from som_lvq_pak_amd import _lib, engine as E
    rs = np.random.RandomState(5)
    cb, ds = E.Codebook(eng, rs.standard_normal((1024, 32)).astype(np.float32)), E.Dataset(eng, rs.standard_normal((200, 32)).astype(np.float32))
    try:
        with pytest.raises(_lib.SomhipError, match="no level-2 lists"):
            E.debug_rerank_pairs(cb, ds, 0, 200, True)
        assert E.debug_rerank_pairs(cb, ds, 0, 200, False)["pairs"].shape[0] >= 200
    finally:
        cb.close()
        ds.close()
