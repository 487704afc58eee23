"""The winner search of a row-sharded codebook with the pre-filter's bounds exchanged between the shards
(somhip_shard_winner_begin / _refine / _finish), on every plan scan_plan can give such a search.

Only one GPU is visible where this suite runs, so the shards live on several engines of one process (a search owns its
engine's scratch) and the collectives are numpy: MIN of the bounds after begin and after refine, MIN of the keys after
finish.  Every case asserts the plan of every shard (somhip_debug_scan_plan) and the kernels that ran, the merged keys
against the CPU oracle's find_winner_euc over the whole codebook and against the MIN of the shards' plain searches, and the
invariant include/somhip.h states for the exchange -- a bound may only remove rows that cannot win -- in float64:
with s = ||c||^2 - 2 <x, c> and s* its minimum over all rows of all shards, both reduced bounds are >= s* - eps, where
eps = (d + 2) 2^-52 (||x|| + max ||c||)^2 is the float64 evaluation's own error and nothing more.  A case with a far shard
(its rows 40 per component away) also asserts that the exchange is not vacuous: that shard abstains for every sample.
test_every_exchange_plan_has_a_case keeps the table complete.  Needs an MI355X:  pytest -m gpu."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_scan_routes import check_kernels, decode, make_data, oracle_winners

pytestmark = pytest.mark.gpu

NONE = np.uint64(0x7FFFFFFFFFFFFFFF)          # "no winner in this shard" (include/somhip.h)
TWO, TWO_RING, TWO_LG, TWO_RING_LG = ("two_level", False, False), ("two_level", True, False), \
    ("two_level", False, True), ("two_level", True, True)
ONE, DIRECT = ("one_level", False, False), ("direct", False, False)
CLASSES = ("dups", "hits", "ulp", "offset", "tiny", "huge", "allinf", "nan")


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    """rows: the shards' row counts (contiguous shards of one codebook, in order); expect: per shard (route, l1_ring,
    l2_global) as scan_plan gives it for want 1 -- a shard that is not two_level is not available for the exchange;
    far: the shard whose rows lie 40 per component away; fused: False runs under SOMHIP_NO_FUSED_GMIN=1;
    reduce: the host's MIN of the bounds; som = (xdim, ydim): interleaved shards of a map instead of row shards.
    data: the name the data are seeded from -- variants of one case (fused or not, the host's MIN) share them."""

    def __init__(self, name, rows, d, count, expect, cls="mix", far=None, wrap=False, fused=True, reduce="minimum",
                 som=None, data=None):
        self.name, self.rows, self.d, self.count, self.expect = name, tuple(rows), d, count, tuple(expect)
        self.cls, self.far, self.fused, self.reduce, self.som = cls, far, fused, reduce, som
        self.n = sum(rows)
        self.cuts = [0] + list(np.cumsum(rows))
        self.ndata = count + 7
        self.first = self.ndata - 7 if wrap else 0
        self.data = data or name
        assert len(self.expect) == len(self.rows) <= 4 and (far is None or cls == "mix")

    def groups(self, s):
        return -(-self.rows[s] // 64)

    def variant(self, s):
        """(l1_ring, l1_wide, l2_global, fused) of shard s: l1_wide as scan_plan forms it, ngroups >= 512 or the ring"""
        _, ring, lg = self.expect[s]
        return (ring, ring or self.groups(s) >= 512, lg, self.fused)


class DataKey:
    """what make_data of test_scan_routes reads of a case"""

    def __init__(self, c):
        self.name, self.n, self.d, self.count, self.ndata, self.first, self.cls = c.data, c.n, c.d, c.count, c.ndata, c.first, c.cls


def _cases():
    cs = []

    def add(name, *a, **k):
        cs.append(Case(name, *a, **k))

    # level 1 narrow, level 2 from LDS; the run length's limits (nsb >= 8, bpad <= 65535) and a window that wraps
    for count in (225, 256, 65504):
        add("narrow_lds_%d" % count, (512, 512, 64), 32, count, (TWO, TWO, TWO), far=1)
    add("narrow_lds_300_wrap", (512, 512, 64), 32, 300, (TWO, TWO, TWO), far=1, wrap=True)
    add("no_fused_narrow_lds", (512, 512, 64), 32, 256, (TWO, TWO, TWO), far=1, fused=False, data="narrow_lds_256")
    for count in (224, 65505):
        add("count_edges_%d" % count, (512, 512), 32, count, (ONE, ONE))
    # rows: 64 is the pre-filter's least; the 63-row shard scans directly and joins by its plain keys
    add("rows64_65", (64, 65, 63), 32, 256, (TWO, TWO, DIRECT), cls="dups")
    # dimension: ceil(ceil(d / 4) / 2) % 4 == 0
    for d in (25, 31, 32, 57, 512):
        add("dims_%d" % d, (1024, 1024), d, 256, (TWO, TWO), far=1)
    for d in (24, 33, 56, 65, 513):
        add("dims_unavailable_%d" % d, (1024, 1024), d, 256, (ONE, ONE))
    # level 1 as the ring kernel by tiles: ceil(nsb / 8) * ceil(ngroups / 4) >= 256
    add("ring_tiles", (4096, 4096), 64, 3841, (TWO_RING, TWO_RING), far=1)
    add("no_fused_ring_tiles", (4096, 4096), 64, 3841, (TWO_RING, TWO_RING), far=1, fused=False, data="ring_tiles")
    add("ring_tiles_3840", (4096, 4096), 64, 3840, (TWO, TWO), far=1)
    # 512 groups: the wide tile without the ring (d8 % 8 != 0), the ring by groups beside a narrow shard
    add("wide_no_ring", (32768, 4096), 32, 256, (TWO, TWO), far=1)
    add("no_fused_wide_no_ring", (32768, 4096), 32, 256, (TWO, TWO), far=1, fused=False, data="wide_no_ring")
    add("ring_groups", (32768, 600), 64, 256, (TWO_RING, TWO), far=1)
    add("ring_groups_far_ring", (32768, 600), 64, 256, (TWO_RING, TWO), far=0)
    # level 2's sample operand from global memory (d8 > 64), under each form of level 1
    add("l2_global", (1024, 1024), 544, 256, (TWO_LG, TWO_LG), far=1)
    add("no_fused_l2_global", (1024, 1024), 544, 256, (TWO_LG, TWO_LG), far=1, fused=False, data="l2_global")
    add("wide_l2_global", (32768, 1024), 544, 256, (TWO_LG, TWO_LG), far=1)
    add("no_fused_wide_l2_global", (32768, 1024), 544, 256, (TWO_LG, TWO_LG), far=1, fused=False, data="wide_l2_global")
    add("ring_l2_global", (32768, 1024), 1024, 256, (TWO_RING_LG, TWO_LG), far=1)       # (the 32768-row form was used)
    add("no_fused_ring_l2_global", (32768, 1024), 1024, 256, (TWO_RING_LG, TWO_LG), far=1, fused=False, data="ring_l2_global")
    # a map over three interleaved shards (8 x 8 patches dealt round-robin): five patches, 320 rows, each
    add("interleaved", (320, 320, 320), 32, 256, (TWO, TWO, TWO), som=(24, 40))
    add("interleaved_hits", (320, 320, 320), 32, 256, (TWO, TWO, TWO), som=(24, 40), cls="hits")
    # the adversarial data classes, narrow and ring; NaN under both readings of the host's MIN
    for cls in CLASSES:
        add("narrow_lds_%s" % cls, (512, 512, 64), 32, 256, (TWO, TWO, TWO), cls=cls)
        add("ring_tiles_%s" % cls, (4096, 4096), 64, 3841, (TWO_RING, TWO_RING), cls=cls)
    add("narrow_lds_nan_fmin", (512, 512, 64), 32, 256, (TWO, TWO, TWO), cls="nan", reduce="fmin", data="narrow_lds_nan")
    add("ring_tiles_nan_fmin", (4096, 4096), 64, 3841, (TWO_RING, TWO_RING), cls="nan", reduce="fmin", data="ring_tiles_nan")
    return sorted(cs, key=lambda c: c.data)        # (stable: the variants of one case follow it and share its reference)


CASES = _cases()


# ------------------------------------------------------------------------------------------------ data and references
def build_data(c):
    """(codes [n, d] in global row order, data [ndata, d]): make_data's classes; for dups / hits also a pair of equal
    rows on either side of every shard cut with a sample on it (make_data itself puts the same row first and last: into
    the first and the last shard, distance 0 to both for hits); a far shard's rows are the near rows plus 40"""
    codes, x, _ = make_data(DataKey(c))
    if c.cls in ("dups", "hits"):
        rs = np.random.RandomState(zlib.crc32(c.data.encode()) ^ 0x5EED)
        win = (c.first + np.arange(c.count)) % c.ndata
        for i, cut in enumerate(c.cuts[1:-1]):
            codes[cut] = codes[cut - 1]
            x[win[40 + 3 * i]] = codes[cut] if c.cls == "hits" else codes[cut] + 0.01 * rs.standard_normal(c.d).astype(np.float32)
    if c.far is not None:
        a, b = c.cuts[c.far], c.cuts[c.far + 1]
        codes[a:b] = codes[a:b] + np.float32(40.0)
    return np.ascontiguousarray(codes, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)


def smallest_s(codes, xs):
    """float64: (s* [m] = min over the rows of ||c||^2 - 2 <x, c>, eps [m] = (d + 2) 2^-52 (||x|| + max ||c||)^2)"""
    m, d = xs.shape
    sstar = np.full(m, np.inf)
    cmax = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(0, codes.shape[0], 4096):
            cd = codes[r:r + 4096].astype(np.float64)
            cn = (cd * cd).sum(axis=1)
            cmax = max(cmax, float(np.sqrt(cn.max())))
            for s in range(0, m, 4096):
                xd = xs[s:s + 4096].astype(np.float64)
                sstar[s:s + 4096] = np.minimum(sstar[s:s + 4096], (cn[None, :] - 2.0 * (xd @ cd.T)).min(axis=1))
        xn = np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1))
        eps = (d + 2) * 2.0 ** -52 * (xn + cmax) ** 2
    return sstar, eps


_REF = {}


def reference(c, oracle):
    """codes, data, the window's samples, the oracle's winners over the whole codebook and s* over the shards that take
    part in the exchange; made once per data name and left unchanged (the last one is kept)"""
    if c.data not in _REF:
        _REF.clear()
        codes, x = build_data(c)
        xs = x[(c.first + np.arange(c.count)) % c.ndata]
        widx, wdiff, _ = oracle_winners(oracle, codes, xs, 1, False)
        wdiff = np.where(widx == -1, np.float32(-1.0), wdiff)         # the ABI's "nothing beat FLT_MAX" (decode_key)
        part = np.concatenate([np.arange(c.cuts[s], c.cuts[s + 1]) for s in range(len(c.rows)) if c.expect[s][0] == "two_level"] or
                              [np.arange(0)])
        sstar, eps = smallest_s(codes[part], xs) if part.size and c.cls not in ("nan", "allinf") else (None, None)
        for a in (codes, x, xs, widx, wdiff):
            a.setflags(write=False)
        _REF[c.data] = {"codes": codes, "x": x, "xs": xs, "widx": widx[:, 0], "wdiff": wdiff[:, 0], "sstar": sstar, "eps": eps}
    return _REF[c.data]


# ------------------------------------------------------------------------------------------------ the engine side
@pytest.fixture(scope="module")
def engines():
    from som_lvq_pak_amd import engine as E
    engs = [E.Engine(0) for _ in range(4)]
    for e in engs:
        e.timing(True)
        e.set_scan_mode("mfma_bf16")
    yield engs
    _REF.clear()
    for e in engs:
        e.close()


def make_shards(E, c, engs, codes):
    """the case's shards, shard s on engs[s]"""
    if c.som:
        xdim, ydim = c.som
        S = len(c.rows)
        units = [E.shard_units(xdim, ydim, r, S) for r in range(S)]
        assert [u.size for u in units] == list(c.rows)
        return [E.Codebook(engs[r], codes[units[r]], E.TOPOL_HEXA, E.NEIGH_BUBBLE, xdim, ydim, interleave=(r, S)) for r in range(S)]
    return [E.Codebook(engs[s], codes[a:b], row_offset=a, n_global=c.n) for s, (a, b) in enumerate(zip(c.cuts, c.cuts[1:]))]


def to_host(e, dev, count, dtype):
    out = np.empty(count, dtype=dtype)
    assert e.lib.somhip_copy_to_host(e.h, out.ctypes.data_as(C.c_void_p), dev, out.nbytes) == 0, e.lib.somhip_last_error()
    return out


def exchange_search(engs, shards, dss, first, count, reduce=np.minimum):
    """begin -> MIN of the bounds on the host -> refine -> MIN -> finish -> MIN of the keys, shard s on engs[s].  Returns
    (merged keys, every shard's own keys, b1, b2, every shard's own bounds after begin, ... after refine)."""
    S = len(shards)
    kb = [e.device_alloc(8 * count) for e in engs]
    bb = [e.device_alloc(4 * count) for e in engs]

    def exchange_bounds():
        own = [to_host(e, b, count, np.float32) for e, b in zip(engs, bb)]
        with np.errstate(invalid="ignore"):
            m = np.ascontiguousarray(reduce.reduce(own))
        for e, b in zip(engs, bb):
            assert e.lib.somhip_copy_to_device(e.h, b, m.ctypes.data_as(C.c_void_p), 4 * count) == 0
        return m, own

    try:
        for s in range(S):
            assert engs[s].lib.somhip_shard_winner_begin(shards[s].h, dss[s].h, first, count, kb[s], bb[s]) == 0, engs[s].lib.somhip_last_error()
        b1, own1 = exchange_bounds()
        for s in range(S):
            assert engs[s].lib.somhip_shard_winner_refine(shards[s].h, dss[s].h, first, count, bb[s]) == 0, engs[s].lib.somhip_last_error()
        b2, own2 = exchange_bounds()
        for s in range(S):
            assert engs[s].lib.somhip_shard_winner_finish(shards[s].h, dss[s].h, first, count, bb[s], kb[s]) == 0, engs[s].lib.somhip_last_error()
        own = [to_host(e, k, count, np.uint64) for e, k in zip(engs, kb)]
    finally:
        for e, k, b in zip(engs, kb, bb):
            e.device_free(k)
            e.device_free(b)
    return np.minimum.reduce(own), own, b1, b2, own1, own2


def plain_search(e, cb, ds, first, count):
    kb = e.device_alloc(8 * count)
    try:
        assert e.lib.somhip_batch_winner_keys(cb.h, ds.h, first, count, kb) == 0, e.lib.somhip_last_error()
        return to_host(e, kb, count, np.uint64)
    finally:
        e.device_free(kb)


class Want1:
    knn = 1                                   # (what check_kernels reads of a case)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_exchanged_search(engines, oracle, monkeypatch, c):
    from som_lvq_pak_amd import engine as E
    if not c.fused:
        monkeypatch.setenv("SOMHIP_NO_FUSED_GMIN", "1")       # read by the library at every call
    ref = reference(c, oracle)
    S = len(c.rows)
    engs = engines[:S]
    shards = make_shards(E, c, engs, ref["codes"])
    dss = [E.Dataset(e, ref["x"]) for e in engs]
    try:
        # the plan of every shard, and who takes part
        plans = [E.scan_plan(cb, ds, c.count, 1) for cb, ds in zip(shards, dss)]
        for s, plan in enumerate(plans):
            assert (plan["route"], plan["l1_ring"], plan["l2_global"]) == c.expect[s], (s, plan)
            two = plan["route"] == "two_level"
            assert plan["bf16"] and plan["fused_gmin"] == (two and c.fused), (s, plan)
            lib = engs[s].lib
            assert lib.somhip_shard_exchange_available(shards[s].h, dss[s].h, c.count) == int(two)
            if not two:
                kb, bb = engs[s].device_alloc(8 * c.count), engs[s].device_alloc(4 * c.count)
                try:
                    assert lib.somhip_shard_winner_begin(shards[s].h, dss[s].h, c.first, c.count, kb, bb) != 0
                    assert b"not available" in lib.somhip_last_error()
                finally:
                    engs[s].device_free(kb)
                    engs[s].device_free(bb)
        live = [s for s in range(S) if plans[s]["route"] == "two_level"]
        if not live:
            return
        pick = lambda seq: [seq[s] for s in live]
        rows0 = [e.scan_stats()["rows"] for e in engs]
        for e in engs:
            e.timing_reset()
        merged, own, b1, b2, own1, own2 = exchange_search(pick(engs), pick(shards), pick(dss), c.first, c.count,
                                                          np.fmin if c.reduce == "fmin" else np.minimum)
        for s in live:                                         # second witness: the kernels that ran
            table = engs[s].timing_table()
            check_kernels(Want1, plans[s], table)
            assert table["k_dist_l2"][0] > 0 and table["k_l2_select"][0] > 0 and table["k_scan_exact"][0] == 0
        rows1 = [e.scan_stats()["rows"] for e in engs]
        plain = [plain_search(e, cb, ds, c.first, c.count) for e, cb, ds in zip(engs, shards, dss)]
        rows2 = [e.scan_stats()["rows"] for e in engs]
    finally:
        for o in shards + dss:
            o.close()
    for s in range(S):                                         # a shard that cannot take part joins by its plain keys
        if s not in live:
            merged = np.minimum(merged, plain[s])

    # keys against the oracle: index (on ties the lowest global index) and distance bits
    idx, diff = decode(merged, False)
    bad = np.nonzero((idx != ref["widx"]) | (diff.view(np.uint32) != ref["wdiff"].view(np.uint32)))[0]
    assert bad.size == 0, "%d of %d samples differ; first at %d: got %d %r (key %#x), oracle %d %r" % (
        bad.size, c.count, bad[0], idx[bad[0]], diff[bad[0]], int(merged[bad[0]]), ref["widx"][bad[0]], ref["wdiff"][bad[0]])
    none = ref["widx"] == -1
    assert (merged[none] == NONE).all(), "a sample nothing beats: key %#x" % int(merged[none][merged[none] != NONE][0])
    if c.cls == "hits":
        assert idx[0] == 0 and diff[0] == 0.0               # rows 0 and n - 1 are the sample: the first shard's wins
        assert none.sum() == 0
    if c.cls in ("nan", "allinf"):
        assert none.any()
    # keys against the plain searches
    assert np.array_equal(merged, np.minimum.reduce(plain))

    # the bounds: never NaN, safe in float64, and the refined one the tighter
    for s, (o1, o2) in enumerate(zip(own1, own2)):
        assert not np.isnan(o1).any() and not np.isnan(o2).any(), "shard %d: a bound is NaN" % live[s]
    if ref["sstar"] is not None:
        for name, b, owns in (("begin", b1, own1), ("refine", b2, own2)):
            low = np.nonzero(b.astype(np.float64) < ref["sstar"] - ref["eps"])[0]
            assert low.size == 0, "%d bounds after %s below s*: sample %d, shard %d, bound %r, s* %r, eps %r" % (
                low.size, name, low[0], live[int(np.argmin([o[low[0]] for o in owns]))], float(b[low[0]]),
                ref["sstar"][low[0]], ref["eps"][low[0]])
    late = np.nonzero(~(b2 <= b1))[0]
    assert late.size == 0, "%d refined bounds above the first: sample %d, %r > %r" % (late.size, late[0], b2[late[0]], b1[late[0]])

    # not vacuous: a far shard abstains for every sample, though on its own it names its best row
    if c.far is not None:
        assert (own[live.index(c.far)] == NONE).all()
        assert (plain[c.far] != NONE).all()
    # k_rerank_pairs (the pair lists' fills) and k_rerank (its own masks) both count the rows they re-rank into
    # scan_stats()["rows"]: with the bounds exchanged the shards together re-rank no more than on their own
    if c.cls == "mix":
        exchanged = sum(rows1[s] - rows0[s] for s in live)
        alone = sum(rows2[s] - rows1[s] for s in live)
        assert 0 < exchanged <= alone, (exchanged, alone)


# ------------------------------------------------------------------------------------------------ completeness
def test_every_exchange_plan_has_a_case(engines, monkeypatch):
    """The (l1_ring, l1_wide, l2_global, fused or not) of the table's shards are every combination scan_plan can give a
    nearest-row two-level search -- the ring implies the wide tile, nothing else is tied -- and a sweep of shapes through
    scan_plan gives no other."""
    from som_lvq_pak_amd import engine as E
    every = {(ring, wide, lg, fused) for ring in (False, True) for wide in (False, True) for lg in (False, True)
             for fused in (False, True) if wide or not ring}
    table = {c.variant(s) for c in CASES for s in range(len(c.rows)) if c.expect[s][0] == "two_level"}
    assert table == every, (every - table, table - every)
    seen = set()
    eng = engines[0]
    for n in (64, 4096, 32768):
        for d in (25, 32, 57, 64, 512, 544, 1024):
            cb = E.Codebook(eng, np.zeros((n, d), dtype=np.float32))
            ds = E.Dataset(eng, np.zeros((8, d), dtype=np.float32))
            for fused in (True, False):
                if fused:
                    monkeypatch.delenv("SOMHIP_NO_FUSED_GMIN", raising=False)
                else:
                    monkeypatch.setenv("SOMHIP_NO_FUSED_GMIN", "1")
                for count in (225, 256, 3840, 3841, 65504):
                    p = E.scan_plan(cb, ds, count, 1)
                    assert p["route"] == "two_level" and p["fused_gmin"] == fused, (n, d, count, p)
                    seen.add((p["l1_ring"], p["l1_ring"] or -(-n // 64) >= 512, p["l2_global"], p["fused_gmin"]))
            cb.close()
            ds.close()
    assert seen == every, (every - seen, seen - every)
