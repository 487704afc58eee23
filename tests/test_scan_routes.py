"""Every route of the winner search, at the thresholds that choose it, against the CPU oracle.

The route of a search is chosen in one place (scan_plan, host_scan.inc) from the run length, the codebook's rows and
groups and the dimension.  Each case below names the route it expects: the test asserts that plan
(somhip_debug_scan_plan) and, as a second witness, the kernels that ran (the timing table's launch counts), then
decodes the keys the way decode_key does and compares index and distance bits with the oracle
(find_winner_euc / find_winner_knn restated in C).  test_every_plan_has_a_case keeps the table complete: a plan
scan_plan can produce without a case here fails it.  Needs an MI355X:  pytest -m gpu."""
import ctypes as C
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu

FLT_MAX_BITS = 0x7F7FFFFF
TOPOL_HEXA, TOPOL_RECT = 3, 4
TIE_FIRST, TIE_KNN = 0, 1
WORKERS = max(1, min(16, os.cpu_count() or 1))


def width(knn):
    return 1 if knn == 1 else 2 if knn == 2 else 4 if knn <= 4 else 8


# ------------------------------------------------------------------------------------------------ the case table
# plan: (route, kth, l1_ring, by_group, l2_global) -- what somhip_debug_scan_plan reports
def P(route, kth=1, ring=False, bg=False, lg=False):
    return (route, kth, ring, bg, lg)


MASKED, DIRECT = P("masked"), P("direct")
ONE, ONE_BG, ONE_K8, ONE_K8_BG = P("one_level"), P("one_level", bg=True), P("one_level", 8), P("one_level", 8, bg=True)
TWO = P("two_level")

# every plan scan_plan can produce (no SOMHIP_* switch set)
ALL_PLANS = {MASKED, DIRECT, ONE, ONE_BG, ONE_K8, ONE_K8_BG} | \
    {P("two_level", 1, ring, False, lg) for ring in (False, True) for lg in (False, True)} | \
    {P("two_level", 8, ring, bg, lg) for ring in (False, True) for bg in (False, True) for lg in (False, True)}


class Case:
    def __init__(self, name, n, d, count, plan, entry="bwk", knn=1, tie=TIE_FIRST, mode="mfma_bf16", cls="mix",
                 som=None, first=0, wrap=False, ndata=None):
        self.name, self.n, self.d, self.count, self.plan = name, n, d, count, plan
        self.entry, self.knn, self.tie, self.mode, self.cls = entry, knn, tie, mode, cls
        self.som = som                      # None: row order (LVQ / k-NN); (xdim, ydim, topol): a SOM map
        self.ndata = ndata or count + 7
        self.first = self.ndata - 7 if wrap else first
        if som:
            assert som[0] * som[1] == n

    def __repr__(self):
        return self.name


def _cases():
    cs = []

    def add(name, *a, **k):
        cs.append(Case(name, *a, **k))

    # run length (want 1), n = 512 x 32: MFMA_MIN_SAMPLES, nsb >= 8, bpad <= 65535, the pre-filter's limit
    for count, plan in ((31, DIRECT), (32, ONE), (33, ONE), (224, ONE), (225, TWO), (65504, TWO), (65505, ONE),
                        (131072, ONE), (131073, DIRECT)):
        add("count%d" % count, 512, 32, count, plan)
    add("count65504_wrap", 512, 32, 65504, TWO, wrap=True, ndata=70001)
    add("count131073_wrap", 512, 32, 131073, DIRECT, wrap=True, ndata=140001)
    add("count65505_ulp", 512, 32, 65505, ONE, cls="ulp")
    add("count225_dups", 512, 32, 225, TWO, cls="dups")
    add("count32_hits", 512, 32, 32, ONE, cls="hits")
    add("count33_fw", 512, 32, 33, ONE, entry="fw")
    # level 1 as the ring kernel: by tiles (64 groups, d8 % 8 == 0)
    add("tiles3840", 4096, 64, 3840, TWO)
    add("tiles3841", 4096, 64, 3841, P("two_level", ring=True))
    add("tiles3841_wrap", 4096, 64, 3841, P("two_level", ring=True), wrap=True, ndata=5000)
    add("tiles3841_dups", 4096, 64, 3841, P("two_level", ring=True), cls="dups")
    add("tiles3841_fw_ulp", 4096, 64, 3841, P("two_level", ring=True), entry="fw", cls="ulp")
    # rows: the want-1 pre-filter (64), the top-k pre-filter (4096), 511 | 512 | 513 groups
    add("rows63", 63, 32, 256, DIRECT)
    add("rows64", 64, 32, 256, TWO, cls="dups")
    add("rows65", 65, 32, 256, TWO, cls="dups")
    add("rows4095_k4", 4095, 32, 256, DIRECT, entry="topk", knn=4, tie=TIE_KNN, cls="dups")
    add("rows4096_k4", 4096, 32, 256, ONE, entry="topk", knn=4, tie=TIE_KNN, cls="dups")
    add("rows4096_k2_first", 4096, 32, 256, ONE, entry="topk", knn=2, tie=TIE_FIRST, cls="dups")
    add("rows4096_k3_fw", 4096, 32, 256, ONE, entry="fw", knn=3, tie=TIE_KNN, cls="hits")
    add("rows32704_k8", 32704, 64, 256, ONE, entry="topk", knn=8, tie=TIE_KNN, cls="dups")
    add("rows32768_k8", 32768, 64, 256, P("two_level", 8, True, True), entry="topk", knn=8, tie=TIE_KNN, cls="dups")
    add("rows32769_k8", 32769, 64, 256, P("two_level", 8, True, True), entry="topk", knn=8, tie=TIE_KNN)
    add("rows32769_k8_first", 32769, 64, 256, P("two_level", 8, True, True), entry="topk", knn=8, tie=TIE_FIRST,
        cls="dups")
    add("rows32768_k5_fw", 32768, 64, 256, P("two_level", 8, True, True), entry="fw", knn=5, tie=TIE_KNN, cls="hits")
    add("rows32768_k4", 32768, 64, 256, ONE_BG, entry="topk", knn=4, tie=TIE_KNN, cls="dups")
    add("rows32768_k8_n224", 32768, 64, 224, ONE_K8_BG, entry="topk", knn=8, tie=TIE_KNN)
    add("rows32768_w1", 32768, 64, 256, P("two_level", ring=True), cls="dups")
    add("rows32768_w1_wrap", 32768, 64, 3841, P("two_level", ring=True), wrap=True, ndata=4000)
    # dimension (want 1, 1024 rows): d8 % 4 (two levels), d8 % 8 (ring), d8 <= 64 (level 2 in LDS)
    for d, plan in ((1, ONE), (3, ONE), (4, ONE), (5, ONE), (24, ONE), (25, TWO), (31, TWO), (32, TWO), (33, ONE),
                    (512, TWO), (513, ONE), (544, P("two_level", lg=True))):
        add("dim%d" % d, 1024, d, 256, plan, cls="ulp" if d in (25, 33) else "mix")
    add("dim3_offset", 1024, 3, 256, ONE, cls="offset")
    add("dim544_hits", 1024, 544, 256, P("two_level", lg=True), cls="hits")
    for d, plan in ((56, ONE), (57, P("two_level", ring=True)), (63, P("two_level", ring=True)),
                    (65, ONE), (32, TWO)):
        add("dim%d_tiles" % d, 4096, d, 3841, plan)
    # the top-8 two-level search at 512 groups: ring (d8 % 8), by group (d & 3, d4 <= 256), level 2 from global (d8 > 64)
    for d, plan in ((32, P("two_level", 8, False, True)), (31, P("two_level", 8, False, False)),
                    (61, P("two_level", 8, True, False)), (544, P("two_level", 8, False, True, True)),
                    (543, P("two_level", 8, False, False, True)), (1021, P("two_level", 8, True, False, True)),
                    (1024, P("two_level", 8, True, True, True)), (1025, ONE_K8), (1028, ONE_K8)):
        add("k8_dim%d" % d, 32768, d, 256, plan, entry="topk", knn=8, tie=TIE_KNN, cls="dups" if d in (31, 1021) else "mix")
    add("w1_dim1024", 32768, 1024, 256, P("two_level", ring=True, lg=True))
    # scan modes: fp32 MFMA (one level only; top-k then scans directly) and the direct scan
    add("mfma_d32", 1024, 32, 256, ONE, mode="mfma", cls="ulp")
    add("mfma_d33_dups", 1024, 33, 256, ONE, mode="mfma", cls="dups")
    add("mfma_k2", 4096, 32, 256, DIRECT, mode="mfma", entry="topk", knn=2, tie=TIE_KNN, cls="dups")
    add("direct_d64", 4096, 64, 256, DIRECT, mode="direct", cls="dups")
    add("direct_k8_fw", 1024, 20, 256, DIRECT, mode="direct", entry="fw", knn=8, tie=TIE_KNN, cls="hits")
    add("masked", 512, 32, 256, MASKED, cls="masked")
    # SOM maps: ragged (row order, zero padding rows) and 8x8 patch order
    add("som13x9", 117, 32, 256, TWO, som=(13, 9, TOPOL_HEXA), cls="zeros")
    add("som17x3", 51, 16, 256, DIRECT, som=(17, 3, TOPOL_RECT), cls="zeros")
    add("som1031x5", 5155, 32, 3841, TWO, som=(1031, 5, TOPOL_HEXA), cls="zeros")
    add("som1031x5_k4", 5155, 32, 512, ONE, som=(1031, 5, TOPOL_HEXA), entry="topk", knn=4, tie=TIE_KNN, cls="zeros")
    add("som1031x5_mfma", 5155, 33, 300, ONE, som=(1031, 5, TOPOL_HEXA), mode="mfma", cls="zeros")
    add("som64x64", 4096, 64, 3841, P("two_level", ring=True), som=(64, 64, TOPOL_HEXA), cls="dups")
    add("som64x64_k4", 4096, 64, 256, ONE, som=(64, 64, TOPOL_HEXA), entry="topk", knn=4, tie=TIE_KNN, cls="hits")
    # classes on the pre-filter routes: offset / one ulp, tiny codebook, fp32 norm overflow, NaN
    for cls in ("offset", "tiny", "huge", "allinf", "nan"):
        add("one_%s" % cls, 1024, 32, 200, ONE, cls=cls)
        add("two_%s" % cls, 1024, 32, 256, TWO, cls=cls)
        add("ring_%s" % cls, 4096, 64, 3841, P("two_level", ring=True), cls=cls)
        add("mfma_%s" % cls, 1024, 33, 256, ONE, mode="mfma", cls=cls)
    for cls in ("offset", "tiny", "huge", "allinf"):
        add("k4_%s" % cls, 4096, 32, 256, ONE, entry="topk", knn=4, tie=TIE_KNN, cls=cls)
        add("k8_%s" % cls, 32768, 64, 256, P("two_level", 8, True, True), entry="topk", knn=8, tie=TIE_KNN, cls=cls)
    add("huge_fw", 4096, 64, 3841, P("two_level", ring=True), entry="fw", cls="huge")
    add("huge_k2_first", 4096, 32, 256, ONE, entry="topk", knn=2, tie=TIE_FIRST, cls="huge")
    # crowded groups: the top-k pair list overflows, the one-wave re-rank decides
    add("crowd_k8", 24576, 16, 64, ONE, entry="topk", knn=8, tie=TIE_KNN, cls="crowd")
    add("crowd_k4_bygroup", 40960, 16, 64, ONE_BG, entry="topk", knn=4, tie=TIE_KNN, cls="crowd")
    add("crowd_k8_first", 24576, 16, 64, ONE, entry="topk", knn=8, tie=TIE_FIRST, cls="crowd")
    return cs


CASES = _cases()


# ------------------------------------------------------------------------------------------------ data classes
def make_data(c):
    """(codes [n, d], data [ndata, d], mask or None) for case c; the sample window is rows (first + i) % ndata"""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()))
    n, d, nd = c.n, c.d, c.ndata
    x, _ = synth(rs.randint(1 << 30), nd, d)
    pick = rs.randint(0, nd, size=n)
    codes = (x[pick] + 0.5 * rs.standard_normal((n, d))).astype(np.float32)
    win = (c.first + np.arange(c.count)) % nd           # data rows in the window, in search order
    mask = None

    def near(r, j, eps=0.01):                            # sample j (window position) close to code row r
        x[win[j]] = codes[r] + eps * rs.standard_normal(d).astype(np.float32)

    tie_rows = [0, n - 1] + [r for r in (63, 4095, 32767) if r + 1 < n]
    if c.cls in ("dups", "hits"):
        for r in tie_rows:
            if r + 1 < n:
                codes[r + 1] = codes[r]
        codes[n - 1] = codes[0]
        for k, r in enumerate(tie_rows):
            for t in range(3):
                j = (5 * k + t) % c.count
                if c.cls == "hits":
                    x[win[j]] = codes[r]                 # distance 0 to two rows at least
                else:
                    near(r, j)
    elif c.cls == "ulp":
        for k in range(min(16, n - 1)):
            r = rs.randint(0, n - 1)
            codes[r + 1] = codes[r]
            i = rs.randint(0, d)
            codes[r + 1, i] = np.nextafter(codes[r, i], np.float32(np.inf))
            x[win[(3 * k) % c.count]] = codes[r]
            if k % 2:
                x[win[(3 * k + 1) % c.count], i] = np.nextafter(codes[r + 1, i], np.float32(np.inf))
    elif c.cls == "offset":
        codes += np.float32(1500.0)
        x += np.float32(1500.0)
        for k in range(min(16, n - 1)):
            r = rs.randint(0, n - 1)
            codes[r + 1] = codes[r]
            i = rs.randint(0, d)
            codes[r + 1, i] = np.nextafter(codes[r, i], np.float32(np.inf))
            near(r, (2 * k) % c.count, eps=1e-3)
    elif c.cls == "tiny":
        codes = (1e-3 * rs.standard_normal((n, d))).astype(np.float32)
        x = (0.02 * x).astype(np.float32)
    elif c.cls == "zeros":
        x[win[::5]] = 0.0                                # zero samples: the zero padding rows must never win
        if n > 40:
            codes[n // 3] = 0.0                          # ... but a real zero row does
    elif c.cls == "huge":
        # a few samples ~3e19 per component and a code row equal to each: ||c||^2 overflows fp32, the distance is 0
        for k in range(4):
            j = (7 * k + 1) % c.count
            x[win[j]] = (3e19 * (1.0 + 0.1 * rs.standard_normal(d))).astype(np.float32)
            codes[(n // 4) * k + 1] = x[win[j]]
        x[win[2]] = (3e19 * (1.0 + 0.1 * rs.standard_normal(d))).astype(np.float32)   # ... and one without its row
    elif c.cls == "allinf":
        codes = (3e19 * (1.0 + rs.random_sample((n, d)))).astype(np.float32)
        x = (-3e19 * (1.0 + rs.random_sample((nd, d)))).astype(np.float32)
    elif c.cls == "nan":
        x[win[3], d // 2] = np.nan                       # nothing beats FLT_MAX: index -1
        codes[n // 2, d - 1] = np.nan                    # never wins
        near(n // 2, 4)
    elif c.cls == "crowd":
        v = codes[0].copy()
        codes[:] = v                                     # every row the same vector ...
        for k, r in enumerate((5, n // 2, n - 3)):
            codes[r] = v + np.float32(0.002 * (k + 1))   # ... but three
        for j in range(c.count):
            x[win[j]] = v + 0.01 * rs.standard_normal(d).astype(np.float32)
    elif c.cls == "masked":
        mask = (rs.random_sample((nd, d)) < 0.2).astype(np.uint8)
    return codes.astype(np.float32), x.astype(np.float32), mask


# ------------------------------------------------------------------------------------------------ references
def oracle_winners(oracle, codes, xs, knn, use_knn, mask=None):
    """oracle.winners over sample chunks on a thread pool (the C oracle releases the GIL)"""
    m = xs.shape[0]
    step = max(16, -(-m // (4 * WORKERS)))
    starts = list(range(0, m, step))

    def one(s):
        return oracle.winners(codes, xs[s:s + step], knn, use_knn, None if mask is None else mask[s:s + step])
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        parts = list(ex.map(one, starts))
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]))


def direct_form(codes, xs):
    """[m, n] fp32 distances with the reference's arithmetic: sum over dims in order of (c - x)^2, two roundings"""
    acc = np.zeros((xs.shape[0], codes.shape[0]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(codes.shape[1]):
            t = codes[None, :, i] - xs[:, None, i]
            acc = acc + t * t
    return acc


def first_rule_topk(codes, xs, k):
    """the k smallest (distance, row) keys in TIE_FIRST order (somhip_batch_topk_keys with SOMHIP_TIE_FIRST)"""
    idx = np.empty((xs.shape[0], k), dtype=np.int64)
    diff = np.empty((xs.shape[0], k), dtype=np.float32)
    for s in range(0, xs.shape[0], 64):
        dd = direct_form(codes, xs[s:s + 64])
        keys = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(codes.shape[0], dtype=np.uint64)
        best = np.sort(keys, axis=1)[:, :k]
        i, f = decode(best, False)
        idx[s:s + 64], diff[s:s + 64] = i, f
    return idx, diff


def decode(keys, inverted):
    """decode_key (host_scan.inc): index -1, diff -1 at or above FLT_MAX; tag, or ~tag under TIE_KNN"""
    keys = np.asarray(keys, dtype=np.uint64)
    bits = (keys >> np.uint64(32)).astype(np.uint32)
    tag = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    idx = (~tag if inverted else tag).astype(np.int32).astype(np.int64)
    diff = bits.view(np.float32).copy()
    none = bits >= FLT_MAX_BITS
    idx[none] = -1
    diff[none] = -1.0
    return idx, diff


# ------------------------------------------------------------------------------------------------ the engine side
@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    e.timing(True)
    yield e
    e.close()


def make_codebook(E, eng, c, codes):
    if c.som:
        xdim, ydim, topol = c.som
        return E.Codebook(eng, codes, topol, E.NEIGH_BUBBLE, xdim, ydim)
    return E.Codebook(eng, codes)


def run_search(E, eng, c, cb, ds):
    """(index [count, knn], diff [count, knn], ret or None) through the case's entry point"""
    from som_lvq_pak_amd import _lib
    if c.entry == "fw":
        idx, diff, ret = E.find_winners(cb, ds, c.first, c.count, c.knn, c.tie)
        return idx.astype(np.int64), diff, ret
    K = width(c.knn)
    buf = eng.device_alloc(8 * c.count * K)
    try:
        if c.entry == "bwk":
            _lib.check(eng.lib.somhip_batch_winner_keys(cb.h, ds.h, c.first, c.count, buf))
        else:
            _lib.check(eng.lib.somhip_batch_topk_keys(cb.h, ds.h, c.first, c.count, c.knn, c.tie, buf))
        keys = np.empty(c.count * K, dtype=np.uint64)
        _lib.check(eng.lib.somhip_copy_to_host(eng.h, keys.ctypes.data_as(C.c_void_p), buf, 8 * c.count * K))
    finally:
        eng.device_free(buf)
    idx, diff = decode(keys.reshape(c.count, K)[:, :c.knn], c.tie == TIE_KNN and c.knn > 1)
    return idx, diff, None


def check_kernels(c, plan, launched):
    """the timing table's launches agree with the plan"""
    ran = {k for k, (n, _) in launched.items() if n > 0}
    route, want = plan["route"], width(c.knn)
    gemm = {"k_dist_mfma", "k_dist_mfma_bf16", "k_dist_l2", "k_l2_select", "k_norms_tau"}
    if route == "masked":
        assert "k_scan_masked" in ran and not ran & gemm and "k_scan_exact" not in ran
    elif route == "direct":
        assert "k_scan_exact" in ran and not ran & gemm
        assert ("k_merge_topk" in ran) == (want > 1)
        assert not ran & {"k_rerank", "k_rerank_pairs", "k_rerank_select"}
    else:
        assert "k_scan_exact" not in ran and "k_merge_topk" not in ran and "k_norms_tau" in ran
        assert ("k_dist_mfma_bf16" if plan["bf16"] else "k_dist_mfma") in ran
        two = route == "two_level"
        assert ("k_dist_l2" in ran) == two and ("k_l2_select" in ran) == two
        if want == 1:
            assert {"k_rerank_select", "k_rerank_pairs", "k_rerank"} <= ran
        else:
            assert "k_rerank" in ran and "k_rerank_pairs" not in ran and "k_rerank_select" not in ran


def plan_key(plan):
    return (plan["route"], plan["kth"], plan["l1_ring"], plan["by_group"], plan["l2_global"])


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_route_matches_oracle(eng, oracle, c):
    from som_lvq_pak_amd import engine as E
    codes, x, mask = make_data(c)
    eng.set_scan_mode(c.mode)
    cb = make_codebook(E, eng, c, codes)
    ds = E.Dataset(eng, x, mask=mask)
    try:
        plan = E.scan_plan(cb, ds, min(c.count, 4096) if c.entry == "fw" else c.count, width(c.knn))
        assert plan_key(plan) == c.plan, plan
        assert plan["bf16"] == (c.mode == "mfma_bf16")
        assert plan["fused_gmin"] == (plan["route"] == "two_level" and width(c.knn) == 1)
        eng.timing_reset()
        idx, diff, ret = run_search(E, eng, c, cb, ds)
        check_kernels(c, plan, eng.timing_table())
        if c.cls == "crowd":
            assert eng.lvq_stats()["topk_overflow"] == 1, "the pair list did not overflow: the case misses its path"
    finally:
        cb.close()
        ds.close()
    win = (c.first + np.arange(c.count)) % c.ndata
    xs = x[win]
    ms = None if mask is None else mask[win]
    if c.entry == "topk" and c.tie == TIE_FIRST and c.knn > 1:
        widx, wdiff = first_rule_topk(codes, xs, c.knn)
        wret = None
    else:
        knn_rule = c.knn > 1
        widx, wdiff, wret = oracle_winners(oracle, codes, xs, c.knn, knn_rule, ms)
        wdiff = np.where(widx == -1, np.float32(-1.0), wdiff)     # the ABI's "nothing beat FLT_MAX" (decode_key)
    bad = np.nonzero((idx != widx).any(axis=1) | (diff.view(np.uint32) != wdiff.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%d of %d samples differ; first at %d: got %s %s, oracle %s %s" % (
        bad.size, c.count, bad[0], idx[bad[0]], diff[bad[0]], widx[bad[0]], wdiff[bad[0]])
    if ret is not None:
        assert np.array_equal(ret, wret)
    if c.cls == "zeros":
        assert idx.max() < c.n
    if c.cls == "mix" and (c.count >= 65504 or c.n >= 32768):
        f64_check(codes, xs, idx[:, 0], c.d)


def f64_check(codes, xs, got, d, nsub=2048):
    """float64: the returned row's distance is within 2 gamma_{d+2} (||x|| + ||c||)^2 of the minimum over all rows (the
    direct form's bound, prefilter_err3): a misreading of the arithmetic the oracle shares would show here"""
    rs = np.random.RandomState(d)
    sub = np.sort(rs.choice(xs.shape[0], size=min(nsub, xs.shape[0]), replace=False))
    cd = codes.astype(np.float64)
    cn = (cd * cd).sum(axis=1)
    u = 2.0 ** -24
    gam = (d + 2) * u / (1 - (d + 2) * u)
    beyond = 0
    for s in range(0, sub.size, 256):
        part = sub[s:s + 256]
        x = xs[part].astype(np.float64)
        xx = (x * x).sum(axis=1)
        dist = xx[:, None] + cn[None, :] - 2.0 * x @ cd.T
        best = dist.argmin(axis=1)
        mine = got[part]
        assert (mine >= 0).all()
        rows = np.arange(part.size)
        bound = 2.0 * gam * (np.sqrt(xx) + np.sqrt(np.maximum(cn[mine], cn[best]))) ** 2
        beyond += int((dist[rows, mine] - dist[rows, best] > bound).sum())
    assert beyond == 0, "float64: %d samples beyond the bound" % beyond


# ------------------------------------------------------------------------------------------------ completeness
def test_every_plan_has_a_case(eng):
    """The table's plans are every plan scan_plan can produce, and a sweep of shapes produces no other."""
    from som_lvq_pak_amd import engine as E
    assert {c.plan for c in CASES} == ALL_PLANS
    seen = set()
    for n in (63, 64, 4095, 4096, 32704, 32768):
        for d in (1, 24, 25, 31, 32, 56, 57, 61, 64, 512, 513, 543, 544, 1021, 1024, 1025, 1028):
            if n == 32704 and d > 64:
                continue
            cb = E.Codebook(eng, np.zeros((n, d), dtype=np.float32))
            ds = E.Dataset(eng, np.zeros((8, d), dtype=np.float32))
            for mode in ("direct", "mfma", "mfma_bf16"):
                eng.set_scan_mode(mode)
                for count in (31, 32, 224, 225, 3840, 3841, 65504, 65505, 131072, 131073):
                    for want in (1, 2, 4, 8):
                        seen.add(plan_key(E.scan_plan(cb, ds, count, want)))
            cb.close()
            ds.close()
    ds = E.Dataset(eng, np.zeros((8, 16), dtype=np.float32), mask=np.eye(8, 16, dtype=np.uint8))
    cb = E.Codebook(eng, np.zeros((64, 16), dtype=np.float32))
    seen.add(plan_key(E.scan_plan(cb, ds, 256, 1)))
    cb.close()
    ds.close()
    assert seen <= ALL_PLANS, seen - ALL_PLANS
    assert seen == ALL_PLANS, ALL_PLANS - seen
