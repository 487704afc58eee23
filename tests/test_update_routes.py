"""Every route of the SOM mini-batch update, at the thresholds that choose it.

The update's choices -- the apply kernel, chunks or tiles per wave, the winners' decode, the members kernel's form, what
its entries carry, the list tail, the group order -- are made in one place (som_update_plan, host_som.inc).  Each case
below runs one batch and asserts that plan (somhip_debug_update_plan), the kernels that ran (the timing table's launch
counts) as a second witness, and the result: exact-mode forms equal the batch oracle bit for bit (codebook and winner
trace; on maps of tens of MiB, the other exact kernel forced by SOMHIP_UPD_LDS on the same run), gemm forms give exact
mode's winners on the same run and lie within the tolerances of test_gpu_parity (8e-6 scale bubble, 2e-5 scale
gaussian).  The data set of the float4-offset case is 4 GiB, generated in HBM; the oracle reads its window through
Dataset.rows.  test_update_plan_thresholds checks the plan on both sides of the thresholds without running an update
(all but two: the gaussian kernels' n < 2^31 rows and the scalar and gemm forms' n d / 4 < 2^32 would need data sets of
64 GiB and more); test_every_update_plan_has_a_case keeps the table complete.  Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu

HEXA, RECT, BUBBLE, GAUSS = 3, 4, 1, 2
KERNEL = {"gemm": "k_som_update_gemm", "bubble_s": "k_som_update_bubble_s", "gauss_h": "k_som_update_run",
          "gauss_s": "k_som_update_run", "run": "k_som_update_run"}
FIELDS = ("apply", "qw", "off32", "ntw", "decode", "members_nt", "members_rr", "entry", "gauss_gemm", "tail", "tail_cut",
          "reach", "order")
# every value every field of the plan can take (tail_cut: tail_need > 0; reach: reach_max >= 0)
ALL_VALUES = {"apply": {"gemm", "gauss_h", "gauss_s", "bubble_s", "run"}, "qw": {0, 2, 4}, "off32": {False, True},
              "ntw": {0, 1, 2, 4}, "decode": {False, True}, "members_nt": {256, 1024}, "members_rr": {4, 8},
              "entry": {"sample", "float4", "byte"}, "gauss_gemm": {False, True}, "tail": {False, True},
              "tail_cut": {False, True}, "reach": {False, True}, "order": {False, True}}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def key(plan):
    k = dict(plan, tail_cut=plan["tail_need"] > 0, reach=plan["reach_max"] >= 0)
    return {f: k[f] for f in FIELDS}


def P(apply, qw=0, off32=False, ntw=0, decode=False, nt=256, rr=4, entry="sample", gauss_gemm=False, tail=False,
      tail_cut=False, reach=False, order=True):
    return dict(apply=apply, qw=qw, off32=off32, ntw=ntw, decode=decode, members_nt=nt, members_rr=rr, entry=entry,
                gauss_gemm=gauss_gemm, tail=tail, tail_cut=tail_cut, reach=reach, order=order)


class Case:
    def __init__(self, name, xd, yd, d, plan, neigh=BUBBLE, topol=HEXA, mode="exact", B=256, n=None, first=0,
                 alpha=0.05, radius=6.0, length=None, masked=False, ref="oracle", gen=False):
        self.name, self.xd, self.yd, self.d, self.plan = name, xd, yd, d, plan
        self.neigh, self.topol, self.mode, self.B, self.first = neigh, topol, mode, B, first
        self.n = n or B + 44
        self.alpha, self.radius, self.length, self.masked = alpha, radius, length or B, masked
        self.ref = ref        # "oracle": the batch oracle; "lds": the LDS-tile kernel (SOMHIP_UPD_LDS); gemm: exact mode
        self.gen = gen        # the data set is generated in HBM (somhip_dataset_generate), n rows

    def __repr__(self):
        return self.name


CASES = [
    # exact mode, small maps: the batch oracle is the yardstick
    Case("run_masked_qw2", 16, 16, 16, P("run", qw=2), masked=True),
    Case("bubble_s_qw2_off32", 16, 16, 32, P("bubble_s", qw=2, off32=True, entry="byte")),
    Case("run_qw2_d36", 16, 16, 36, P("run", qw=2), topol=RECT),                        # d4 % 8 != 0
    Case("gauss_h", 16, 16, 32, P("gauss_h", decode=True), neigh=GAUSS, n=600),
    Case("gauss_s_wrap", 16, 16, 32, P("gauss_s", decode=True), neigh=GAUSS, n=600, first=500),
    Case("gauss_s_d48", 13, 9, 48, P("gauss_s", decode=True), neigh=GAUSS, topol=RECT),   # d4 % 8 != 0
    Case("gauss_wide", 16, 16, 32, P("gauss_h", decode=True, nt=1024), neigh=GAUSS, B=1025),
    Case("gauss_masked_run", 16, 16, 32, P("run", qw=2, decode=True), neigh=GAUSS, masked=True),
    Case("wide_1025", 16, 16, 8, P("run", qw=2, nt=1024), B=1025),
    Case("long_16383", 32, 24, 8, P("run", qw=2, nt=1024), B=16383),
    Case("long_16384_deep", 32, 24, 8, P("run", qw=2, decode=True, nt=1024, rr=8, reach=True), B=16384),
    Case("long_16384_bubble_s", 32, 24, 32, P("bubble_s", qw=2, off32=True, entry="byte", decode=True, nt=1024, rr=8,
                                              reach=True), B=16384, radius=3.0),
    # more than 8192 row groups: no group order; QW 4 by the group count
    Case("no_order_qw4", 1024, 520, 4, P("run", qw=4, order=False), radius=3.0),
    # 32 MiB map: QW 4 by size, the scalar-operand kernel against the LDS-tile kernel on the same run
    Case("bubble_s_qw4", 256, 128, 256, P("bubble_s", qw=4, off32=True, entry="byte"), B=512, radius=8.0, ref="lds"),
    # ... and on a data set of exactly 4 GiB: float4 row offsets in the entries (no OFF32), the window past 2^32 bytes
    Case("bubble_s_qw4_4gib", 256, 128, 256, P("bubble_s", qw=4, entry="float4"), B=512, n=4194304, first=4194304 - 600,
         radius=8.0, gen=True),
    # update mode gemm: exact mode on the same run is the yardstick
    Case("gemm_tail", 32, 24, 128, P("gemm", ntw=1, entry="float4", tail=True, tail_cut=True), mode="gemm", B=512,
         alpha=0.3, length=100000),
    Case("gemm_tail_whole", 32, 24, 128, P("gemm", ntw=1, entry="float4", tail=True), mode="gemm", B=512),
    Case("gemm_gauss", 32, 24, 128, P("gemm", ntw=1, decode=True, entry="float4", gauss_gemm=True), neigh=GAUSS,
         mode="gemm", B=512, length=100000),
    Case("gemm_ntw2", 256, 256, 256, P("gemm", ntw=2, entry="float4", tail=True, tail_cut=True), mode="gemm", B=2048,
         n=4096, alpha=0.3, radius=30.0, length=100000),
    Case("gemm_gauss_ntw4", 256, 128, 1024, P("gemm", ntw=4, decode=True, entry="float4", gauss_gemm=True), neigh=GAUSS,
         mode="gemm", B=256, length=100000),
    Case("gemm_long_nt256", 64, 512, 128, P("gemm", ntw=1, decode=True, entry="float4", tail=True, tail_cut=True,
                                            reach=True), mode="gemm", B=16384, alpha=0.3, radius=64.0, length=1000000),
    Case("gemm_long_deep", 64, 512, 128, P("gemm", ntw=1, decode=True, nt=1024, rr=8, entry="float4", tail=True,
                                           reach=True), mode="gemm", B=16384, alpha=0.05, radius=8.0),
]


# the apply kernel's grid and workgroup size the plan reports for each case
LAUNCH = {"run_masked_qw2": (4, 256), "bubble_s_qw2_off32": (4, 256), "run_qw2_d36": (8, 256), "gauss_h": (4, 64),
          "gauss_s_wrap": (4, 128), "gauss_s_d48": (2, 192), "gauss_wide": (4, 64), "gauss_masked_run": (4, 256),
          "wide_1025": (4, 256), "long_16383": (12, 256), "long_16384_deep": (12, 256), "long_16384_bubble_s": (12, 256),
          "no_order_qw4": (8320, 256), "bubble_s_qw4": (2048, 256), "bubble_s_qw4_4gib": (2048, 256), "gemm_tail": (12, 256),
          "gemm_tail_whole": (12, 256), "gemm_gauss": (12, 256), "gemm_ntw2": (1024, 256), "gemm_gauss_ntw4": (1024, 256),
          "gemm_long_nt256": (512, 256), "gemm_long_deep": (512, 256)}


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


def make_inputs(E, eng, c):
    """(data set, the run's window of rows, initial codebook, the window's mask or None)"""
    rs = np.random.RandomState(sum(map(ord, c.name)))
    win = (c.first + np.arange(c.B)) % c.n
    if c.gen:
        assert c.first + c.B <= c.n
        ds = E.Dataset(eng, generate=(rs.randint(1 << 30), 16, c.d, 0, c.n))
        x, xw, mask = None, ds.rows(c.first, c.B), None
    else:
        x, _ = synth(rs.randint(1 << 30), c.n, c.d)
    pool = xw if c.gen else x
    ini = (pool[rs.randint(0, pool.shape[0], c.xd * c.yd)] + 0.3 * rs.standard_normal((c.xd * c.yd, c.d))).astype(np.float32)
    if not c.gen:
        mask = (rs.random_sample((c.n, c.d)) < 0.2).astype(np.uint8) if c.masked else None
        ds, xw = E.Dataset(eng, x, mask=mask), x[win]
        mask = None if mask is None else mask[win]
    return ds, xw, ini, mask


def train(eng, E, c, ini, ds, mode, env=None, monkeypatch=None):
    """one batch of case c in update mode `mode`: (plan, kernels launched, codebook, winner trace)"""
    eng.set_update_mode(mode)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        cb = E.Codebook(eng, ini, c.topol, c.neigh, c.xd, c.yd)
        plan = E.update_plan(cb, ds, c.length, c.alpha, c.radius, c.B, data_first=c.first)
        eng.timing(True)
        eng.timing_reset()
        ti, _ = E.som_train(cb, ds, c.length, c.alpha, c.radius, batch=c.B, count=c.B, data_first=c.first)
        ran = {k: n for k, (n, _) in eng.timing_table().items()}
        eng.timing(False)
        out = cb.download()
        cb.close()
    finally:
        eng.set_update_mode("exact")
        for k in env or {}:
            monkeypatch.delenv(k, raising=False)
    return plan, ran, out, ti


def check_kernels(plan, ran):
    """the timing table's launches agree with the plan (k_order_groups is timed as k_decode_winners)"""
    assert ran["k_som_members"] == 1
    assert ran["k_decode_winners"] == int(plan["decode"]) + int(plan["order"])
    for name in set(KERNEL.values()):
        assert ran[name] == (1 if name == KERNEL[plan["apply"]] else 0), name


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_update_route(eng, E, oracle, monkeypatch, c):
    ds, xw, ini, mask = make_inputs(E, eng, c)
    try:
        plan, ran, got, ti = train(eng, E, c, ini, ds, c.mode)
        assert key(plan) == c.plan, plan
        assert (plan["grid"], plan["block"]) == LAUNCH[c.name], plan
        check_kernels(plan, ran)
        if c.mode == "gemm":
            _, _, want, wi = train(eng, E, c, ini, ds, "exact")
            assert np.array_equal(ti, wi)
            tol = 2e-5 if c.neigh == GAUSS else 8e-6
            assert float(np.abs(got - want).max()) <= tol * float(np.abs(want).max())
        elif c.ref == "lds":
            lplan, _, want, wi = train(eng, E, c, ini, ds, "exact", {"SOMHIP_UPD_LDS": "1"}, monkeypatch)
            assert lplan["apply"] == "run" and lplan["qw"] == plan["qw"]
            assert np.array_equal(ti, wi) and np.array_equal(bits(got), bits(want))
        else:
            assert c.length == c.B                        # the oracle starts at iteration 0: the run's window is its data
            want, wi, _ = oracle.som_train(ini, c.xd, c.yd, c.topol, c.neigh, xw, c.B, c.alpha, c.radius, mask=mask,
                                           batch=c.B)
            assert np.array_equal(ti, wi)
            assert np.array_equal(bits(got), bits(want))
    finally:
        ds.close()


# ------------------------------------------------------------------------------------------------ plans only
def plan_with(eng, E, cb, ds, B, mode="exact", first=0, alpha=0.05, radius=6.0, length=None):
    eng.set_update_mode(mode)
    try:
        return E.update_plan(cb, ds, length or B, alpha, radius, B, data_first=first)
    finally:
        eng.set_update_mode("exact")


def plan_of(eng, E, xd, yd, d, ds, B, mode="exact", neigh=BUBBLE, **kw):
    cb = E.Codebook(eng, np.zeros((xd * yd, d), dtype=np.float32), HEXA, neigh, xd, yd)
    try:
        return plan_with(eng, E, cb, ds, B, mode, **kw)
    finally:
        cb.close()


def test_update_plan_thresholds(eng, E):
    """both sides of every threshold of som_update_plan; no update runs (the > 4 GiB data sets are generated in HBM)"""
    def rows(n, d, masked=False):
        x = np.zeros((n, d), dtype=np.float32)
        return E.Dataset(eng, x, mask=np.ones((n, d), dtype=np.uint8) if masked else None)

    ds = rows(70000, 16)
    # chunks per wave: row groups x ceil(d4 / 4) >= 8192; group order: <= 8192 row groups
    assert key(plan_of(eng, E, 64, 8191, 16, ds, 256)) == P("run", qw=2)
    assert key(plan_of(eng, E, 64, 8192, 16, ds, 256)) == P("run", qw=4)
    assert key(plan_of(eng, E, 64, 8193, 16, ds, 256)) == P("run", qw=4, order=False)
    # members: 1024 threads for fewer than 512 row groups and runs over 1024; decoded winners from 16384 samples on
    assert plan_of(eng, E, 16, 16, 16, ds, 1024)["members_nt"] == 256
    assert plan_of(eng, E, 16, 16, 16, ds, 1025)["members_nt"] == 1024
    assert plan_of(eng, E, 64, 511, 16, ds, 1025)["members_nt"] == 1024
    assert plan_of(eng, E, 64, 512, 16, ds, 1025)["members_nt"] == 256
    assert plan_of(eng, E, 64, 512, 16, ds, 8191)["members_nt"] == 256
    assert plan_of(eng, E, 64, 512, 16, ds, 8192)["members_nt"] == 1024          # long run, whole lists
    assert key(plan_of(eng, E, 16, 16, 16, ds, 16383)) == P("run", qw=2, nt=1024)
    assert key(plan_of(eng, E, 16, 16, 16, ds, 16384)) == P("run", qw=2, decode=True, nt=1024, rr=8, reach=True)
    ds.close()
    ds = rows(20000, 16, masked=True)                                             # every sample skipped: no reach
    assert key(plan_of(eng, E, 16, 16, 16, ds, 16384)) == P("run", qw=2, decode=True, nt=1024)
    ds.close()
    # gauss_h: the run in one piece of the data set; gauss_s otherwise; no gaussian scalar kernel beyond n samples
    ds = rows(1000, 32)
    assert plan_of(eng, E, 16, 16, 32, ds, 500, neigh=GAUSS, first=500)["apply"] == "gauss_h"
    assert plan_of(eng, E, 16, 16, 32, ds, 500, neigh=GAUSS, first=501)["apply"] == "gauss_s"
    assert plan_of(eng, E, 16, 16, 32, ds, 1000, neigh=GAUSS)["apply"] == "gauss_h"
    assert plan_of(eng, E, 16, 16, 32, ds, 1001, neigh=GAUSS)["apply"] == "run"
    assert plan_of(eng, E, 16, 16, 32, ds, 1000)["apply"] == "bubble_s"
    assert plan_of(eng, E, 16, 16, 32, ds, 1001)["apply"] == "run"                # count <= n
    ds.close()
    # gemm: dims in whole 128s, runs up to 65504 samples, rates in [0, 1], gaussian map sides up to 1024
    ds = rows(65505, 128)
    assert plan_of(eng, E, 16, 16, 128, ds, 65504, "gemm")["apply"] == "gemm"
    assert key(plan_of(eng, E, 16, 16, 128, ds, 65505, "gemm")) == P("bubble_s", qw=2, off32=True, entry="byte",
                                                                       decode=True, nt=1024, rr=8, reach=True)
    assert plan_of(eng, E, 16, 16, 128, ds, 512, "gemm", alpha=1.0)["apply"] == "gemm"
    assert plan_of(eng, E, 16, 16, 128, ds, 512, "gemm", alpha=1.5)["apply"] == "bubble_s"
    assert key(plan_of(eng, E, 1024, 4, 128, ds, 48, "gemm", neigh=GAUSS)) == \
        P("gemm", ntw=1, decode=True, entry="float4", gauss_gemm=True)
    assert plan_of(eng, E, 1025, 4, 128, ds, 48, "gemm", neigh=GAUSS)["apply"] == "gauss_h"
    # the list tail: (1 - a_min)^need < 2^-24 within half the run
    p = plan_of(eng, E, 32, 24, 128, ds, 512, "gemm", alpha=0.3, length=100000)
    assert p["tail"] and p["tail_need"] == 64
    p = plan_of(eng, E, 32, 24, 128, ds, 127, "gemm", alpha=0.3, length=100000)
    assert p["tail"] and p["tail_need"] == 0
    ds.close()
    ds = rows(100, 96)
    assert plan_of(eng, E, 16, 16, 96, ds, 64, "gemm")["apply"] == "bubble_s"
    ds.close()
    # gemm tiles per wave: by dims, by expected list length, by the grid (1024 workgroups)
    ds = rows(4096, 256)
    assert plan_of(eng, E, 256, 256, 256, ds, 2048, "gemm", radius=30.0, length=100000)["ntw"] == 2
    assert plan_of(eng, E, 256, 248, 256, ds, 2048, "gemm", radius=30.0, length=100000)["ntw"] == 1
    assert plan_of(eng, E, 256, 256, 256, ds, 256, "gemm", radius=2.0, length=100000)["ntw"] == 1
    ds.close()
    ds = rows(256, 1024)
    assert plan_of(eng, E, 256, 128, 1024, ds, 256, "gemm", neigh=GAUSS)["ntw"] == 4
    assert plan_of(eng, E, 256, 120, 1024, ds, 256, "gemm", neigh=GAUSS)["ntw"] == 2
    ds.close()
    # byte offsets (OFF32) for data sets below 4 GiB; at 2 chunks per wave the scalar kernel needs them
    for n, off32 in ((4194303, True), (4194304, False)):
        ds = E.Dataset(eng, generate=(7, 4, 256, 0, n))
        assert key(plan_of(eng, E, 256, 128, 256, ds, 512)) == \
            P("bubble_s", qw=4, off32=off32, entry="byte" if off32 else "float4")
        assert plan_of(eng, E, 16, 16, 256, ds, 512)["apply"] == ("bubble_s" if off32 else "run")
        if n == 4194304:
            # gauss_h: the run's rows below 4 GiB (count d 4 < 2^32)
            assert plan_of(eng, E, 16, 16, 256, ds, n - 1, neigh=GAUSS)["apply"] == "gauss_h"
            assert plan_of(eng, E, 16, 16, 256, ds, n, neigh=GAUSS)["apply"] == "gauss_s"
        ds.close()


def test_every_update_plan_has_a_case(eng, E):
    """The table's plans take every value of every field, and a sweep of shapes and runs produces no other."""
    for f in FIELDS:
        assert {c.plan[f] for c in CASES} == ALL_VALUES[f], f
    seen = {f: set() for f in FIELDS}
    for d, n in ((8, 20000), (32, 20000), (128, 70000)):
        dss = [E.Dataset(eng, np.zeros((n, d), dtype=np.float32)),
               E.Dataset(eng, np.zeros((n, d), dtype=np.float32), mask=np.eye(n, d, dtype=np.uint8))]
        for xd, yd in ((16, 16), (64, 511), (64, 512), (1025, 4), (64, 8193)):
            for neigh in (BUBBLE, GAUSS):
                cb = E.Codebook(eng, np.zeros((xd * yd, d), dtype=np.float32), HEXA, neigh, xd, yd)
                for ds in dss:
                    for mode in ("exact", "gemm"):
                        for B in (64, 1025, 8192, 16384, 65505):
                            for alpha, first in ((0.05, 0), (0.3, n - 100), (1.5, 0)):
                                p = key(plan_with(eng, E, cb, ds, B, mode, first, alpha, 8.0, 100000))
                                for f in FIELDS:
                                    seen[f].add(p[f])
                cb.close()
        for ds in dss:
            ds.close()
    for f in FIELDS:
        assert seen[f] <= ALL_VALUES[f], (f, seen[f] - ALL_VALUES[f])
