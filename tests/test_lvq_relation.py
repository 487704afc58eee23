"""Relation (*) of the exact batched LVQ engine and its components, one batch at a time, against a float64 replay.

somhip_debug_lvq_relation runs one batch's front and relation as somhip_lvq_train would and returns what they made;
tests/lvq_relation_replay.py states what they must make.  Per case:
  (a) the candidate keys are the replay's, as bits;
  (b) rho, the fp32 norms and amax lie in their bands;
  (c) soundness: every pair of the slack-free relation `must` has an edge (a missing edge lets two workgroups stage the
      same code row -- the end-to-end tests only notice if the two samples really share a winner in that batch);
  (d) tightness: no pair beyond the documented slack (`must_not`) has one (an engine that answers "edge" everywhere is
      exact and serial; only a count of components in one end-to-end case would notice);
  (e) the bit rows are symmetric, with a clear diagonal and no bit at or above count;
  (f) the components are those of the returned adjacency by a host union-find, in the documented order;
  (g) the plan names the pair kernel the case was written for.
somhip_debug_lvq_components runs k_lvq_components alone on made graphs.

The parts without the gpu marker need no GPU: the replay's cases are not vacuous (enough pairs on either side of the
band, few inside), the huge-value recipe is finite in the replay and in the oracle, and each checker can fail."""
import zlib

import numpy as np
import pytest

import lvq_relation_replay as R
from conftest import synth

gpu = pytest.mark.gpu
ALPHA_LINEAR, ALPHA_INVERSE_T = 1, 2
LVQ1, OLVQ1, LVQ2, LVQ3 = 1, 2, 3, 4


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, name, d, count, cls="plain", kind=LVQ1, ncodes=160, ndata=None, first=0, k=6, length=100000,
                 alpha=0.05, alpha_type=ALPHA_LINEAR, winlen=0.3, epsilon=0.1, start_iter=0, masked=False, rates=None):
        self.name, self.d, self.count, self.cls, self.kind = name, d, count, cls, kind
        self.ncodes, self.k, self.masked, self.rates = ncodes, k, masked, rates
        self.ndata = ndata or count + 7
        self.first = first
        self.length, self.alpha, self.alpha_type, self.winlen, self.epsilon = length, alpha, alpha_type, winlen, epsilon
        self.start_iter = start_iter
        self.pairs = "masked" if masked else "mfma" if d % 8 == 0 else "direct"
        self.form = "gram" if self.pairs == "mfma" else "direct"

    @property
    def plain(self):                    # a Gaussian mixture at scale 1: the vacuity floors apply
        return self.cls == "plain"

    def __repr__(self):
        return self.name


def _cases():
    cs = []

    def add(name, *a, **k):
        cs.append(Case(name, *a, **k))

    # every count on each kernel: one sample, the 64-pair tile's border, more than one tile, the last tile partial, full
    for count in (1, 63, 64, 65, 129, 1000, 1024):
        add("gram_d32_n%d" % count, 32, count, k=8)
        add("direct_d12_n%d" % count, 12, count, kind=LVQ2, k=7)
        add("masked_d13_n%d" % count, 13, count, masked=True, k=6)
    # the Gram kernel's k0 + 32 <= d loop and its 8-wide tail; the direct kernel's float4 and scalar loads, with tails
    for d in (8, 24, 40, 64):
        add("gram_d%d" % d, d, 129, k=6 + d // 8)
    for d in (36, 1, 3, 13, 33):
        add("direct_d%d" % d, d, 129, k=6 if d < 4 else 10, ncodes=96 if d < 4 else 160)
    add("masked_d16", 16, 129, masked=True, kind=LVQ3, k=9)          # word mask loads (d % 4 == 0); d13: byte loads
    # the data window wraps; a window longer than the data (the same row twice: distance 0, joined)
    add("wrap_gram", 32, 129, ndata=200, first=195, k=12)
    add("wrap_direct", 13, 65, ndata=90, first=85, k=6)
    add("wrap_masked", 16, 129, ndata=150, first=145, masked=True, k=6)
    add("short_data_gram", 24, 129, ndata=40, first=0, k=6)
    add("short_data_direct", 13, 129, ndata=40, first=33, k=6)
    # tiny codebook: no list is full, rho = +inf, one component
    add("tiny_gram", 32, 129, cls="tiny", ncodes=6)
    add("tiny_direct", 13, 129, cls="tiny", ncodes=6, kind=LVQ2)
    add("tiny_masked", 13, 65, cls="tiny", ncodes=6, masked=True)
    # the four kinds and their rate bounds
    add("invt_lvq1", 32, 129, alpha_type=ALPHA_INVERSE_T, length=5000, start_iter=300, alpha=0.3, k=10)
    add("lvq2_late", 12, 129, kind=LVQ2, length=4000, start_iter=3871, alpha=0.2, k=8)
    add("lvq3_eps", 32, 129, kind=LVQ3, epsilon=2.5, alpha=0.1, k=14)
    add("lvq3_eps_direct", 13, 129, kind=LVQ3, epsilon=2.5, alpha=0.1, k=8)
    add("olvq1_rates", 32, 129, kind=OLVQ1, rates="ok", alpha=0.3, k=9)
    add("olvq1_rates_masked", 13, 129, kind=OLVQ1, rates="ok", alpha=0.3, masked=True, k=6)
    add("olvq1_rate_one", 32, 129, cls="unknown", kind=OLVQ1, rates="one", alpha=0.3)
    add("olvq1_rate_one_direct", 13, 65, cls="unknown", kind=OLVQ1, rates="one", alpha=0.3)
    add("alpha_nan", 32, 129, cls="unknown", alpha=float("nan"))
    add("alpha_nan_masked", 13, 65, cls="unknown", alpha=float("nan"), masked=True, kind=LVQ3)
    # pairs at the threshold
    add("sweep_direct", 12, 128, cls="sweep", ndata=128, alpha=0.05)
    add("sweep_gram", 32, 128, cls="sweep", ndata=128, alpha=0.05)
    add("sweep_masked", 16, 128, cls="sweep", ndata=128, alpha=0.05, masked=True)
    # a NaN among a sample's values: no distance of that sample is a number, so nothing separates it from anyone
    add("nan_gram", 32, 129, cls="nan", k=8)
    add("nan_direct", 13, 129, cls="nan", k=6)
    # large norms: the Gram slack grows with them
    add("offset_gram", 64, 129, cls="offset", k=8)
    # fp32 norms overflow, distances between neighbours do not
    add("huge_gram", 16, 256, cls="huge", ncodes=40, ndata=256)
    add("huge_direct", 13, 256, cls="huge", ncodes=40, ndata=256)
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def window(c):
    return (c.first + np.arange(c.count)) % c.ndata


def huge_data(d, ndata=256, ncodes=40):
    """the huge-value recipe: components 2e19 (1 + 0.02 synth), codes drawn from the data"""
    x, lab = synth(1234 + d, ndata, d)
    x = (2e19 * (1.0 + 0.02 * x.astype(np.float64))).astype(np.float32)
    pick = np.random.RandomState(77 + d).choice(ndata, size=ncodes, replace=False)
    return x, lab, x[pick].copy(), lab[pick].copy()


def make_sweep(c, rs):
    """64 pairs x_j = x_i + s e_0 with s from 0.98 to 1.05 of (1 + amax)(R_i + R_j).  Every sample has 12 code rows of its
    own at distance 0.8 .. 1 in the subspace orthogonal to e_0, the same offsets for both samples of a pair: x_j's rows
    move with it, x_i's rows are sqrt(s^2 + |offset|^2) away from it, so x_j's list does not depend on s."""
    d, npair = c.d, 64
    amax = float(R.amax_schedule(R.alpha_schedule(c.alpha_type, c.start_iter, c.count, c.length, c.alpha), c.epsilon))
    cen = rs.uniform(-3.0, 3.0, size=(npair, d))
    off = rs.standard_normal((npair, 12, d))
    off[:, :, 0] = 0.0
    off *= (rs.uniform(0.8, 1.0, size=(npair, 12, 1)) / np.sqrt((off * off).sum(axis=2, keepdims=True)))
    mask = None
    if c.masked:
        mask = (rs.random_sample((2 * npair, d)) < 0.2).astype(np.uint8)
        mask[:, 0] = 0

    def build(s):
        x = np.empty((2 * npair, d))
        x[0::2] = cen
        x[1::2] = cen
        x[1::2, 0] += s
        codes = np.concatenate([x[0::2, None, :] + off, x[1::2, None, :] + off], axis=1).reshape(-1, d)
        return x.astype(np.float32), codes.astype(np.float32)
    x, codes = build(np.full(npair, 2.1))
    rad = R.radii(R.topk_keys(codes, x, mask))
    s = (0.98 + 0.07 * np.arange(npair) / (npair - 1)) * (1.0 + amax) * (rad[0::2] + rad[1::2])
    x, codes = build(s)
    return {"codes": codes, "clab": rs.randint(1, 4, size=codes.shape[0]).astype(np.int32), "x": x,
            "xlab": rs.randint(1, 4, size=2 * npair).astype(np.int32), "mask": mask, "talpha": None}


def make_case(c):
    rs = np.random.RandomState(zlib.crc32(c.name.encode()))
    if c.cls == "sweep":
        return make_sweep(c, rs)
    if c.cls == "huge":
        x, xlab, codes, clab = huge_data(c.d, c.ndata, c.ncodes)
        return {"codes": codes, "clab": clab, "x": x, "xlab": xlab, "mask": None, "talpha": None}
    x, xlab = synth(rs.randint(1 << 30), c.ndata, c.d, k=c.k)
    pick = rs.randint(0, c.ndata, size=c.ncodes)
    codes = (x[pick] + 0.5 * rs.standard_normal((c.ncodes, c.d))).astype(np.float32)
    clab = xlab[pick].copy()
    if c.cls == "offset":
        x, codes = x + np.float32(1500.0), codes + np.float32(1500.0)
    mask, talpha = None, None
    win = window(c)
    if c.cls == "nan":
        x = x.copy()
        x[win[5], c.d // 2] = np.nan
    if c.masked:
        mask = (rs.random_sample(x.shape) < 0.2).astype(np.uint8)
        if c.count >= 8:                             # two samples of the window without a common component
            a, b = win[3], win[c.count - 2]
            mask[a] = np.arange(c.d) % 2
            mask[b] = 1 - mask[a]
        mask[mask.all(axis=1), 0] = 0                # (a row with every component masked is refused)
        x = x.copy()
        poison = np.where(rs.random_sample(x.shape) < 0.5, np.float32(np.nan), np.float32(1e30))
        x[mask != 0] = poison[mask != 0]             # whatever a masked position stores is never read into a result
    if c.rates:
        talpha = rs.uniform(0.01, 0.25, size=c.ncodes).astype(np.float32)
        if c.rates == "one":                         # a listed row with rate 1.0: no bound
            k0 = R.topk_keys(codes, x[win[:1]], None if mask is None else mask[win[:1]])
            talpha[int(k0[0, 2] & np.uint64(0xFFFFFFFF))] = 1.0
    return {"codes": codes, "clab": clab, "x": x.astype(np.float32), "xlab": xlab, "mask": mask, "talpha": talpha}


_REPLAYS = {}


def replay(c):
    """the case's data and everything the replay says about it, computed once and shared (read only)"""
    if c.name in _REPLAYS:
        return _REPLAYS[c.name]
    data = make_case(c)
    win = window(c)
    xs = data["x"][win]
    ms = None if data["mask"] is None else data["mask"][win]
    knn2 = c.kind >= LVQ2
    keys = R.topk_keys(data["codes"], xs, ms, knn2)
    rad = R.radii(keys)
    if c.kind == OLVQ1:
        amax = R.amax_olvq(keys, knn2, data["talpha"], c.alpha)
    else:
        amax = R.amax_schedule(R.alpha_schedule(c.alpha_type, c.start_iter, c.count, c.length, c.alpha), c.epsilon)
    D = R.pair_distances(xs, ms)
    N64 = R.own_norms(xs, ms)
    must = R.must_pairs(D, rad, amax)
    # what the replay expects rho to be (the engine's own rho judges tightness on the GPU; this one the vacuity floors)
    with np.errstate(over="ignore"):
        n32 = N64.astype(np.float32)
        v = R.rho_value(rad, amax, n32)
        rho = v.astype(np.float32)
        rho = np.where(rho.astype(np.float64) < v, np.nextafter(rho, np.float32(np.inf)), rho)
    out = {"data": data, "xs": xs, "ms": ms, "keys": keys, "rad": rad, "amax": amax, "D": D, "N64": N64, "must": must,
           "must_not": R.must_not_pairs(D, rho, n32, c.d, c.form)}
    _REPLAYS[c.name] = out
    return out


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_replay_cases_are_not_vacuous(c):
    """From the replay alone: a plain case has at least 5 % of its pairs on either side of the band and at most 2 %
    inside; the degenerate classes are what their names say; the sweep's pairs straddle the threshold."""
    rep = replay(c)
    must, must_not = rep["must"], rep["must_not"]
    assert not (must & must_not).any()
    assert np.array_equal(must, must.T) and np.array_equal(must_not, must_not.T)
    pairs = c.count * (c.count - 1)
    if c.plain and pairs:
        assert 6 <= c.k <= 20
        assert must.sum() >= 0.05 * pairs, must.sum() / pairs
        assert must_not.sum() >= 0.05 * pairs, must_not.sum() / pairs
        assert pairs - must.sum() - must_not.sum() <= 0.02 * pairs
        assert np.isfinite(rep["rad"]).all() and rep["amax"] is not None
    if c.cls == "tiny":
        assert np.isinf(rep["rad"]).all() and must.sum() == pairs
    if c.cls == "unknown":
        assert rep["amax"] is None and must.sum() == pairs
    if c.kind == OLVQ1 and c.cls != "unknown":
        assert rep["amax"] is not None and np.float32(c.alpha) <= rep["amax"] < 1
    if c.kind == LVQ3 and c.epsilon > 1 and rep["amax"] is not None:
        assert rep["amax"] > np.abs(R.alpha_schedule(c.alpha_type, c.start_iter, c.count, c.length, c.alpha)).max()
    if c.masked and c.count >= 8 and c.cls != "sweep":
        a, b = 3, c.count - 2
        assert not ((rep["ms"][a] == 0) & (rep["ms"][b] == 0)).any() and rep["D"][a, b] == 0.0 and must[a, b]
    if c.ndata < c.count:
        assert must[0, c.ndata] and rep["D"][0, c.ndata] == 0.0           # the same row twice
    if c.cls == "sweep":
        i, j = np.arange(0, c.count, 2), np.arange(1, c.count, 2)
        assert must[i, j].sum() >= 8 and must_not[i, j].sum() >= 8
        assert must[i, j][:8].all() and must_not[i, j][-8:].all()
        assert np.isfinite(rep["rad"]).all()
    if c.cls == "nan":
        assert np.isinf(rep["rad"][5]) and must[5].sum() == c.count - 1 and must_not.sum() >= 0.05 * pairs
    if c.cls == "offset":
        assert must.sum() >= 0.05 * pairs                                  # (tightness there is whatever the norm term leaves)
    if c.cls == "huge":
        assert np.isfinite(R.key_distance(rep["keys"])).all() and np.isfinite(rep["rad"]).all()
        assert (rep["N64"] > R.FLT_MAX).all()                              # ... while every fp32 norm overflows
        assert 0 < must.sum() < pairs


def test_huge_recipe_is_finite_in_the_oracle(oracle):
    """256 rows of 2e19 (1 + 0.02 synth), d = 16, 40 codes drawn from them, 600 iterations: the reference's arithmetic
    trains all four kinds with finite codes and finite winner distances, so the batched engine has to as well"""
    x, xlab, codes, clab = huge_data(16)
    for kind in (LVQ1, OLVQ1, LVQ2, LVQ3):
        want, _, ti, td = oracle.lvq_train(kind, codes, clab, x, xlab, 600, 0.05, winlen=0.3, epsilon=0.1)
        assert np.isfinite(want).all() and np.isfinite(td).all() and (ti >= 0).all(), kind
        if kind != LVQ2:                 # (LVQ2.1 finds no window here: the two nearest rows carry the blob's label)
            assert not np.array_equal(want, codes)


def _toy():
    rs = np.random.RandomState(5)
    x = np.concatenate([rs.standard_normal((20, 4)), 8.0 + rs.standard_normal((20, 4))]).astype(np.float32)
    D = R.pair_distances(x)
    rad = np.full(40, 2.5)
    must = R.must_pairs(D, rad, np.float32(0.05))
    A = D <= 1.06 * 5.0
    A[np.arange(40), np.arange(40)] = False
    return D, must, A


def test_soundness_checker_can_fail():
    D, must, A = _toy()
    R.check_sound(A, must)
    i, j = np.argwhere(must)[7]
    A[i, j] = A[j, i] = False
    with pytest.raises(AssertionError, match="must pairs have no edge"):
        R.check_sound(A, must)


def test_tightness_checker_can_fail():
    D, must, A = _toy()
    rho = np.full(40, 2.5 * 1.06, dtype=np.float32)
    must_not = R.must_not_pairs(D, rho, (D * 0).sum(axis=1), 4, "direct")
    assert must_not.any()
    R.check_tight(A, must_not)
    with pytest.raises(AssertionError, match="separable pairs have an edge"):
        R.check_tight(np.ones((40, 40), dtype=bool), must_not)
    gram = R.must_not_pairs(D, rho, np.full(40, 80.0), 4, "gram")
    with pytest.raises(AssertionError, match="separable pairs have an edge"):
        R.check_tight(np.ones((40, 40), dtype=bool), gram)


def test_layout_and_component_checkers_can_fail():
    D, must, A = _toy()
    adj = R.pack_adj(A)
    assert np.array_equal(R.unpack_adj(adj, 40), A)
    R.check_layout(adj, 40)
    bad = adj.copy()
    bad[3, 1] |= np.uint32(1 << 8)                       # bit 40 of row 3: at or above count
    with pytest.raises(AssertionError):
        R.check_layout(bad, 40)
    bad = adj.copy()
    bad[3, 0] ^= np.uint32(1 << 30)                      # one direction of a pair only
    with pytest.raises(AssertionError, match="symmetric"):
        R.check_layout(bad, 40)
    ncomp, start, comp = R.host_components(A)
    assert ncomp == 2 and start.tolist() == [0, 20, 40] and np.array_equal(comp, np.arange(40))
    R.check_components(A, ncomp, start, comp)
    with pytest.raises(AssertionError, match="component count"):      # one component split in two
        R.check_components(A, 3, np.array([0, 20, 30, 40], dtype=np.int32), comp)
    swapped = comp.copy()
    swapped[[19, 20]] = swapped[[20, 19]]
    with pytest.raises(AssertionError, match="comp_samples"):
        R.check_components(A, ncomp, start, swapped)
    # order: size descending, then root ascending
    B = np.zeros((6, 6), dtype=bool)
    for i, j in ((1, 4), (2, 3), (3, 5)):
        B[i, j] = B[j, i] = True
    ncomp, start, comp = R.host_components(B)
    assert ncomp == 3 and start.tolist() == [0, 3, 5, 6] and comp.tolist() == [2, 3, 5, 1, 4, 0]


# ------------------------------------------------------------------------------------------------ the relation on the GPU
def run_relation(eng, c, data):
    """(plan, what somhip_debug_lvq_relation returned) for the case on `eng`"""
    from som_lvq_pak_amd import engine as E
    cb = E.Codebook(eng, data["codes"], labels=data["clab"])
    ds = E.Dataset(eng, data["x"], mask=data["mask"], labels=data["xlab"])
    try:
        if c.kind == OLVQ1:
            E.lvq_rates_upload(cb, data["talpha"])
        plan = E.lvq_plan(cb, ds, c.kind, c.length, c.alpha, c.alpha_type, c.winlen, c.epsilon, c.start_iter, c.count,
                          c.first, trace=False)
        got = E.lvq_relation(cb, ds, c.kind, c.length, c.alpha, c.alpha_type, c.winlen, c.epsilon, c.start_iter, c.first,
                             c.count)
    finally:
        cb.close()
        ds.close()
    return plan, got


def check_relation(c, rep, got, form):
    """(a) .. (f) of the module docstring; returns (must pairs without an edge, must pairs) for the record"""
    count = c.count
    A = R.unpack_adj(got["adj"], count)
    must = rep["must"]
    print("%s: count %d, must %d, edges %d, must without an edge %d, components %d" % (
        c.name, count, must.sum() // 2, A.sum() // 2, (must & ~A).sum() // 2, got["ncomp"]))
    # (a)
    gk, wk = got["keys"], rep["keys"]
    if c.cls == "nan":                         # a NaN distance is no winner whatever its bits: compare it as that
        none = (wk >> np.uint64(32)) >= np.uint64(R.FLT_MAX_BITS)
        assert ((gk >> np.uint64(32)) >= np.uint64(R.FLT_MAX_BITS))[none].all()
        gk, wk = np.where(none, R.KEY_NONE, gk), np.where(none, R.KEY_NONE, wk)
    assert np.array_equal(gk, wk), ("candidate keys differ at", np.argwhere(gk != wk)[:4].tolist())
    # (b)
    if rep["amax"] is None:
        assert got["amax"] < 0
    else:
        assert np.float32(got["amax"]).view(np.uint32) == np.float32(rep["amax"]).view(np.uint32), (got["amax"], rep["amax"])
    R.check_rho_band(got["rho"], got["xnorm"], rep["rad"], rep["amax"], rep["N64"], c.d)
    # (c), (d)
    R.check_sound(A, must)
    must_not = R.must_not_pairs(rep["D"], got["rho"], got["xnorm"], c.d, form)
    R.check_tight(A, must_not)
    # (e), (f)
    R.check_layout(got["adj"], count)
    R.check_components(A, got["ncomp"], got["start"], got["comp_samples"])
    return must_not


@gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_relation_is_sound_and_no_looser_than_its_slack(eng, c):
    rep = replay(c)
    plan, got = run_relation(eng, c, rep["data"])
    assert plan["engine"] == "batched" and not plan["single"]
    assert plan["pairs"] == c.pairs, plan                                   # (g)
    must_not = check_relation(c, rep, got, c.form)
    pairs = c.count * (c.count - 1)
    if c.plain and pairs:                      # the engine's own rho leaves the tightness check as much to judge
        assert must_not.sum() >= 0.05 * pairs
    if c.cls == "sweep":
        assert must_not[np.arange(0, c.count, 2), np.arange(1, c.count, 2)].sum() >= 8
    if c.cls in ("tiny", "unknown", "huge"):   # rho = +inf: always
        assert np.isposinf(got["rho"]).all() and got["ncomp"] == 1
        assert R.unpack_adj(got["adj"], c.count).sum() == pairs


@gpu
def test_stale_scratch_does_not_leak_into_the_next_batch(eng):
    """A dense batch of 1024 samples leaves its adjacency rows, rho and components in the engine's scratch; a batch of
    65 samples after it comes out as on an engine that never saw the first."""
    from som_lvq_pak_amd import engine as E
    big = Case("dense1024", 32, 1024, cls="unknown", alpha=float("nan"))
    _, g0 = run_relation(eng, big, replay(big)["data"])
    assert g0["ncomp"] == 1 and R.unpack_adj(g0["adj"], 1024).sum() == 1024 * 1023
    for c in (BY_NAME["gram_d32_n65"], BY_NAME["direct_d12_n65"], BY_NAME["masked_d13_n65"]):
        _, g0 = run_relation(eng, big, replay(big)["data"])
        _, after = run_relation(eng, c, replay(c)["data"])
        fresh_eng = E.Engine(0)
        try:
            _, fresh = run_relation(fresh_eng, c, replay(c)["data"])
        finally:
            fresh_eng.close()
        for k in ("keys", "rho", "xnorm", "adj", "start", "comp_samples"):
            assert np.array_equal(after[k].view(np.uint32) if after[k].dtype == np.float32 else after[k],
                                  fresh[k].view(np.uint32) if fresh[k].dtype == np.float32 else fresh[k]), (c.name, k)
        assert after["ncomp"] == fresh["ncomp"]
        check_relation(c, replay(c), after, c.form)


@gpu
def test_both_pair_kernels_on_the_same_input(eng, monkeypatch):
    """SOMHIP_LVQ_PAIRS_VALU=1 sends a d = 32 batch to the direct-form kernel: both kernels are sound and tight on the
    same input, each by its own slack; SOMHIP_LVQ_SERIAL=1 makes the batch one component in iteration order."""
    for name in ("gram_d32_n129", "gram_d32_n1000", "sweep_gram"):
        c = BY_NAME[name]
        rep = replay(c)
        plan, got = run_relation(eng, c, rep["data"])
        assert plan["pairs"] == "mfma"
        check_relation(c, rep, got, "gram")
        monkeypatch.setenv("SOMHIP_LVQ_PAIRS_VALU", "1")
        plan, valu = run_relation(eng, c, rep["data"])
        monkeypatch.delenv("SOMHIP_LVQ_PAIRS_VALU")
        assert plan["pairs"] == "direct"
        check_relation(c, rep, valu, "direct")
        assert np.array_equal(got["rho"].view(np.uint32), valu["rho"].view(np.uint32))
        both = R.unpack_adj(got["adj"], c.count) & R.unpack_adj(valu["adj"], c.count)
        R.check_sound(both, rep["must"])
    c = BY_NAME["gram_d32_n129"]
    monkeypatch.setenv("SOMHIP_LVQ_SERIAL", "1")
    plan, one = run_relation(eng, c, replay(c)["data"])
    monkeypatch.delenv("SOMHIP_LVQ_SERIAL")
    assert plan["single"] and one["ncomp"] == 1 and one["start"].tolist() == [0, c.count]
    assert np.array_equal(one["comp_samples"], np.arange(c.count)) and np.array_equal(one["keys"], replay(c)["keys"])


@gpu
def test_relation_diagnostic_refuses_what_training_would_not_run(eng, monkeypatch):
    from som_lvq_pak_amd import _lib, engine as E
    c = BY_NAME["gram_d32_n65"]
    data = replay(c)["data"]
    cb = E.Codebook(eng, data["codes"], labels=data["clab"])
    ds = E.Dataset(eng, data["x"], labels=data["xlab"])
    bare_cb, bare_ds = E.Codebook(eng, data["codes"]), E.Dataset(eng, data["x"])
    try:
        for count in (0, 1025):
            with pytest.raises(_lib.SomhipError, match="a batch has 1..1024 samples"):
                E.lvq_relation(cb, ds, LVQ1, 100000, 0.05, count=count)
        with pytest.raises(_lib.SomhipError, match="codebook has no labels"):
            E.lvq_relation(bare_cb, ds, LVQ1, 100000, 0.05, count=65)
        with pytest.raises(_lib.SomhipError, match="data has no labels"):
            E.lvq_relation(cb, bare_ds, LVQ1, 100000, 0.05, count=65)
        with pytest.raises(_lib.SomhipError, match="OLVQ1 needs rates"):
            E.lvq_relation(cb, ds, OLVQ1, 100000, 0.05, count=65)
        with pytest.raises(_lib.SomhipError, match="iterations outside schedule"):
            E.lvq_relation(cb, ds, LVQ1, 100, 0.05, start_iter=50, count=65)
        monkeypatch.setenv("SOMHIP_LVQ_ONLINE", "1")
        with pytest.raises(_lib.SomhipError, match="does not run the batched engine"):
            E.lvq_relation(cb, ds, LVQ1, 100000, 0.05, count=65)
        monkeypatch.delenv("SOMHIP_LVQ_ONLINE")
        for count in (0, 1025):
            with pytest.raises(_lib.SomhipError, match="a batch has 1..1024 samples"):
                E.lvq_components(eng, np.zeros((count, R.AW), dtype=np.uint32), count)
    finally:
        for h in (cb, ds, bare_cb, bare_ds):
            h.close()


# ------------------------------------------------------------------------------------------------ components alone
def _path(order):
    n = len(order)
    A = np.zeros((n, n), dtype=bool)
    A[order[:-1], order[1:]] = True
    return A | A.T


def _bitrev(n):
    bits = max(1, (n - 1).bit_length())
    rev = [int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)]
    return np.array([r for r in rev if r < n], dtype=np.int64)


def _graphs(count):
    rs = np.random.RandomState(count)
    ar = np.arange(count)
    out = [("empty", np.zeros((count, count), dtype=bool)), ("complete", ~np.eye(count, dtype=bool))]
    if count > 1:
        out += [("path", _path(ar)), ("path_reversed", _path(ar[::-1])), ("path_bitrev", _path(_bitrev(count))),
                ("path_random", _path(rs.permutation(count)))]
        star = np.zeros((count, count), dtype=bool)
        star[count - 1, :count - 1] = star[:count - 1, count - 1] = True
        out.append(("star_last", star))
        for p in (0.5, 1.0, 2.0):
            Ar = np.triu(rs.random_sample((count, count)) < p / count, 1)
            out.append(("er_%g" % p, Ar | Ar.T))
    if count == 1024:
        two = np.zeros((count, count), dtype=bool)
        two[:512, :512] = two[512:, 512:] = True
        two[ar, ar] = False
        two[100, 900] = two[900, 100] = True
        out.append(("two_cliques_one_edge", two))
        inter = (ar[:, None] % 16 == ar[None, :] % 16) & ~np.eye(count, dtype=bool)
        out.append(("cliques_interleaved", inter))
    return out


COUNTS = (1, 31, 32, 33, 63, 64, 65, 1023, 1024)


@gpu
@pytest.mark.parametrize("count", COUNTS)
def test_components_equal_host_union_find(eng, count):
    from som_lvq_pak_amd import engine as E
    # (stale rows of a dense graph stay in the scratch: the kernel reads its own count only)
    E.lvq_components(eng, R.pack_adj(~np.eye(1024, dtype=bool)), 1024)
    for name, A in _graphs(count):
        ncomp, start, comp = E.lvq_components(eng, R.pack_adj(A), count)
        try:
            R.check_components(A, ncomp, start, comp)
        except AssertionError as err:
            raise AssertionError("%s, count %d: %s" % (name, count, err))
        if name == "empty":
            assert ncomp == count and np.array_equal(comp, np.arange(count))
        if name in ("complete", "path", "path_bitrev", "star_last", "two_cliques_one_edge"):
            assert ncomp == 1 and np.array_equal(comp, np.arange(count))
        if name == "cliques_interleaved":      # equal sizes: the smaller root first
            assert ncomp == 16 and np.array_equal(comp.reshape(16, 64), (np.arange(64)[None, :] * 16 + np.arange(16)[:, None]))
    A = _graphs(count)[-1][1]
    ncomp, start, comp = E.lvq_components(eng, R.pack_adj(A), count, single=True)
    assert ncomp == 1 and start.tolist() == [0, count] and np.array_equal(comp, np.arange(count))


# ------------------------------------------------------------------------------------------------ end to end
@gpu
@pytest.mark.parametrize("kind", (LVQ1, OLVQ1, LVQ2, LVQ3))
def test_huge_values_train_like_the_oracle(eng, oracle, monkeypatch, kind):
    """The huge-value recipe through somhip_lvq_train, as planned and as one serial walk: trace and codebook are the
    oracle's bits.  (The relation test above is the decisive one: with rho = +inf the batch is one component, and a
    graph that lost its edges there could still train right by luck.  It did not: while k_lvq_pair_adj_mfma tested
    "d2 <= ..." on a NaN, the huge_gram batch had none of its 28 617 must edges, 256 components, and this test failed
    for LVQ1, OLVQ1 and LVQ3 in the planned form; with "not (d2 > ...)" no must pair is without an edge.)"""
    from som_lvq_pak_amd import engine as E
    x, xlab, codes, clab = huge_data(16)
    want, wta, wi, wd = oracle.lvq_train(kind, codes, clab, x, xlab, 600, 0.05, winlen=0.3, epsilon=0.1)
    assert np.isfinite(want).all() and np.isfinite(wd).all()
    ds = E.Dataset(eng, x, labels=xlab)
    try:
        for serial in (False, True):
            if serial:
                monkeypatch.setenv("SOMHIP_LVQ_SERIAL", "1")
            cb = E.Codebook(eng, codes, labels=clab)
            plan = E.lvq_plan(cb, ds, kind, 600, 0.05, winlen=0.3, epsilon=0.1)
            assert plan["engine"] == "batched" and plan["single"] == serial and plan["pairs"] == "mfma"
            ta, ti, td = E.lvq_train(cb, ds, kind, 600, 0.05, winlen=0.3, epsilon=0.1)
            got = cb.download()
            cb.close()
            if serial:
                monkeypatch.delenv("SOMHIP_LVQ_SERIAL")
            assert np.array_equal(ti, wi), (kind, serial, np.flatnonzero(ti != wi)[:4])
            assert np.array_equal(td.view(np.uint32), wd.view(np.uint32)), (kind, serial)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, serial)
            if kind == OLVQ1:
                assert np.array_equal(ta.view(np.uint32), wta.view(np.uint32))
    finally:
        ds.close()
