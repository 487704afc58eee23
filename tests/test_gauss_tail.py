"""The gaussian rate's four cases, met by design in every kernel that forms the rate.

kernels/gauss_rate.hpp decides per (sample, unit) between the short form, the exact zero (y <= -104), the library chain
because the float would be subnormal (-104 < y < -87) and the library chain because e^y lies next to the midpoint of
two floats (y = (double)(-dd * dd) / (2 radius^2)).  On the host all four are checked against glibc
(tests/helpers/gauss_rate_check.c); on the GPU the device build has parts of its own -- the coefficients held in scalar
registers, v_ldexp_f64, the non-inlined gaussian_alpha_call under a divergent exec mask in k_som_update_gauss_h (at a
forced 8 waves per SIMD) and k_mapset_train -- and the other kernels form the same float with the library chain alone.

One schedule is used for every case: 4096 iterations from radius 6.0 to 1, alpha 0.05, linear, on a 16 x 16 hexa and a
20 x 13 rect map, 4096 rows of the seeded mixture, randinit from the oracle.  Before any GPU work every (iteration,
unit) pair of the oracle's run is classified in NumPy as the header classifies it (the radius of som_replay.som_radius,
the lattice distance of som_replay.lattice_dist, y by one IEEE division: the correctly rounded quotient, which is what
the header's Markstein sequence gives), and the run must hold at least MIN_MID near-midpoint pairs, MIN_WINDOW window
pairs and MIN_ZERO zero pairs.  Near-midpoint is counted with a margin of 0x0F00 around 2^28 in the low 29 bits of
np.exp(y)'s double, inside the header's 0x1000: a pair counted here is declined by the short form whatever last-place
difference there is between NumPy's exp and the header's polynomial.  These are conditions on the inputs; they are
checked without a GPU too (test_every_run_meets_every_case), so a change of seed, shape or schedule that loses a case
fails there.  The runs whose oracle differs (batch 500, d = 48, the wrapped rows, the mask, batch 1) are classified on
their own.

Then the same inputs go through each kernel (RUNS): the plan of every batch is the witness of the apply kernel, the
timing tables of k_som_online_step and k_mapset_train, and codebook bits, winner trace and trace distances equal the
oracle's som_train with the same batch size bit for bit.

A batch of 512 of 4096 rows cannot wrap the data set in every batch, so the wrapped k_som_update_gauss_s run takes the
first 520 rows as its data set and starts at row 519: the batches start at rows 519, 511, ..., 463 and every one of
them wraps.

The final codebook is a weak witness of a single rate: a rate of the subnormal window changes no code of ordinary
size, and a last-place error of a rate near a midpoint is mostly rounded away by the updates behind it.
test_rates_read_back therefore reads the rates themselves.  The last four dims of every code are 0 and of every row 1,
so one iteration leaves c + a * (1 - c) = a, the unit's rate bit for bit, in those dims -- subnormal rates and exact
zeros included.  The iterations are chosen on the CPU: for rows that win at a corner, at the far corner and in the
middle, the first (up to six) iterations of the schedule whose radius puts some unit of the map next to a midpoint, and two late
ones for the window and the zero; each is run alone (start_iter = it, count = 1) through every kernel and compared with
som_replay's float32 replay, which is the batch oracle's arithmetic.

Update mode gemm is out of scope: its rate is exp2f by design, its tolerance is relative to the map's scale
(test_gemm_replay), and the rates of the tail lie far below that.  Needs an MI355X:  pytest -m gpu."""
import numpy as np
import pytest

from conftest import synth
from helpers import som_replay

HEXA, RECT, GAUSS = 3, 4, 2
LENGTH, ALPHA, RADIUS, N_ROWS, SEED = 4096, 0.05, 6.0, 4096, 1
MIN_MID, MIN_WINDOW, MIN_ZERO = 8, 300, 300
MAPS = {"hexa16x16": (16, 16, HEXA), "rect20x13": (20, 13, RECT)}


class Run:
    def __init__(self, name, apply, d=32, B=512, rows=N_ROWS, first=0, masked=False, env=None, how="batch"):
        self.name, self.apply, self.d, self.B, self.rows, self.first = name, apply, d, B, rows, first
        self.masked, self.env, self.how = masked, env or {}, how

    def oracle_key(self, m):
        return (m, self.d, self.B, self.rows, self.first, self.masked)


RUNS = [
    Run("gauss_h", "gauss_h"),                                   # the run of every batch in one piece
    Run("gauss_h_partial_tile", "gauss_h", B=500),               # lists of 7 x 64 + 52 entries
    Run("gauss_s_d48", "gauss_s", d=48),                         # d4 % 8 != 0
    Run("gauss_s_wrap", "gauss_s", rows=520, first=519),         # every batch wraps the data set
    Run("run_lds", "run", env={"SOMHIP_UPD_LDS": "1"}),          # the gaussian form of the LDS-tile kernel
    Run("run_lds_masked", "run", masked=True, env={"SOMHIP_UPD_LDS": "1"}),
    Run("online", None, B=1, how="online"),                      # k_som_online_step
    Run("mapset", None, B=1, how="mapset"),                      # k_mapset_train<GAUSS>, two maps of the same rows
]
CASES = [(m, r) for m in MAPS for r in RUNS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def classify(topol, xdim, ydim, winners, length, radius):
    """{case: (iteration, unit) pairs} of a run with these winners, as gauss_rate.hpp decides them"""
    tx, ty = np.arange(xdim * ydim) % xdim, np.arange(xdim * ydim) // xdim
    dist = {}
    n = {"short": 0, "zero": 0, "window": 0, "mid": 0}
    for j in range(length):
        w = int(winners[j])
        if w < 0:                                                # a sample without a winner teaches nothing
            continue
        if w not in dist:
            dd = som_replay.lattice_dist(topol, w % xdim, w // xdim, tx, ty)
            dist[w] = (-(dd * dd)).astype(np.float64)            # the float product, then the double
        r = float(som_replay.som_radius(j, length, radius))
        y = dist[w] / (2.0 * r * r)
        zero = y <= -104.0
        window = (y > -104.0) & (y < -87.0)
        low = (np.exp(y).view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64)
        mid = ~zero & ~window & (np.abs(low - 0x10000000) <= 0x0F00)
        n["zero"] += int(zero.sum())
        n["window"] += int(window.sum())
        n["mid"] += int(mid.sum())
        n["short"] += int((~zero & ~window & ~mid).sum())
    return n


_REFERENCE = {}


def reference(oracle, m, run):
    """the oracle's run of map m with the inputs of `run`, and its classification: made once, shared, left unchanged"""
    key = run.oracle_key(m)
    if key not in _REFERENCE:
        xdim, ydim, topol = MAPS[m]
        x, _ = synth(SEED + run.d, N_ROWS, run.d)
        ini = oracle.randinit(x, xdim, ydim, SEED)
        x = x[:run.rows]
        mask = (np.random.RandomState(SEED + 7).random_sample(x.shape) < 0.2).astype(np.uint8) if run.masked else None
        # the oracle reads its rows from row 0 on: hand it the rows in the run's order
        xo = np.roll(x, -run.first, axis=0)
        mo = None if mask is None else np.roll(mask, -run.first, axis=0)
        oc, oi, od = oracle.som_train(ini, xdim, ydim, topol, GAUSS, xo, LENGTH, ALPHA, RADIUS, mask=mo, batch=run.B)
        ref = dict(x=x, mask=mask, ini=ini, codes=oc, ti=oi, td=od, counts=classify(topol, xdim, ydim, oi, LENGTH, RADIUS))
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def check_counts(ref):
    c = ref["counts"]
    assert c["mid"] >= MIN_MID and c["window"] >= MIN_WINDOW and c["zero"] >= MIN_ZERO, c
    assert c["short"] > 1000 * c["mid"], c


@pytest.mark.parametrize("m,run", CASES, ids=["%s-%s" % (m, r.name) for m, r in CASES])
def test_every_run_meets_every_case(oracle, m, run):
    """no GPU: the oracle's run alone forms every case of the rate often enough"""
    check_counts(reference(oracle, m, run))


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


def check_result(ref, got, ti, td, what=""):
    assert np.array_equal(ti, ref["ti"]), what
    assert np.array_equal(bits(td), bits(ref["td"])), what
    assert np.array_equal(bits(got), bits(ref["codes"])), what


@pytest.mark.gpu
@pytest.mark.parametrize("m,run", CASES, ids=["%s-%s" % (m, r.name) for m, r in CASES])
def test_gaussian_tail(eng, E, oracle, monkeypatch, m, run):
    xdim, ydim, topol = MAPS[m]
    ref = reference(oracle, m, run)
    check_counts(ref)                                            # before the first GPU call
    for k, v in run.env.items():
        monkeypatch.setenv(k, v)
    ds = E.Dataset(eng, ref["x"], mask=ref["mask"])
    try:
        if run.how == "mapset":
            ms = E.MapSet(eng, np.stack([ref["ini"], ref["ini"]]), topol, GAUSS, xdim, ydim)
            eng.timing(True)
            try:
                before = eng.mapset_timing()["k_mapset_train"][0]
                ti, td = ms.train(ds, LENGTH, ALPHA, RADIUS, trace=True)
                assert eng.mapset_timing()["k_mapset_train"][0] > before
            finally:
                eng.timing(False)
            got = ms.download()
            ms.close()
            for k in range(2):
                check_result(ref, got[k], ti[k], td[k], "map %d" % k)
            return
        cb = E.Codebook(eng, ref["ini"], topol, GAUSS, xdim, ydim)
        if run.how == "online":
            ti, td = E.som_train(cb, ds, LENGTH, ALPHA, RADIUS, batch=1)           # whole chunks from the captured graph
            check_result(ref, cb.download(), ti, td, "graph")
            cb.upload(ref["ini"])
            eng.timing(True)
            eng.timing_reset()
            try:
                ti, td = E.som_train(cb, ds, LENGTH, ALPHA, RADIUS, batch=1)
                table = eng.timing_table()
            finally:
                eng.timing(False)
            assert table["k_som_online_step"][0] >= LENGTH
            assert table["k_som_update_run"][0] == 0 and table["k_som_members"][0] == 0
        else:
            for it in range(0, LENGTH, run.B):                   # the plan of every batch
                plan = E.update_plan(cb, ds, LENGTH, ALPHA, RADIUS, min(run.B, LENGTH - it), start_iter=it,
                                     data_first=(run.first + it) % run.rows)
                assert plan["apply"] == run.apply, (it, plan)
            eng.timing(True)
            eng.timing_reset()
            try:
                ti, td = E.som_train(cb, ds, LENGTH, ALPHA, RADIUS, batch=run.B, data_first=run.first)
                table = eng.timing_table()
            finally:
                eng.timing(False)
            assert table["k_som_update_run"][0] == -(-LENGTH // run.B)      # (every gaussian apply kernel is timed under this name)
            assert table["k_som_online_step"][0] == 0 and table["k_som_update_gemm"][0] == 0
        check_result(ref, cb.download(), ti, td)
        cb.close()
    finally:
        ds.close()


# ------------------------------------------------------------------------------------------------ the rates read back
PROBE = 4                                                        # dims that hold 0 in every code and 1 in every row
N_MID, LATE = 6, (LENGTH - 60, LENGTH - 1)
STEP_KERNELS = [("gauss_h", 32, {}), ("gauss_s", 48, {}), ("run", 32, {"SOMHIP_UPD_LDS": "1"}), ("online", 32, {}),
                ("mapset", 32, {})]
_PROBES = {}


def pair_cases(neg, radius):
    """(zero, window, mid) masks of the pairs with the double products `neg` = -dd * dd at this radius"""
    y = neg / (2.0 * float(radius) * float(radius))
    zero = y <= -104.0
    window = (y > -104.0) & (y < -87.0)
    low = (np.exp(y).view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64)
    return zero, window, ~zero & ~window & (np.abs(low - 0x10000000) <= 0x0F00)


def probes(oracle, m, d):
    """codes and rows with the probe dims, and per chosen (iteration, row): the replayed codebook and the pairs' cases"""
    if (m, d) not in _PROBES:
        xdim, ydim, topol = MAPS[m]
        units = xdim * ydim
        x, _ = synth(SEED + d, N_ROWS, d)
        codes = oracle.randinit(x, xdim, ydim, SEED)
        codes[:, d - PROBE:] = 0.0
        at = [0, units - 1, (ydim // 2) * xdim + xdim // 2]      # the rows: copies of these units, so they win there
        rows = codes[at].copy()
        rows[:, d - PROBE:] = 1.0
        wi, _, _ = oracle.winners(codes, rows)
        assert list(wi[:, 0]) == at
        tx, ty = np.arange(units) % xdim, np.arange(units) // xdim
        steps = []
        for r, w in enumerate(at):
            dd = som_replay.lattice_dist(topol, w % xdim, w // xdim, tx, ty)
            neg = (-(dd * dd)).astype(np.float64)
            vals = np.unique(neg)
            mids = [it for it in range(LENGTH) if pair_cases(vals, som_replay.som_radius(it, LENGTH, RADIUS))[2].any()]
            for it in mids[:N_MID] + list(LATE):
                zero, window, mid = pair_cases(neg, som_replay.som_radius(it, LENGTH, RADIUS))
                want = som_replay.replay(codes, xdim, ydim, topol, GAUSS, rows, LENGTH, ALPHA, RADIUS, [w], start_iter=it,
                                         count=1, data_first=r).codes
                steps.append(dict(it=it, row=r, winner=w, want=want, zero=int(zero.sum()), window=int(window.sum()),
                                  mid=int(mid.sum())))
        _PROBES[m, d] = dict(codes=codes, rows=rows, steps=steps)
    return _PROBES[m, d]


def check_probes(p, d):
    """conditions on the inputs: the chosen iterations form every case, and the probe dims hold the rates"""
    steps = p["steps"]
    assert sum(s["mid"] > 0 for s in steps) >= MIN_MID and sum(s["mid"] for s in steps) >= MIN_MID
    assert sum(s["window"] for s in steps) >= 20 and sum(s["zero"] for s in steps) >= 20
    rate = np.concatenate([s["want"][:, d - 1] for s in steps])
    assert ((rate > 0) & (rate < np.finfo(np.float32).tiny)).sum() >= 20        # subnormal rates, read back as they are
    assert (rate == 0).sum() >= 20 and (rate > 1e-3).sum() >= 20
    for s in steps:
        assert all(np.array_equal(bits(s["want"][:, d - 1]), bits(s["want"][:, d - 1 - k])) for k in range(PROBE))


@pytest.mark.parametrize("m", list(MAPS))
@pytest.mark.parametrize("d", [32, 48])
def test_the_probe_iterations_form_every_case(oracle, m, d):
    """no GPU"""
    check_probes(probes(oracle, m, d), d)


@pytest.mark.gpu
@pytest.mark.parametrize("m", list(MAPS))
@pytest.mark.parametrize("kernel,d,env", STEP_KERNELS, ids=[k for k, _, _ in STEP_KERNELS])
def test_rates_read_back(eng, E, oracle, monkeypatch, m, kernel, d, env):
    xdim, ydim, topol = MAPS[m]
    p = probes(oracle, m, d)
    check_probes(p, d)                                           # before the first GPU call
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ds = E.Dataset(eng, p["rows"])
    if kernel == "mapset":
        both = np.stack([p["codes"], p["codes"]])
        ms = E.MapSet(eng, both, topol, GAUSS, xdim, ydim)
    else:
        cb = E.Codebook(eng, p["codes"], topol, GAUSS, xdim, ydim)
    try:
        for s in p["steps"]:
            what = (s["it"], s["row"])
            if kernel == "mapset":
                ms.upload(both)
                ti, _ = ms.train(ds, LENGTH, ALPHA, RADIUS, start_iter=s["it"], count=1, data_first=s["row"], trace=True)
                got = ms.download()
                assert ti[0, 0] == s["winner"] and ti[1, 0] == s["winner"], what
                assert np.array_equal(bits(got[1]), bits(got[0])), what
                got = got[0]
            else:
                batch = 1 if kernel == "online" else 512
                if batch > 1:
                    plan = E.update_plan(cb, ds, LENGTH, ALPHA, RADIUS, 1, start_iter=s["it"], data_first=s["row"])
                    assert plan["apply"] == kernel, (what, plan)
                cb.upload(p["codes"])
                ti, _ = E.som_train(cb, ds, LENGTH, ALPHA, RADIUS, batch=batch, start_iter=s["it"], count=1,
                                    data_first=s["row"])
                got = cb.download()
                assert ti[0] == s["winner"], what
            bad = np.nonzero((bits(got) != bits(s["want"])).any(axis=1))[0]
            assert len(bad) == 0, (what, bad[:8], got[bad[:8], d - 1], s["want"][bad[:8], d - 1])
    finally:
        (ms if kernel == "mapset" else cb).close()
        ds.close()
