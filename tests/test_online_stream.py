"""The two one-launch-per-iteration kernels at the edges of their row stream, bit for bit against the CPU oracle.

online_stream (kernels/som_online.hpp) is the loop k_som_online_step (K3: som_train with batch 1) and
k_lvq_online_step (K5) run over a code row: two register buffers of 8 float4 chunks, a main loop for d4 >= 16 with a
prefetch clamped at d4 - 1, a tail loop for d4 % 16 chunks, scalar loads with a bound for dim % 4 != 0, and the
compile-time variants MASKED / UPD / SEARCH.  The cases below put d4 on both sides of 16 and 32, dims on every
remainder of 4, maps on both sides of a wave and of a workgroup, runs through the captured graph of 1024 launches and
its cache, and K5 both where somhip_lvq_train takes it by itself (rows too wide for the batched engine, a labelled map
stored as 8x8 patches) and forced by SOMHIP_LVQ_ONLINE=1.

The witness is oracle.som_train(batch=1) / oracle.lvq_train; masked LVQ, which the oracle's loop does not take, is
replayed from the oracle's primitives (tests/lvq_masked_replay.py, itself pinned to oracle.lvq_train on the CPU below).
Winner trace, distance trace, codebook and OLVQ1 rates: equal indices, equal bit patterns, no tolerance anywhere.
The data hold NaN and 1e30 under the mask, so a kernel that reads a masked component shows."""
import numpy as np
import pytest

from conftest import synth
from lvq_masked_replay import lvq_replay

gpu = pytest.mark.gpu
HEXA, RECT, BUBBLE, GAUSSIAN = 3, 4, 1, 2
CHUNK = 1024                    # ONLINE_CHUNK of csrc/somhip.hip: launches per captured graph


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def _mask(seed, m, d, frac=0.15):
    rs = np.random.RandomState(seed)
    mask = (rs.random_sample((m, d)) < frac).astype(np.uint8)
    mask[mask.all(axis=1), 0] = 0                            # no fully masked row unless a case makes one
    return mask


def _garbage(x, mask, seed):
    """the rows as the device gets them: NaN and 1e30 where the mask is set"""
    if mask is None:
        return x
    rs = np.random.RandomState(seed)
    xs = x.copy()
    xs[mask != 0] = np.where(rs.random_sample(int((mask != 0).sum())) < 0.5, np.nan, 1e30).astype(np.float32)
    return xs


# =========================================================================== K3: k_som_online_step
def _som_check(eng, E, oracle, xd, yd, topol, neigh, x, mask, length, alpha=0.07, radius=8.0, ini=None, calls=None,
               weight=None, fixed=None, alpha_type=1, data_first=0, cb=None, ds=None):
    """one schedule of `length` iterations on the engine, in the calls [(start_iter, count), ...], against one oracle run;
    the oracle sees the data rolled by data_first and clean values, the engine garbage under the mask"""
    m = x.shape[0]
    ini = oracle.randinit(x, xd, yd, 3) if ini is None else ini

    def roll(a):
        return None if a is None else np.roll(a, -data_first, axis=0)

    oc, oi, od = oracle.som_train(ini, xd, yd, topol, neigh, roll(x), length, alpha, radius, alpha_type=alpha_type,
                                  weight=roll(weight), fixed_xy=roll(fixed), mask=roll(mask),
                                  fixed_on=int(fixed is not None), weights_on=int(weight is not None))
    own_cb, own_ds = cb is None, ds is None
    cb = E.Codebook(eng, ini, topol, neigh, xd, yd) if own_cb else cb
    ds = E.Dataset(eng, _garbage(x, mask, 11), mask=mask, weight=weight, fixed_xy=fixed) if own_ds else ds
    try:
        ti, td = [], []
        for start, count in calls or [(0, length)]:
            i, d = E.som_train(cb, ds, length, alpha, radius, alpha_type=alpha_type, use_fixed=int(fixed is not None),
                               use_weights=int(weight is not None), batch=1, start_iter=start, count=count,
                               data_first=(data_first + start) % m)
            ti.append(i)
            td.append(d)
        ti, td = np.concatenate(ti), np.concatenate(td)
        got = cb.download()
    finally:
        if own_cb:
            cb.close()
        if own_ds:
            ds.close()
    assert np.array_equal(ti, oi), np.flatnonzero(ti != oi)[:5]
    assert np.array_equal(bits(td), bits(od)), np.flatnonzero(bits(td) != bits(od))[:5]
    assert np.array_equal(bits(got), bits(oc)), np.argwhere(bits(got) != bits(oc))[:5]
    assert not np.array_equal(bits(oc), bits(ini))           # the run taught something
    return oi


# ---- 1. stream edges: d4 on both sides of one and two trips of the main loop, vector and scalar loads
#      d4 = 15: tail only | 16: one trip, no tail | 17: one trip + 1 tail chunk | 31: one trip + 15 | 32: two trips | 33
EDGE_DIMS = [60, 59, 64, 62, 68, 65, 124, 123, 128, 126, 132, 129]      # 4 d4, then 4 d4 - 1 | - 2 | - 3 | - 1 | - 2 | - 3


assert sorted({(d + 3) // 4 for d in EDGE_DIMS}) == [15, 16, 17, 31, 32, 33] and {d % 4 for d in EDGE_DIMS} == {0, 1, 2, 3}
assert all(4 * d4 in EDGE_DIMS for d4 in (15, 16, 17, 31, 32, 33))


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN], ids=["bubble", "gaussian"])
@pytest.mark.parametrize("dim", EDGE_DIMS)
def test_k3_stream_edges(eng, E, oracle, dim, neigh, masked):
    """13 x 5 = 65 units: the second wave has one live lane.  Radius 8 -> 1: early iterations update every wave, late
    ones only the winner's, so the other wave runs the search-only variant."""
    x, _ = synth(1000 + dim, 150, dim)
    mask = _mask(dim, 150, dim) if masked else None
    _som_check(eng, E, oracle, 13, 5, HEXA, neigh, x, mask, 300)


# ---- 2. map shapes
MAPS = [(9, 7), (8, 8), (16, 16), (20, 13), (24, 16)]       # 63 | 64 patch | 256 patch, one workgroup | 260: 4 + 1 waves | 384 patch


@gpu
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN], ids=["bubble", "gaussian"])
@pytest.mark.parametrize("topol", [HEXA, RECT], ids=["hexa", "rect"])
@pytest.mark.parametrize("dim", [68, 67])
@pytest.mark.parametrize("xd,yd", MAPS)
def test_k3_map_shapes(eng, E, oracle, xd, yd, dim, topol, neigh):
    x, _ = synth(2000 + xd + dim, 150, dim)
    mask = _mask(xd * yd, 150, dim) if dim == 67 else None
    _som_check(eng, E, oracle, xd, yd, topol, neigh, x, mask, 300)


# ---- 3. semantics at a pipelined, ragged dim
def _sem_case(what):
    m = {"single_row": 1, "short_data": 37}.get(what, 150)
    x, _ = synth(3000, 150, 67)
    x = x[:m].copy()
    mask = _mask(67, m, 67)
    kw = {}
    rs = np.random.RandomState(31)
    if what in ("all_masked", "everything"):
        mask[[0, 70, 71, 149]] = 1               # iteration 0, two in a row, the last; 149 -> 0 is a second pair
    if what in ("fixed", "everything"):
        fixed = np.full((m, 2), -1, dtype=np.int16)
        for r in rs.choice(m, 24, replace=False):
            fixed[r] = (rs.randint(0, 13), rs.randint(0, 5))
        fixed[0] = (4, 2); fixed[149] = (12, 4)                                  # first and last iteration
        fixed[5] = (13, 2); fixed[6] = (3, 5); fixed[7] = (40, 40); fixed[8] = (200, 300); fixed[9] = (14, 6)
        if what == "everything":
            fixed[70] = (6, 2)                  # a fixed point on a fully masked sample: an update that changes nothing
        kw["fixed"] = fixed
    if what in ("weights", "everything"):
        kw["weight"] = rs.randint(0, 4, m).astype(np.int16)
        assert (kw["weight"] == 0).any() and (kw["weight"] > 1).any()
    if what == "inverse_t":
        kw["alpha_type"] = 2
    if what == "data_first":
        kw["data_first"] = 41
    return x, mask, kw


@gpu
@pytest.mark.parametrize("neigh", [BUBBLE, GAUSSIAN], ids=["bubble", "gaussian"])
@pytest.mark.parametrize("what", ["all_masked", "fixed", "weights", "inverse_t", "single_row", "short_data", "data_first",
                                  "everything"])
def test_k3_semantics_at_dim_67(eng, E, oracle, what, neigh):
    x, mask, kw = _sem_case(what)
    ini = oracle.randinit(synth(3000, 150, 67)[0], 13, 5, 3)
    oi = _som_check(eng, E, oracle, 13, 5, HEXA, neigh, x, mask, 300, ini=ini, **kw)
    if what == "all_masked":
        assert np.array_equal(np.flatnonzero(oi == -2), [0, 70, 71, 149, 150, 220, 221, 299])
    if what in ("fixed", "everything"):
        assert (oi == -3).sum() >= 40 and oi[0] == -3 and oi[299] == -3


# ---- 4. graph replay and its cache
def _graph_case():
    x, _ = synth(4000, 150, 67)
    return x, _mask(4, 150, 67)


GRAPH_LEN = 2 * CHUNK + 77


@gpu
@pytest.mark.parametrize("calls", [[(0, CHUNK)], [(0, CHUNK + 1)], [(0, GRAPH_LEN)],
                                   [(0, 1000), (1000, 1100), (2100, GRAPH_LEN - 2100)]],
                         ids=["1024", "1025", "2125", "1000+1100+25"])
def test_k3_graph_replay(eng, E, oracle, calls):
    """whole chunks are replayed from the captured graph, the rest of a call is launched one by one: 1024 = one replay,
    1025 = replay + 1, 2125 = two replays + 77; then 1000 launches, one replay + 76 from inside a chunk, 25 launches"""
    x, mask = _graph_case()
    _som_check(eng, E, oracle, 13, 5, HEXA, GAUSSIAN, x, mask, sum(c for _, c in calls), calls=calls)


@gpu
def test_k3_timed_run_takes_no_graph_and_gives_the_same_bits(eng, E, oracle):
    x, mask = _graph_case()
    eng.timing(True)
    eng.timing_reset()
    try:
        _som_check(eng, E, oracle, 13, 5, HEXA, GAUSSIAN, x, mask, GRAPH_LEN)
        launches = eng.timing_table()["k_som_online_step"][0]
    finally:
        eng.timing(False)
    assert launches == GRAPH_LEN + 1                         # every iteration a timed launch of its own, + the flush


@gpu
def test_k3_cached_graph_is_not_replayed_for_another_codebook_or_data_set(E, oracle, capsys):
    """An engine keeps the graph of one chunk and replays it while the launches' arguments stay the same.  After a graph
    is cached: another codebook of the same n and d but other xdim, another data set of the same shape without a mask,
    a codebook of the other lattice -- each trained for more than a chunk, each against its own oracle run.  Whether
    the allocator handed the old addresses out again (the case in which only the key's other fields tell the runs
    apart) is printed."""
    eng = E.Engine(0)
    try:
        x, mask = _graph_case()
        x2, _ = synth(4001, 150, 67)
        length = CHUNK + 100
        ini = oracle.randinit(x, 13, 5, 3)
        ini2 = oracle.randinit(x2, 5, 13, 8)
        cb = E.Codebook(eng, ini, HEXA, GAUSSIAN, 13, 5)
        ds = E.Dataset(eng, _garbage(x, mask, 11), mask=mask)
        _som_check(eng, E, oracle, 13, 5, HEXA, GAUSSIAN, x, mask, length, ini=ini, cb=cb, ds=ds)      # caches the graph
        p0 = E.device_ptrs(cb, ds)
        # 1. other rows, other xdim, same n and d
        cb.close()
        cb = E.Codebook(eng, ini2, HEXA, GAUSSIAN, 5, 13)
        p1 = E.device_ptrs(cb, ds)
        _som_check(eng, E, oracle, 5, 13, HEXA, GAUSSIAN, x, mask, length, ini=ini2, cb=cb, ds=ds)
        # 2. other data of the same shape, no mask; the codebook goes on from where it is
        ds.close()
        ds = E.Dataset(eng, x2)
        p2 = E.device_ptrs(cb, ds)
        _som_check(eng, E, oracle, 5, 13, HEXA, GAUSSIAN, x2, None, length, ini=cb.download(), cb=cb, ds=ds)
        # 3. the first shape on the other lattice
        cb.close()
        cb = E.Codebook(eng, ini, RECT, GAUSSIAN, 13, 5)
        p3 = E.device_ptrs(cb, ds)
        _som_check(eng, E, oracle, 13, 5, RECT, GAUSSIAN, x2, None, length, ini=ini, cb=cb, ds=ds)
        # ... and the first pair once more: a graph made for run 3 must not serve it either
        cb.close(); ds.close()
        cb = E.Codebook(eng, ini, HEXA, GAUSSIAN, 13, 5)
        ds = E.Dataset(eng, _garbage(x, mask, 11), mask=mask)
        p4 = E.device_ptrs(cb, ds)
        _som_check(eng, E, oracle, 13, 5, HEXA, GAUSSIAN, x, mask, length, ini=ini, cb=cb, ds=ds)
        with capsys.disabled():
            print("\n[online graph cache] same addresses as the run before: 1 tiles %s | 2 rows %s | 3 tiles %s | "
                  "4 tiles %s rows %s mask %s" % (p1[0] == p0[0], p2[1] == p1[1], p3[0] == p2[0], p4[0] == p3[0],
                                                  p4[1] == p3[1], p4[2] == p0[2]))
    finally:
        eng.close()


# =========================================================================== K5: k_lvq_online_step
KINDS = [1, 2, 3, 4]                                        # LVQ1, OLVQ1, LVQ2.1, LVQ3


def _lvq_kw(kind):
    kw = {"winlen": 0.25} if kind >= 3 else {}
    if kind == 4:
        kw["epsilon"] = 0.2
    return kw


def _lvq_case(seed, n, d, m):
    """three close blobs with the labels mixed inside them: the two nearest rows often differ in label and lie at nearly
    the same distance, so every rule of the four algorithms fires; codes are data rows plus a little noise"""
    x, _ = synth(seed, m, d, k=3, spread=0.5)
    rs = np.random.RandomState(seed + 1)
    lab = rs.randint(1, 4, m).astype(np.int32)
    pick = rs.choice(m, n, replace=False) if n <= m else rs.randint(0, m, n)
    codes = (x[pick] + 0.05 * rs.standard_normal((n, d))).astype(np.float32)
    # (more codes than rows: a row's noisy copies are each other's nearest, so they get labels of their own)
    clab = lab[pick].copy() if n <= m else rs.randint(1, 4, n).astype(np.int32)
    return codes, clab, x, lab


def _lvq_check(eng, E, kind, codes, clab, x, lab, length, want, mask=None, online=True, grid=None, cut=None):
    """the run in two calls (start_iter and the returned rates carry it over) against `want` = (codes, rates, trace
    index, trace distance) of one whole run"""
    oc, ol, oi, od = want
    alpha = 0.3 if kind == 2 else 0.05
    kw = _lvq_kw(kind)
    cb = (E.Codebook(eng, codes, HEXA, BUBBLE, grid[0], grid[1], labels=clab) if grid
          else E.Codebook(eng, codes, labels=clab))
    ds = E.Dataset(eng, _garbage(x, mask, 13), mask=mask, labels=lab)
    try:
        plan = E.lvq_plan(cb, ds, kind, length, alpha, **kw)
        assert plan["engine"] == ("online" if online else "batched"), plan
        before = eng.lvq_stats()
        cut = length // 3 + 1 if cut is None else cut
        tal, t1, d1 = E.lvq_train(cb, ds, kind, length, alpha, count=cut, **kw)
        tal, t2, d2 = E.lvq_train(cb, ds, kind, length, alpha, start_iter=cut, talpha=tal, **kw)
        after = eng.lvq_stats()
        got = cb.download()
    finally:
        cb.close()
        ds.close()
    assert after["samples"] == before["samples"]             # the batched engine ran nothing
    ti, td = np.concatenate([t1, t2]), np.concatenate([d1, d2])
    assert np.array_equal(ti, oi), np.flatnonzero(ti != oi)[:5]
    assert np.array_equal(bits(td), bits(od)), np.flatnonzero(bits(td) != bits(od))[:5]
    assert np.array_equal(bits(got), bits(oc)), np.argwhere(bits(got) != bits(oc))[:5]
    if kind == 2:
        assert np.array_equal(bits(tal), bits(ol))
    assert not np.array_equal(bits(oc), bits(codes))         # the run corrected something


def _oracle_lvq(oracle, kind, codes, clab, x, lab, length):
    return oracle.lvq_train(kind, codes, clab, x, lab, length, 0.3 if kind == 2 else 0.05, **_lvq_kw(kind))


# ---- 5. where somhip_lvq_train takes K5 by itself
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [2052, 2049])
def test_k5_rows_too_wide_for_the_batched_engine(eng, E, oracle, monkeypatch, dim, kind):
    """d4 = 513 > LVQ_BT: 32 trips of the main loop and one tail chunk, whole (2052) and with one component (2049)"""
    monkeypatch.delenv("SOMHIP_LVQ_ONLINE", raising=False)
    codes, clab, x, lab = _lvq_case(5000 + dim, 70, dim, 200)
    _lvq_check(eng, E, kind, codes, clab, x, lab, 400, _oracle_lvq(oracle, kind, codes, clab, x, lab, 400))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [20, 68])
def test_k5_labelled_map_stored_as_patches(eng, E, oracle, monkeypatch, dim, kind):
    """a labelled 16 x 8 map keeps its rows as 8x8 patches of units: labels, rates and the trace are in unit order"""
    monkeypatch.delenv("SOMHIP_LVQ_ONLINE", raising=False)
    codes, clab, x, lab = _lvq_case(5100 + dim, 128, dim, 200)
    _lvq_check(eng, E, kind, codes, clab, x, lab, 400, _oracle_lvq(oracle, kind, codes, clab, x, lab, 400), grid=(16, 8))


# ---- 6. K5 forced
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [70, 300, 1030])               # 1, 2 and 5 workgroups: the merge of prev_part over prev_nblk
@pytest.mark.parametrize("dim", [61, 64, 65, 68, 125, 132])
def test_k5_forced_unmasked(eng, E, oracle, monkeypatch, dim, n, kind):
    monkeypatch.setenv("SOMHIP_LVQ_ONLINE", "1")
    codes, clab, x, lab = _lvq_case(6000 + dim + n, n, dim, 240)
    _lvq_check(eng, E, kind, codes, clab, x, lab, 300, _oracle_lvq(oracle, kind, codes, clab, x, lab, 300))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_k5_forced_ties(eng, E, oracle, monkeypatch, kind):
    """pairs of identical code rows with different labels, each next to a sample: one winner takes the earlier row
    (find_winner_euc, lvq_pak.c:79), two winners list the later row first (find_winner_knn, lvq_pak.c:197: the ~tag of
    the keys).  The twins sit in one wave, in two waves of a workgroup and in two workgroups."""
    monkeypatch.setenv("SOMHIP_LVQ_ONLINE", "1")
    codes, clab, x, lab = _lvq_case(6500, 300, 67, 240)
    pairs = [(3, 40), (5, 100), (7, 290), (64, 255), (256, 299), (10, 11)]
    for j, (a, b) in enumerate(pairs):
        codes[b] = codes[a]
        clab[a], clab[b] = 1, 2
        for s in (2 * j, 2 * j + 1):                         # two samples at the twins, one of each label
            x[s] = codes[a] + np.float32(0.001) * x[s]
            lab[s] = 1 + s % 2
    want = _oracle_lvq(oracle, kind, codes, clab, x, lab, 300)
    knn = 2 if kind >= 3 else 1
    trace = want[2].reshape(-1, knn)
    for j, (a, b) in enumerate(pairs):                       # every pair is still a tie when its first sample arrives,
        assert list(trace[2 * j]) == ([b, a] if knn == 2 else [a]), (j, trace[2 * j])      # in the reference's order
    _lvq_check(eng, E, kind, codes, clab, x, lab, 300, want)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [61, 64, 67, 68, 131])
def test_k5_forced_masked(eng, E, oracle, monkeypatch, dim, kind):
    monkeypatch.setenv("SOMHIP_LVQ_ONLINE", "1")
    codes, clab, x, lab = _lvq_case(7000 + dim, 300, dim, 200)
    mask = _mask(dim + 1, 200, dim)
    want = lvq_replay(oracle, kind, codes, clab, x, lab, 300, 0.3 if kind == 2 else 0.05, mask=mask, **_lvq_kw(kind))
    _lvq_check(eng, E, kind, codes, clab, x, lab, 300, want, mask=mask)


# =========================================================================== CPU: the witnesses themselves
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [13, 64])
def test_replay_without_a_mask_is_the_oracle(oracle, dim, kind):
    """tests/lvq_masked_replay.py, unmasked, against oracle.lvq_train: traces, codes and rates bit for bit, in one run and
    in two pieces; with a mask of zeros it is the same run again"""
    codes, clab, x, lab = _lvq_case(8000 + dim, 90, dim, 200)
    alpha = 0.3 if kind == 2 else 0.05
    oc, ol, oi, od = oracle.lvq_train(kind, codes, clab, x, lab, 500, alpha, **_lvq_kw(kind))
    assert not np.array_equal(bits(oc), bits(codes))
    for mask in (None, np.zeros(x.shape, dtype=np.uint8)):
        rc, rl, ri, rd = lvq_replay(oracle, kind, codes, clab, x, lab, 500, alpha, mask=mask, **_lvq_kw(kind))
        assert np.array_equal(ri, oi) and np.array_equal(bits(rd), bits(od)) and np.array_equal(bits(rc), bits(oc))
        if kind == 2:
            assert np.array_equal(bits(rl), bits(ol))
            wrong = clab[oi] != lab[np.arange(500) % 200]
            assert (ol < np.float32(alpha)).any() and wrong.any() and not wrong.all()       # both branches of the rate rule ran
    c1, l1, i1, d1 = lvq_replay(oracle, kind, codes, clab, x, lab, 500, alpha, count=123, **_lvq_kw(kind))
    c2, l2, i2, d2 = lvq_replay(oracle, kind, c1, clab, x, lab, 500, alpha, start_iter=123, talpha=l1, **_lvq_kw(kind))
    assert np.array_equal(np.concatenate([i1, i2]), oi) and np.array_equal(bits(c2), bits(oc))


def test_replay_with_a_mask_skips_what_the_sample_masks(oracle):
    """the masked replay reads no masked component (garbage under the mask changes nothing) and is another run than the
    unmasked one"""
    codes, clab, x, lab = _lvq_case(8100, 90, 13, 200)
    mask = _mask(9, 200, 13)
    a = lvq_replay(oracle, 4, codes, clab, x, lab, 300, 0.05, mask=mask, **_lvq_kw(4))
    b = lvq_replay(oracle, 4, codes, clab, _garbage(x, mask, 1), lab, 300, 0.05, mask=mask, **_lvq_kw(4))
    c = lvq_replay(oracle, 4, codes, clab, x, lab, 300, 0.05, **_lvq_kw(4))
    assert np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(bits(a[0]), bits(b[0]))
    assert not np.array_equal(bits(a[0]), bits(c[0]))


def test_oracle_is_the_reference_at_dim_67_masked(oracle, ref):
    """the oracle's own pin at a long ragged dim: ref.som_train == oracle.som_train, 13 x 5 hexa gaussian, masked"""
    x, mask = _graph_case()
    ini = oracle.randinit(x, 13, 5, 3)
    rc, ri, rd = ref.som_train(ini, 13, 5, HEXA, GAUSSIAN, x, 300, 0.07, 8.0, mask=mask)
    oc, oi, od = oracle.som_train(ini, 13, 5, HEXA, GAUSSIAN, x, 300, 0.07, 8.0, mask=mask)
    assert np.array_equal(oi, ri) and np.array_equal(bits(od), bits(rd)) and np.array_equal(bits(oc), bits(rc))
    assert not np.array_equal(bits(oc), bits(ini))
