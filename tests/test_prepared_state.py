"""A codebook's prepared copies follow every writer of its rows.

Every pre-filtered search reads derived copies of the codebook: the bf16 hi / lo tiles, the squared norms and, on long
runs, the row-major fp32 copy that the EXACT re-rank gathers from.  They are a cache on the codebook, guarded by
prep_valid and rowmajor_valid (csrc/somhip.hip: "cleared by every writer"); pf_prepare trusts the flags.  A writer that
forgets one gives a silently wrong answer.  Here the state is read as it lies (somhip_debug_prepared_state: nothing is
launched, no flag changes) after every writer and every reader of the ABI:

  check_state   a flag that is set must tell the truth -- tiles bit-equal to the full split of the rows downloaded, norms
                within the bound of recursive summation (bit-equal for rows no writer touched), the row-major copy
                bit-equal -- and, flags or not, the next search must be find_winner_euc's over the rows as they are.
  writers       one table; each case starts on the cached route (flags (1, 1)) and must move rows.
  LVQ           the batched engine keeps prep_valid by re-splitting exactly the rows a batch corrected (k_prep_rows_bf16):
                flags (1, 0) afterwards are the witness that the partial re-split ran, and check_state holds it to the
                full split.
  readers       keep the flags and the bits.

Priming.  somhip_find_winners searches a run in pieces of at most 4096 samples, so on its own it never asks for the
row-major copy (pf_prepare makes it from 8192 samples per run on).  The prime therefore runs the search of a whole
8192-sample run first (somhip_batch_winner_keys, what som_train's long batches and the shard drivers call) and then
find_winners over the same rows, which from then on gathers from the copy: flags (1, 1).

Needs an MI355X:  pytest -m gpu  (the last tests of the file do not)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth
from test_lvq_family_layouts import unit_of_row
from test_prepared_copies import row_norms, split_bf16, tiles  # noqa: F401  (split_bf16: what tiles splits with)

gpu = pytest.mark.gpu

U = 2.0 ** -24
N, DIM = 8192, 32                    # samples (the smallest run that gets the row-major copy) and their components
MAP = (64, 64)                       # 64 row groups (the fewest with the copy), stored by 8 x 8 patches
PLAIN = 4133                         # 65 groups, the last partial; from 4096 rows on LVQ's top-8 scan is pre-filtered
PAD_NORM = np.float32(3.0e38)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    e.set_scan_mode("mfma_bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    x, lab = synth(4242, N, DIM)
    return x, lab


@pytest.fixture(scope="module")
def ds(E, eng, data):
    return E.Dataset(eng, data[0], labels=data[1])


def map_rows(data, seed=1):
    rs = np.random.RandomState(seed)
    n = MAP[0] * MAP[1]
    return (data[0][rs.randint(0, N, n)] + 0.3 * rs.standard_normal((n, DIM))).astype(np.float32)


def plain_rows(data, n=PLAIN, seed=2):
    rs = np.random.RandomState(seed)
    pick = rs.randint(0, N, n)
    d = data[0].shape[1]
    rows = (data[0][pick] + 0.3 * rs.standard_normal((n, d))).astype(np.float32)
    clab = data[1][pick].copy()
    wrong = rs.random_sample(n) < 0.3            # neighbours of different classes: LVQ2.1 and LVQ3 find their windows
    clab[wrong] = rs.randint(1, 7, wrong.sum())
    return rows, clab


def make_map(E, eng, data, neigh=None):
    return E.Codebook(eng, map_rows(data), E.TOPOL_HEXA, E.NEIGH_BUBBLE if neigh is None else neigh, MAP[0], MAP[1])


def make_plain(E, eng, data):
    rows, clab = plain_rows(data)
    return E.Codebook(eng, rows, labels=clab)


# ------------------------------------------------------------------------------------------------ the state
def storage_units(cb):
    """the unit each storage row holds: a map whose sides are multiples of 8 is stored by 8 x 8 patches"""
    if cb.topol >= 3 and cb.xdim % 8 == 0 and cb.ydim % 8 == 0:
        return unit_of_row(cb.xdim, cb.ydim)
    return np.arange(cb.n)


def prime(E, eng, cb, ds, count=N):
    """the cached route: one whole run of `count` samples, then find_winners; flags (1, 1) or the case is void"""
    kb = eng.device_alloc(8 * count)
    try:
        E.check(eng.lib.somhip_batch_winner_keys(cb.h, ds.h, 0, count, kb))
        eng.sync()
    finally:
        eng.device_free(kb)
    E.find_winners(cb, ds, 0, count)
    st = E.debug_prepared_state(cb)
    assert (st["prep_valid"], st["rowmajor_valid"]) == (1, 1), "the case is not on the cached route"
    assert st["chi"] is not None and st["clo"] is not None and st["cn"] is not None and st["rowmajor"] is not None
    return st


def first_rows(diff):
    return np.unique(np.nonzero(diff)[0])[:8]


def check_state(E, eng, oracle, cb, ds, x, count=N, split_rows=None, want=None):
    """What the flags claim against the rows as they are, then the end-to-end witness.  split_rows: the rows at the last
    full split -- the norms of rows that still have those bits keep the bits of the full split's sum.  want: (index,
    distance) of oracle.winners for these rows where the caller has them already.  Returns the state and `want`."""
    rows = cb.download()
    st = E.debug_prepared_state(cb)
    n, d = rows.shape
    d8, ng = (d + 7) // 8, (n + 63) // 64
    stored = rows[storage_units(cb)]
    if st["rowmajor_valid"]:
        assert st["prep_valid"], "rowmajor_valid without prep_valid"
    if st["prep_valid"]:
        chi, clo = tiles(stored, 64, d8)
        for name, got, ref in (("chi", st["chi"], chi), ("clo", st["clo"], clo)):
            assert got is not None, name
            bad = got != ref
            assert not bad.any(), "%s: stale tiles in groups %s" % (name, first_rows(bad))
        cn = st["cn"]
        assert np.array_equal(cn[n:].view(np.uint32), np.full(ng * 64 - n, PAD_NORM).view(np.uint32)), "padding rows' norms"
        # recursive summation of the 8 d8 rounded squares in any order: gamma_k, k = 8 d8 + 1 (one rounding per square,
        # at most 8 d8 - 1 per sum, one to spare), relative to the sum of the squares themselves -- all terms are >= 0
        k = 8 * d8 + 1
        gam = k * U / (1.0 - k * U)
        s64 = (stored.astype(np.float64) ** 2).sum(axis=1)
        err = np.abs(cn[:n].astype(np.float64) - s64)
        assert (err <= gam * s64).all(), ("norms outside gamma_%d in storage rows" % k, np.flatnonzero(err > gam * s64)[:8])
        if split_rows is not None:
            same = (bits(stored) == bits(split_rows[storage_units(cb)])).all(axis=1)
            assert same.any()
            full = row_norms(stored, d8)
            assert np.array_equal(cn[:n][same].view(np.uint32), full[same].view(np.uint32)), "untouched rows' norms changed"
    if st["rowmajor_valid"]:
        ref = np.zeros((ng * 64, d), dtype=np.float32)
        ref[:n] = stored
        bad = st["rowmajor"].view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), "stale row-major copy in storage rows %s" % first_rows(bad)
    # the witness: the next search finds find_winner_euc's winners over the rows as they are
    gi, gd, _ = E.find_winners(cb, ds, 0, count)
    if want is None:
        oi, od, _ = oracle.winners(rows, x[:count])
        want = (oi, od)
    assert np.array_equal(gi, want[0]), ("winners differ at samples", np.flatnonzero((gi != want[0]).reshape(count, -1).any(axis=1))[:8])
    assert np.array_equal(bits(gd), bits(want[1])), "distances differ"
    fresh = E.Codebook(eng, rows, cb.topol, cb.neigh, cb.xdim, cb.ydim, labels=cb.labels)
    try:
        fi, fd, _ = E.find_winners(fresh, ds, 0, count)
    finally:
        fresh.close()
    assert np.array_equal(gi, fi) and np.array_equal(bits(gd), bits(fd)), "a fresh codebook of the same rows answers differently"
    return st, want


# ------------------------------------------------------------------------------------------------ writers
class DevBuf:
    def __init__(self, eng, nbytes):
        self.e, self.p = eng, eng.device_alloc(max(1, int(nbytes)))

    def free(self):
        self.e.device_free(self.p)


def lvq_kw(kind):
    kw = {"winlen": 0.3} if kind >= 3 else {}
    if kind == 4:
        kw["epsilon"] = 0.15
    return kw


def w_upload(E, eng, cb, ds, data):
    cb.upload((1.5 * cb.download()[::-1] - 2.0).astype(np.float32))


def w_som_train(batch, mode="exact"):
    def run(E, eng, cb, ds, data):
        eng.set_update_mode(mode)
        try:
            E.som_train(cb, ds, 300 if batch == 1 else 512, 0.5, 6.0, batch=batch, trace=False)
        finally:
            eng.set_update_mode("exact")
    return run


def w_som_batch_update(E, eng, cb, ds, data):
    from som_lvq_pak_amd._lib import SomParams
    kb = DevBuf(eng, 8 * 256)
    try:
        p = SomParams(512, 0.5, 6.0, E.ALPHA_LINEAR, 0, 0, 256, 0, 512, 0)
        for it0 in (0, 256):
            E.check(eng.lib.somhip_batch_winner_keys(cb.h, ds.h, it0, 256, kb.p))
            E.check(eng.lib.somhip_som_batch_update(cb.h, ds.h, C.byref(p), it0, 256, it0, kb.p))
        eng.sync()
    finally:
        kb.free()


def w_lvq_train(kind, env=None):
    def run(E, eng, cb, ds, data):
        if env:
            os.environ[env] = "1"
        try:
            plan = E.lvq_plan(cb, ds, kind, 400, 0.3, trace=False, **lvq_kw(kind))
            E.lvq_train(cb, ds, kind, 400, 0.3, trace=False, **lvq_kw(kind))
        finally:
            if env:
                os.environ.pop(env, None)
        assert (plan["engine"], plan["loop"]) == {None: ("batched", "nowait"), "SOMHIP_LVQ_SYNC": ("batched", "careful"),
                                                   "SOMHIP_LVQ_ONLINE": ("online", "nowait")}[env], plan
    return run


def w_lvq_batch_apply(kind):
    """the three calls of a batch over a row-sharded codebook, on a codebook that is the only shard"""
    def run(E, eng, cb, ds, data):
        from som_lvq_pak_amd._lib import LvqParams
        length, B, xrows, d4 = 400, 256, 8, (cb.dim + 3) // 4
        kw = lvq_kw(kind)
        if kind == E.OLVQ1:
            E.lvq_rates_upload(cb, np.full(cb.n, 0.3, dtype=np.float32))
        keys, lab, ta, rows = DevBuf(eng, 8 * B * 8), DevBuf(eng, 4 * B * 8), DevBuf(eng, 4 * B * 8), DevBuf(eng, 4 * B * xrows * 4 * d4)
        try:
            p = LvqParams(kind, length, 0.3, E.ALPHA_LINEAR, kw.get("winlen", 0.0), kw.get("epsilon", 0.0), 0, 0, 0)
            off = 0
            while off < length:
                c = min(B, length - off)
                E.check(eng.lib.somhip_batch_topk_keys(cb.h, ds.h, off, c, 8, E.TIE_KNN if kind >= 3 else E.TIE_FIRST, keys.p))
                E.check(eng.lib.somhip_lvq_batch_candidates(cb.h, c, kind, keys.p, xrows, lab.p, ta.p if kind == E.OLVQ1 else None, rows.p))
                done = C.c_int64(0)
                E.check(eng.lib.somhip_lvq_batch_apply(cb.h, ds.h, C.byref(p), off, c, off, keys.p, lab.p, ta.p if kind == E.OLVQ1 else None,
                                                       rows.p, xrows, C.byref(done), None, None))
                assert 0 < done.value <= c
                off += done.value
        finally:
            for b in (keys, lab, ta, rows):
                b.free()
    return run


def w_som_batchmap(E, eng, cb, ds, data):
    E.som_batchmap(cb, ds, 2, 6.0)


def w_batchmap_whole(E, eng, cb, ds, data):
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds)
    E.batchmap_finish(cb, 6.0)


def w_batchmap_ranges(E, eng, cb, ds, data):
    ng = (cb.n + 63) // 64
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds)
    E.batchmap_finish(cb, 6.0, 0, ng // 2)
    st = E.debug_prepared_state(cb)
    assert (st["prep_valid"], st["bm_open"], st["bm_moved"]) == (0, 1, 1), "between two ranges of a combine"
    E.batchmap_finish(cb, 6.0, ng // 2, ng - ng // 2)


def w_batchmap_ranks(E, eng, cb, ds, data):
    from som_lvq_pak_amd import _lib
    comm = C.c_void_p()
    E.check(eng.lib.somhip_comm_create_sockets(eng.h, 0, 1, None, C.byref(comm)))
    try:
        p = _lib.BatchmapParams(2, 6.0, 0, 2, 0, ds.n)
        q = np.zeros(2, dtype=np.float32)
        E.check(eng.lib.somhip_som_batchmap_ranks(cb.h, ds.h, C.byref(p), comm, q.ctypes.data_as(_lib.c_float_p)))
    finally:
        eng.lib.somhip_comm_destroy(comm)


def w_batchmap_combine(E, eng, cb, ds, data):
    hits, sums = E.batchmap_sums(cb, ds)
    E.batchmap_combine(cb, 6.0, hits, sums)


M = 2048          # samples of an epoch of the full-batch trainers: enough to move most rows, seconds on the device


def w_glvq_train(E, eng, cb, ds, data):
    E.glvq_train(cb, ds, 2, 50.0, n=M, stats=False)


def w_glvq_update(E, eng, cb, ds, data):
    s = E.glvq_sums(cb, ds, n=M)
    E.glvq_update(cb, 50.0, M, s["sums_plus"], s["n_plus"], s["sums_minus"], s["n_minus"])


def w_grlvq_train(E, eng, cb, ds, data):
    E.grlvq_train(cb, ds, 2, 50.0, 0.01, n=M, stats=False)


def w_grlvq_update(E, eng, cb, ds, data):
    s = E.grlvq_sums(cb, ds, n=M)
    E.grlvq_update(cb, 50.0, 0.01, M, None, s["sums_plus"], s["n_plus"], s["sums_minus"], s["n_minus"], s["grad"])


def w_gmlvq_train(E, eng, cb, ds, data):
    E.gmlvq_train(cb, ds, 2, 50.0, 0.01, n=M, stats=False)


def w_gmlvq_update(E, eng, cb, ds, data):
    s = E.gmlvq_sums(cb, ds, n=M)
    E.gmlvq_update(cb, 50.0, 0.01, M, None, s["sums_plus"], s["n_plus"], s["sums_minus"], s["n_minus"], s["grad"])


def w_ng_train(E, eng, cb, ds, data):
    E.ng_train(cb, ds, 2, lambda0=2.0, n=M, qerror=False)


def w_ng_update(E, eng, cb, ds, data):
    w = E.ng_schedule(cb.n, 2, 0, 2.0)[2]
    hits, sums, wsum = E.ng_sums(cb, ds, w, n=M)
    E.ng_update(cb, hits, sums, wsum)


LVQ_LOOPS = (("nowait", None), ("careful", "SOMHIP_LVQ_SYNC"), ("online", "SOMHIP_LVQ_ONLINE"))

# id -> (entry points that write rows, codebook, the writer, the flags (prep_valid, rowmajor_valid) it must leave)
WRITERS = {
    "upload_map": (("somhip_codebook_upload",), "map", w_upload, (0, 0)),
    "upload_plain": (("somhip_codebook_upload",), "plain", w_upload, (0, 0)),
    "som_train_batch1": (("somhip_som_train",), "map", w_som_train(1), (0, 0)),
    "som_train_batch256_exact": (("somhip_som_train",), "map", w_som_train(256), (0, 0)),
    "som_train_batch256_gemm": (("somhip_som_train",), "map", w_som_train(256, "gemm"), (0, 0)),
    "som_train_batch256_gaussian": (("somhip_som_train",), "map_gaussian", w_som_train(256), (0, 0)),
    "som_batch_update": (("somhip_som_batch_update",), "map", w_som_batch_update, (0, 0)),
    "som_batchmap": (("somhip_som_batchmap",), "map", w_som_batchmap, (0, 0)),
    "batchmap_pieces_whole": (("somhip_batchmap_finish",), "map", w_batchmap_whole, (0, 0)),
    "batchmap_pieces_two_ranges": (("somhip_batchmap_finish",), "map", w_batchmap_ranges, (0, 0)),
    "som_batchmap_ranks": (("somhip_som_batchmap_ranks",), "map", w_batchmap_ranks, (0, 0)),
    "debug_batchmap_combine": (("somhip_debug_batchmap_combine",), "map", w_batchmap_combine, (0, 0)),
    "glvq_train": (("somhip_glvq_train",), "plain", w_glvq_train, (0, 0)),
    "debug_glvq_update": (("somhip_debug_glvq_update",), "plain", w_glvq_update, (0, 0)),
    "grlvq_train": (("somhip_grlvq_train",), "plain", w_grlvq_train, (0, 0)),
    "debug_grlvq_update": (("somhip_debug_grlvq_update",), "plain", w_grlvq_update, (0, 0)),
    "gmlvq_train": (("somhip_gmlvq_train",), "plain", w_gmlvq_train, (0, 0)),
    "debug_gmlvq_update": (("somhip_debug_gmlvq_update",), "plain", w_gmlvq_update, (0, 0)),
    "ng_train": (("somhip_ng_train",), "plain", w_ng_train, (0, 0)),
    "ng_train_map": (("somhip_ng_train",), "map", w_ng_train, (0, 0)),
    "debug_ng_update": (("somhip_debug_ng_update",), "plain", w_ng_update, (0, 0)),
}
for _kind in (1, 2, 3, 4):
    for _loop, _env in LVQ_LOOPS:
        # the batched engine re-splits the rows it corrected and keeps the tiles; the row-major copy is not re-split
        WRITERS["lvq_train_kind%d_%s" % (_kind, _loop)] = (("somhip_lvq_train",), "plain", w_lvq_train(_kind, _env),
                                                           (0, 0) if _loop == "online" else (1, 0))
    WRITERS["lvq_batch_apply_kind%d" % _kind] = (("somhip_lvq_batch_apply",), "plain", w_lvq_batch_apply(_kind), (1, 0))
BATCHMAP_PIECES = ("batchmap_pieces_whole", "batchmap_pieces_two_ranges")


def make_codebook(E, eng, data, which):
    if which == "plain":
        return make_plain(E, eng, data)
    return make_map(E, eng, data, E.NEIGH_GAUSSIAN if which == "map_gaussian" else None)


@gpu
@pytest.mark.parametrize("case", sorted(WRITERS))
def test_writer_leaves_a_true_state(E, eng, oracle, data, ds, case):
    _, which, writer, flags = WRITERS[case]
    cb = make_codebook(E, eng, data, which)
    try:
        prime(E, eng, cb, ds)
        before = cb.download()
        writer(E, eng, cb, ds, data)
        after = cb.download()
        moved = (bits(after) != bits(before)).any(axis=1)
        assert moved.sum() >= 8, "the writer moved %d rows" % moved.sum()
        st = E.debug_prepared_state(cb)
        if case not in BATCHMAP_PIECES:
            assert st["bm_open"] == 0
        assert (st["prep_valid"], st["rowmajor_valid"]) == flags
        check_state(E, eng, oracle, cb, ds, data[0], split_rows=before)
    finally:
        cb.close()


# ------------------------------------------------------------------------------------------------ LVQ: the partial re-split
def labelled(seed, n, d):
    """8192 `synth` rows of d components and a codebook of n rows near them"""
    x, lab = synth(seed, N, d)
    rows, clab = plain_rows((x, lab), n, seed + 1)
    return x, lab, rows, clab


def run_resplit(E, eng, oracle, x, lab, rows, clab, kind, length, alpha, count=N, env=None):
    """prime, train in the batched engine, (1, 0), check_state; returns the rows before and after"""
    dsl = E.Dataset(eng, x, labels=lab)
    cb = E.Codebook(eng, rows, labels=clab)
    try:
        prime(E, eng, cb, dsl)
        if env:
            os.environ[env] = "1"
        try:
            E.lvq_train(cb, dsl, kind, length, alpha, trace=False, **lvq_kw(kind))
        finally:
            if env:
                os.environ.pop(env, None)
        after = cb.download()
        assert (bits(after) != bits(rows)).any()
        st = E.debug_prepared_state(cb)
        # kept by the re-split of the corrected rows; a full split would have left no reason to drop the row-major copy
        assert (st["prep_valid"], st["rowmajor_valid"]) == (1, 0), "k_prep_rows_bf16 did not keep the tiles"
        check_state(E, eng, oracle, cb, dsl, x, count=count, split_rows=rows)
        return after
    finally:
        cb.close()
        dsl.close()


@gpu
@pytest.mark.parametrize("loop,env", [("nowait", None), ("careful", "SOMHIP_LVQ_SYNC")])
@pytest.mark.parametrize("n,d,length,count", [(4096, 36, 400, N),        # odd d4: the zero half of the last k-block
                                              (4096, 520, 600, 512)])    # d8 = 65: the second trip of the 64 lanes
def test_lvq_resplit_shapes(E, eng, oracle, n, d, length, count, loop, env):
    """(4133 x 32, every kind and loop, is in the writers' table)"""
    x, lab, rows, clab = labelled(100 + d, n, d)
    for kind in (E.LVQ1, E.LVQ3):
        run_resplit(E, eng, oracle, x, lab, rows, clab, kind, length, 0.3, count=count, env=env)


@gpu
def test_lvq_resplit_skips_a_poisoned_batch(E, eng, oracle):
    """A dozen rows of mixed labels inside one tight blob that holds every sample, every other row far away: the walk
    runs out of candidates, the batch is poisoned, the no-wait loop's refresh of that batch must be skipped (its row list
    is not committed) and the careful redo's must not."""
    d = DIM
    rs = np.random.RandomState(77)
    x = (0.3 * rs.standard_normal((N, d))).astype(np.float32)
    lab = rs.randint(1, 4, N).astype(np.int32)
    rows = (100.0 + rs.standard_normal((PLAIN, d))).astype(np.float32)
    clab = rs.randint(1, 4, PLAIN).astype(np.int32)
    rows[:12] = x[:12]
    clab[:12] = lab[:12]
    s0 = eng.lvq_stats()
    after = run_resplit(E, eng, oracle, x, lab, rows, clab, E.LVQ1, 1500, 0.08)
    s1 = eng.lvq_stats()
    assert s1["stop_list"] - s0["stop_list"] > 0, "no batch ran out of candidates: tighten the blob"
    assert (bits(after[12:]) == bits(rows[12:])).all()


@gpu
def test_lvq_resplit_row_grows_to_the_largest_norm(E, eng, oracle):
    """the samples of an outlier class pull one row outward until it holds the codebook's largest norm: the windows of the
    next search are formed from the maximum over d_cn, which only the partial re-split has updated"""
    x, lab, rows, clab = labelled(300, PLAIN, DIM)
    x, lab = x.copy(), lab.copy()
    rs = np.random.RandomState(5)
    axis = np.zeros(DIM, dtype=np.float32)
    axis[3] = 1.0
    x[::16] = 300.0 * axis + rs.standard_normal((N // 16, DIM)).astype(np.float32)
    lab[::16] = 9
    rows[17], clab[17] = 0.0, 9
    rows[17] = np.float32(0.95 * np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max())) * axis
    norms = (rows.astype(np.float64) ** 2).sum(axis=1)
    xs = x[::16].astype(np.float64)
    dist = (xs ** 2).sum(axis=1)[:, None] - 2.0 * xs @ rows.astype(np.float64).T + norms[None, :]
    # the construction: row 17 is the nearest row of every outlier sample (its own class), and not yet the largest
    assert (dist.argmin(axis=1) == 17).all() and norms.argmax() != 17
    after = run_resplit(E, eng, oracle, x, lab, rows, clab, E.LVQ1, 400, 0.3)
    grown = (after.astype(np.float64) ** 2).sum(axis=1)
    assert grown.argmax() == 17 and grown[17] > 2.0 * norms.max(), (grown.argmax(), grown[17], norms.max())


# ------------------------------------------------------------------------------------------------ scan-mode edges
@gpu
def test_writer_in_another_scan_mode(E, eng, oracle, data, ds):
    """a valid bf16 state; rows written while the engine scans in another mode; back in bf16 the state must be invalid"""
    for mode, which in (("mfma", "plain"), ("direct", "map")):
        cb = make_codebook(E, eng, data, which)
        try:
            prime(E, eng, cb, ds)
            before = cb.download()
            eng.set_scan_mode(mode)
            try:
                if which == "plain":
                    E.lvq_train(cb, ds, E.LVQ1, 400, 0.3, trace=False)
                else:
                    E.som_train(cb, ds, 512, 0.5, 6.0, batch=256, trace=False)
            finally:
                eng.set_scan_mode("mfma_bf16")
            assert (bits(cb.download()) != bits(before)).any()
            st = E.debug_prepared_state(cb)
            assert st["prep_valid"] == 0 and st["rowmajor_valid"] == 0, mode
            check_state(E, eng, oracle, cb, ds, data[0])
        finally:
            cb.close()


@gpu
def test_fp32_search_between_two_bf16_searches(E, eng, oracle, data, ds):
    """an "mfma" search of unchanged rows rewrites d_cn in k_row_norms' order: the flags stay, the norms stay in bound"""
    cb = make_map(E, eng, data)
    try:
        prime(E, eng, cb, ds)
        eng.set_scan_mode("mfma")
        try:
            mi, md, _ = E.find_winners(cb, ds, 0, N)
        finally:
            eng.set_scan_mode("mfma_bf16")
        st = E.debug_prepared_state(cb)
        assert (st["prep_valid"], st["rowmajor_valid"]) == (1, 1)
        _, want = check_state(E, eng, oracle, cb, ds, data[0])
        assert np.array_equal(mi, want[0]) and np.array_equal(bits(md), bits(want[1]))
    finally:
        cb.close()


# ------------------------------------------------------------------------------------------------ readers
def r_find_winners(knn):
    def run(E, eng, cb, ds):
        E.find_winners(cb, ds, 0, N, knn=knn, tie=E.TIE_KNN if knn > 1 else E.TIE_FIRST)
    return run


def r_distortion(E, eng, cb, ds):
    st = E.Distortion(cb)
    try:
        st.accumulate(cb, ds)
        st.evaluate(cb, 3.0)
        hits, sums, sq = st.read()
    finally:
        st.close()
    E.distortion_evaluate(cb, 3.0, hits, sums, sq)


def r_map_connectivity(E, eng, cb, ds):
    conn = E.Conn(eng)
    try:
        E.map_connectivity(cb, ds, conn, quality=True)
    finally:
        conn.close()


def r_batchmap_open(E, eng, cb, ds):
    E.batchmap_begin(cb)
    E.batchmap_accumulate(cb, ds)
    E.batchmap_state(cb)
    st = E.debug_prepared_state(cb)
    assert (st["bm_open"], st["bm_moved"]) == (1, 0)
    E.batchmap_end(cb)
    assert E.debug_prepared_state(cb)["bm_open"] == 0


def r_plans(E, eng, cb, ds):
    E.scan_plan(cb, ds, N, 1)
    E.device_ptrs(cb, ds)
    if cb.topol >= 3:
        E.update_plan(cb, ds, 512, 0.5, 6.0, 256)
    else:
        E.lvq_plan(cb, ds, E.LVQ1, 400, 0.3)
        E.lvq_relation(cb, ds, E.LVQ1, 400, 0.3, count=256)


def r_shard_search(E, eng, cb, ds):
    """the search of a row-sharded codebook in its three calls, and the top-8 lists with their candidates' rows"""
    lib = eng.lib
    keys, bound = DevBuf(eng, 8 * N), DevBuf(eng, 4 * N)
    lab, rows = DevBuf(eng, 4 * 1024 * 8), DevBuf(eng, 4 * 1024 * 8 * 4 * ((cb.dim + 3) // 4))
    try:
        assert lib.somhip_shard_exchange_available(cb.h, ds.h, N) == 1
        E.check(lib.somhip_shard_winner_begin(cb.h, ds.h, 0, N, keys.p, bound.p))
        E.check(lib.somhip_shard_winner_refine(cb.h, ds.h, 0, N, bound.p))
        E.check(lib.somhip_shard_winner_finish(cb.h, ds.h, 0, N, bound.p, keys.p))
        E.check(lib.somhip_batch_topk_keys(cb.h, ds.h, 0, 1024, 8, E.TIE_FIRST, keys.p))
        if cb.labels is not None:
            E.check(lib.somhip_lvq_batch_candidates(cb.h, 1024, E.LVQ1, keys.p, 8, lab.p, None, rows.p))
        eng.sync()
    finally:
        for b in (keys, bound, lab, rows):
            b.free()


def r_rates(E, eng, cb, ds):
    E.lvq_rates_upload(cb, np.full(cb.n, 0.25, dtype=np.float32))
    back = np.empty(cb.n, dtype=np.float32)
    E.check(eng.lib.somhip_lvq_rates_download(cb.h, back.ctypes.data_as(C.POINTER(C.c_float))))
    assert (back == np.float32(0.25)).all()


def r_sammon(E, eng, cb, ds):
    E.sammon_zero_pairs(cb)
    rs = np.random.RandomState(3)
    E.sammon(cb, rs.random_sample(cb.n), rs.random_sample(cb.n), 1)


def r_debug_searches(E, eng, cb, ds):
    from som_lvq_pak_amd import _lib
    E.debug_rerank_pairs(cb, ds, 0, 1024, False)
    wmin, tau, bpad = np.zeros(((cb.n + 63) // 64, 1024), np.float32), np.zeros(1024, np.float32), C.c_int64(0)
    E.check(eng.lib.somhip_debug_prefilter(cb.h, ds.h, 0, 1024, wmin.ctypes.data_as(_lib.c_float_p), tau.ctypes.data_as(_lib.c_float_p),
                                           C.byref(bpad)))
    assert bpad.value == 1024


# id -> (entry points, codebook, the reader)
READERS = {
    "find_winners_knn1": (("somhip_find_winners",), "map", r_find_winners(1)),
    "find_winners_knn8": (("somhip_find_winners",), "plain", r_find_winners(8)),
    "find_winners_knn9": (("somhip_find_winners",), "plain", r_find_winners(9)),
    "knn_vote": (("somhip_knn_vote",), "plain", lambda E, eng, cb, ds: E.knn_vote(cb, ds, knn=5)),
    "map_quality": (("somhip_map_quality",), "map", lambda E, eng, cb, ds: E.map_quality(cb, ds)),
    "map_connectivity": (("somhip_map_connectivity",), "map", r_map_connectivity),
    "distortion": (("somhip_distortion_create", "somhip_distortion_accumulate", "somhip_distortion_evaluate",
                    "somhip_debug_distortion_evaluate"), "map", r_distortion),
    "batchmap_begin_accumulate": (("somhip_batchmap_begin", "somhip_batchmap_accumulate", "somhip_batchmap_state", "somhip_batchmap_end"),
                                  "map", r_batchmap_open),
    "debug_batchmap_sums": (("somhip_debug_batchmap_sums",), "map", lambda E, eng, cb, ds: E.batchmap_sums(cb, ds)),
    "umatrix": (("somhip_umatrix",), "map", lambda E, eng, cb, ds: E.umatrix(cb, average=True)),
    "planes": (("somhip_planes",), "map", lambda E, eng, cb, ds: E.planes(cb)),
    "qerror2": (("somhip_qerror2",), "map", lambda E, eng, cb, ds: E.qerror2_sum(cb, ds, 3.0, count=1024)),
    "glvq_search": (("somhip_debug_glvq_search", "somhip_debug_glvq_sums"), "plain",
                    lambda E, eng, cb, ds: (E.glvq_search(cb, ds), E.glvq_sums(cb, ds, n=M))),
    "grlvq_search": (("somhip_grlvq_search", "somhip_debug_grlvq_sums"), "plain",
                     lambda E, eng, cb, ds: (E.grlvq_search(cb, ds), E.grlvq_sums(cb, ds, n=M))),
    "gmlvq_search": (("somhip_gmlvq_search", "somhip_debug_gmlvq_sums"), "plain",
                     lambda E, eng, cb, ds: (E.gmlvq_search(cb, ds), E.gmlvq_sums(cb, ds, n=M))),
    "gmlvq_project": (("somhip_gmlvq_project",), "plain", lambda E, eng, cb, ds: (E.gmlvq_project(cb, ds), E.gmlvq_project(cb))),
    "ng_ranks_sums": (("somhip_debug_ng_ranks", "somhip_debug_ng_sums"), "plain",
                      lambda E, eng, cb, ds: (E.ng_ranks(cb, ds, 9, n=M), E.ng_sums(cb, ds, E.ng_schedule(cb.n, 2, 0, 2.0)[2], n=M))),
    "download": (("somhip_codebook_download",), "plain", lambda E, eng, cb, ds: cb.download()),
    "lvq_rates": (("somhip_lvq_rates_upload", "somhip_lvq_rates_download"), "plain", r_rates),
    "plans_map": (("somhip_debug_scan_plan", "somhip_debug_device_ptrs", "somhip_debug_update_plan"), "map", r_plans),
    "plans_plain": (("somhip_debug_lvq_plan", "somhip_debug_lvq_relation"), "plain", r_plans),
    "shard_search": (("somhip_shard_exchange_available", "somhip_shard_winner_begin", "somhip_shard_winner_refine",
                      "somhip_shard_winner_finish", "somhip_batch_topk_keys", "somhip_lvq_batch_candidates"), "plain", r_shard_search),
    "debug_searches": (("somhip_debug_rerank_pairs", "somhip_debug_prefilter"), "map", r_debug_searches),
    "sammon": (("somhip_sammon_zero_pairs", "somhip_sammon"), "map", r_sammon),
    "prepared_state": (("somhip_debug_prepared_state",), "map", lambda E, eng, cb, ds: E.debug_prepared_state(cb)),
}
# the search of a whole run that the prime itself makes
PRIME = ("somhip_batch_winner_keys",)
# entry points that take a codebook and belong to neither table, and why
NEITHER = {
    "somhip_codebook_destroy": "ends the codebook",
    "somhip_debug_prepared": "clears prep_valid and prepares again by definition (tests/test_prepared_copies.py)",
    "somhip_debug_level1": "takes rows of whole 64-dim steps only, which neither codebook here has; it prepares through pf_prepare, "
                           "as every search in the readers' table does",
}


@pytest.fixture(scope="module")
def primed(E, eng, oracle, data, ds):
    """one primed codebook of each kind for all readers (they change nothing), with its winners computed once"""
    out = {}
    for which in ("map", "plain"):
        cb = make_codebook(E, eng, data, which)
        st = prime(E, eng, cb, ds)
        rows = cb.download()
        oi, od, _ = oracle.winners(rows, data[0])
        out[which] = (cb, rows, st, (oi, od))
    yield out
    for cb, _, _, _ in out.values():
        cb.close()


@gpu
@pytest.mark.parametrize("case", sorted(READERS))
def test_reader_keeps_the_cache(E, eng, oracle, data, ds, primed, case):
    _, which, reader = READERS[case]
    cb, rows, st0, want = primed[which]
    reader(E, eng, cb, ds)
    st = E.debug_prepared_state(cb)
    assert (st["prep_valid"], st["rowmajor_valid"], st["bm_open"]) == (1, 1, 0)
    for name in ("chi", "clo"):
        assert np.array_equal(st[name], st0[name]), name
    assert np.array_equal(st["rowmajor"].view(np.uint32), st0["rowmajor"].view(np.uint32))
    assert np.array_equal(bits(cb.download()), bits(rows)), "a reader moved rows"
    check_state(E, eng, oracle, cb, ds, data[0], split_rows=rows, want=want)


@gpu
def test_state_of_a_codebook_never_searched(E, eng, data):
    """no buffer exists yet: every flag 0, every array None, nothing written"""
    cb = make_plain(E, eng, data)
    try:
        st = E.debug_prepared_state(cb)
        assert [st[k] for k in ("prep_valid", "rowmajor_valid", "bm_open", "bm_moved")] == [0, 0, 0, 0]
        assert all(st[k] is None for k in ("chi", "clo", "cn", "rowmajor"))
        flags = (C.c_int32 * 4)(7, 7, 7, 7)
        E.check(eng.lib.somhip_debug_prepared_state(cb.h, flags, None, None, None, None))
        assert list(flags) == [0, 0, 0, 0]
    finally:
        cb.close()


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.fixture(scope="module")
def built():
    import subprocess
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


def header():
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def test_symbol_and_signature(built):
    from som_lvq_pak_amd import _lib, engine
    assert ("int somhip_debug_prepared_state(somhip_codebook *cb, int32_t flags[4], uint16_t *chi, uint16_t *clo, float *cn, "
            "float *rowmajor);") in header()
    assert _lib.SIGNATURES["somhip_debug_prepared_state"] == (C.c_int, [C.c_void_p, _lib.c_i32_p, _lib.c_u16_p, _lib.c_u16_p,
                                                                        _lib.c_float_p, _lib.c_float_p])
    assert hasattr(_lib.load(), "somhip_debug_prepared_state") and hasattr(engine, "debug_prepared_state")


def test_null_handles_are_refused_by_name(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    flags = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.somhip_debug_prepared_state(None, flags, None, None, None, None) != 0
    assert lib.somhip_last_error().decode() == "somhip_debug_prepared_state: null argument"
    assert list(flags) == [7, 7, 7, 7]


def test_every_writer_has_a_case():
    """every entry point of the ABI that takes a codebook it may write to is in the writers' table or the readers'"""
    takes = set()
    for name, args in re.findall(r"\b(somhip_[a-z0-9_]+) ?\(([^;{}]*?)\) ?;", header()):
        if re.search(r"(?<!const )somhip_codebook \*(?!\*)", args):
            takes.add(name)
    assert len(takes) >= 60 and "somhip_lvq_train" in takes and "somhip_codebook_create" not in takes
    writers = {s for syms, _, _, _ in WRITERS.values() for s in syms}
    readers = {s for syms, _, _ in READERS.values() for s in syms} | set(PRIME)
    assert not (writers & readers), writers & readers
    assert not (set(NEITHER) & (writers | readers))
    missing = takes - writers - readers - set(NEITHER)
    assert not missing, "entry points that take a codebook and have no case: %s" % sorted(missing)
    unknown = (writers | readers | set(NEITHER)) - takes
    assert not unknown, "not in the header: %s" % sorted(unknown)
