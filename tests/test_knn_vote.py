"""somhip_knn_vote (K1v): the class vote over find_winner_knn's neighbours, formed on the device behind the keys of
the search somhip_find_winners runs, against the oracle's find_winner_knn followed by a Python replay of the reference's
hit list (labels.c:370-410).  label, freq, own and found must be equal as integers.

The replay is the list itself -- [label, count] entries, a new label appended, a bumped entry swapped towards the head
while its predecessor's count is strictly smaller -- not the closed form the kernel uses ("the label whose count first
reaches the final maximum"); without a GPU it is compared with pak_io.c's list through tests/helpers/hitlist_heads.c."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

TIE_FIRST, TIE_KNN = 0, 1
TOPOL_HEXA = 3
KNNS = (1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 128, 255, 256)
ROWS = (1, 5, 64, 300, 1100)
DIMS = (1, 5, 37)
COUNTS = (1, 4, 5, 33)


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


def replay(labels):
    """the reference's hit list after add_hit of `labels` in order: [[label, count], ...], head first"""
    hl = []
    for lab in labels:
        lab = int(lab)
        for i, he in enumerate(hl):                 # find_hit
            if he[0] == lab:
                break
        else:
            hl.append([lab, 1])                     # add to end of list
            continue
        hl[i][1] += 1
        while i > 0 and hl[i - 1][1] < hl[i][1]:    # higher frequencies are in the beginning
            hl[i - 1], hl[i] = hl[i], hl[i - 1]
            i -= 1
    return hl


# ------------------------------------------------------------------------------------------------ without a GPU
def test_symbols_and_signatures(built):
    from som_lvq_pak_amd import _lib, engine
    lib = _lib.load()
    assert hasattr(lib, "somhip_knn_vote") and hasattr(lib, "somhip_knn_vote_timing")
    assert _lib.SIGNATURES["somhip_knn_vote"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                                            _lib.c_i32_p, _lib.c_i32_p, _lib.c_i32_p, _lib.c_i32_p])
    assert _lib.SIGNATURES["somhip_knn_vote_timing"] == (C.c_int, [C.c_void_p, _lib.c_i64_p, _lib.c_double_p])
    assert hasattr(engine, "knn_vote") and hasattr(engine.Engine, "knn_vote_timing")
    hdr = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert "somhip_knn_vote(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int knn," in hdr
    assert "somhip_knn_vote_timing(somhip_engine *e, int64_t *launches, double *total_ms);" in hdr


def test_null_handles_are_errors_not_crashes(built):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 4)()
    assert lib.somhip_knn_vote(None, None, 0, 1, 5, out, None, None, None) != 0
    assert lib.somhip_last_error().decode() == "somhip_knn_vote: null handle"
    n, ms = C.c_int64(0), C.c_double(0)
    assert lib.somhip_knn_vote_timing(None, C.byref(n), C.byref(ms)) != 0
    assert lib.somhip_last_error().decode() == "somhip_knn_vote_timing: null engine"


def test_replay_equals_the_tools_hit_list(built, tmp_path):
    """random label sequences (few classes: many ties; label 0; negative and large labels) through pak_io.c's add_hit"""
    exe = str(tmp_path / "hitlist_heads")
    host = os.path.join(ROOT, "som_lvq_pak_amd", "host")
    subprocess.check_call(["gcc", "-O2", "-I", host, "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "hitlist_heads.c"), os.path.join(host, "pak_io.c"), "-lm"])
    rs = np.random.RandomState(3)
    seqs = [[], [0], [7, 7], [5, 7, 2, 9, 7, 2, 9, 5]]
    for _ in range(400):
        classes = rs.choice([0, 1, 2, 3, 5, 8, -4, 70000, 2 ** 31 - 1], size=rs.randint(1, 7), replace=False)
        seqs.append([int(v) for v in rs.choice(classes, size=rs.randint(1, 300))])
    src = tmp_path / "seqs.txt"
    src.write_text("".join(" ".join(str(v) for v in s) + "\n" for s in seqs))
    p = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(seqs)
    for s, line in zip(seqs, lines):
        assert line == " ".join("%d:%d" % (lab, n) for lab, n in replay(s)), s
    # the list's head is not the smallest, the largest or the nearest label, but the first to reach the largest count
    assert replay([5, 7, 2, 9, 7, 2, 9, 5])[0] == [7, 2]


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    e.set_scan_mode("direct")
    yield e
    e.close()


def witness(oracle, codes, clab, x, xlab, knn, mask=None):
    """(label, freq, own, found) from the oracle's find_winner_knn and the replayed hit list"""
    widx, _, _ = oracle.winners(codes, x, knn, True, mask)
    m = x.shape[0]
    out = np.zeros((4, m), dtype=np.int32)
    for s in range(m):
        nb = widx[s][widx[s] >= 0]
        hl = replay(clab[nb])
        out[0, s], out[1, s] = hl[0] if hl else (-1, 0)
        out[2, s] = -1 if xlab is None else int((clab[nb] == xlab[s]).sum())
        out[3, s] = nb.size
    return out


def same(got, want, what=""):
    got = np.stack(got)
    bad = np.nonzero((got != want).any(axis=0))[0]
    assert bad.size == 0, "%s: %d of %d samples differ; first at %d: got (label, freq, own, found) %s, witness %s" % (
        what, bad.size, got.shape[1], bad[0], got[:, bad[0]], want[:, bad[0]])


def vote(E, eng, codes, clab, x, xlab, knn, mask=None, first=0, count=None, **cbkw):
    cb = E.Codebook(eng, codes, labels=clab, **cbkw)
    ds = E.Dataset(eng, x, mask=mask, labels=xlab)
    try:
        return E.knn_vote(cb, ds, first, count, knn=knn)
    finally:
        cb.close()
        ds.close()


@pytest.fixture(scope="module")
def grid_data():
    """per dimension: rows, their labels (four classes, 0 among them: ties are common), samples and their labels"""
    out = {}
    for dim in DIMS:
        rs = np.random.RandomState(40 + dim)
        out[dim] = (rs.standard_normal((max(ROWS), dim)).astype(np.float32), rs.randint(0, 4, max(ROWS)).astype(np.int32),
                    rs.standard_normal((max(COUNTS), dim)).astype(np.float32), rs.randint(0, 4, max(COUNTS)).astype(np.int32))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("knn", KNNS)
def test_knn_rows_dims_and_counts(E, eng, oracle, grid_data, knn):
    for dim in DIMS:
        codes, clab, x, xlab = grid_data[dim]
        for rows in ROWS:
            want = witness(oracle, codes[:rows], clab[:rows], x, xlab, knn)
            assert (want[3] == min(knn, rows)).all()
            cb = E.Codebook(eng, codes[:rows], labels=clab[:rows])
            ds = E.Dataset(eng, x, labels=xlab)
            try:
                for count in COUNTS:
                    same(E.knn_vote(cb, ds, 0, count, knn=knn), want[:, :count],
                         "knn %d, %d rows, dim %d, %d samples" % (knn, rows, dim, count))
            finally:
                cb.close()
                ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (5, 9))
def test_two_chunks_and_a_wrapping_run(E, eng, oracle, knn):
    """4097 samples are a chunk of 4096 and one more (both routes); a run past the data's end wraps to its first rows"""
    rs = np.random.RandomState(11)
    codes = rs.standard_normal((70, 3)).astype(np.float32)
    clab = rs.randint(0, 3, 70).astype(np.int32)
    x = rs.standard_normal((4097, 3)).astype(np.float32)
    xlab = rs.randint(0, 3, 4097).astype(np.int32)
    want = witness(oracle, codes, clab, x, xlab, knn)
    cb = E.Codebook(eng, codes, labels=clab)
    ds = E.Dataset(eng, x, labels=xlab)
    try:
        eng.timing(True)
        eng.timing_reset()
        same(E.knn_vote(cb, ds, knn=knn), want, "4097 samples, knn %d" % knn)
        n, ms = eng.knn_vote_timing()["k_knn_vote"]
        assert n == 2 and ms > 0.0
        assert "k_knn_vote" not in eng.timing_table()                   # the published kernel table is closed
        eng.timing(False)
        win = (4090 + np.arange(20)) % 4097
        same(E.knn_vote(cb, ds, 4090, 20, knn=knn), want[:, win], "wrap, knn %d" % knn)
    finally:
        eng.timing(False)
        cb.close()
        ds.close()


def line_codes(order):
    """one-dimensional rows around a sample at 0 such that row order[j] is its j-th nearest (distance j + 1)"""
    codes = np.zeros((len(order), 1), dtype=np.float32)
    codes[np.asarray(order), 0] = 1.0 + np.arange(len(order))
    return codes


@pytest.mark.gpu
def test_label_patterns(E, eng, oracle):
    x = np.zeros((1, 1), dtype=np.float32)
    xlab = np.array([7], dtype=np.int32)
    rs = np.random.RandomState(2)

    def run(seq, knn, order=None):
        """the vote of the sample over rows whose labels, nearest first, are seq"""
        order = rs.permutation(len(seq)) if order is None else order
        clab = np.zeros(len(seq), dtype=np.int32)
        clab[order] = seq
        codes = line_codes(order)
        got = vote(E, eng, codes, clab, x, xlab, knn)
        same(got, witness(oracle, codes, clab, x, xlab, knn), "labels %s, knn %d" % (seq, knn))
        return tuple(int(g[0]) for g in got)

    # all rows one label; all labels different: the head is the nearest's
    assert run([4] * 12, 12) == (4, 12, 0, 12)
    assert run([7] * 12, 5) == (7, 5, 5, 5)
    assert run(list(range(30, 10, -1)), 20) == (30, 1, 0, 20)
    assert run(list(range(300, 0, -1)), 256) == (300, 1, 0, 256)
    # two and three classes tied at the largest count, then four: smallest label 2, largest 9, nearest 5 -- the head is 7,
    # the first to reach the count
    assert run([5, 7, 2, 9, 7, 5], 6) == (7, 2, 2, 6)
    assert run([5, 7, 2, 9, 7, 2, 5], 7) == (7, 2, 2, 7)
    assert run([5, 7, 2, 9, 7, 2, 9, 5], 8) == (7, 2, 2, 8)
    assert run([5, 7, 2, 9, 7, 2, 9, 5], 4) == (5, 1, 1, 4)               # ... cut before any count reaches 2
    assert run([5, 7, 2, 9, 7, 2, 9, 5, 9], 9) == (9, 3, 2, 9)            # a later third hit takes the head
    # the same across the lanes' strides: ties whose second hits lie beyond neighbour 64 and 128
    far = [5, 7, 2, 9] + list(range(100, 160)) + [2, 9] + list(range(200, 270)) + [7, 5, 9, 2]
    assert run(far, len(far)) == (9, 3, 2, len(far))
    assert run(far, 130) == (2, 2, 1, 130)
    assert run([5, 7] + list(range(300, 430)) + [7, 5], 134) == (7, 2, 2, 134)
    # label 0 is a label like any other
    assert run([0, 3, 0, 3, 3, 0], 6) == (3, 3, 0, 6)
    assert run([0, 3, 0, 3], 4) == (0, 2, 0, 4)
    # equal rows with different labels: the later row comes first
    codes = np.ones((4, 1), dtype=np.float32)
    clab = np.array([1, 1, 2, 2], dtype=np.int32)
    for knn, head in ((4, (2, 2)), (3, (2, 2)), (1, (1, 1))):               # knn 1 is find_winner_euc: the first row
        got = vote(E, eng, codes, clab, x, xlab, knn)
        same(got, witness(oracle, codes, clab, x, xlab, knn), "equal rows, knn %d" % knn)
        assert (got[0][0], got[1][0]) == head


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (1, 5, 9, 64))
def test_masked_data_and_no_data_labels(E, eng, oracle, knn):
    rs = np.random.RandomState(31)
    codes = rs.standard_normal((300, 7)).astype(np.float32)
    clab = rs.randint(0, 5, 300).astype(np.int32)
    x = rs.standard_normal((35, 7)).astype(np.float32)
    xlab = rs.randint(0, 5, 35).astype(np.int32)
    mask = (rs.random_sample((35, 7)) < 0.3).astype(np.uint8)
    mask[4] = 1
    mask[4, 2] = 0                               # a single live component
    mask[11] = 1                                 # nothing live: no neighbours
    mask[20] = 0
    got = vote(E, eng, codes, clab, x, xlab, knn, mask=mask)
    same(got, witness(oracle, codes, clab, x, xlab, knn, mask), "masked, knn %d" % knn)
    assert tuple(g[11] for g in got) == (-1, 0, 0, 0)
    assert (np.delete(got[3], 11) == knn).all()
    got = vote(E, eng, codes, clab, x, None, knn, mask=mask)
    same(got, witness(oracle, codes, clab, x, None, knn, mask), "masked, no data labels, knn %d" % knn)
    assert (got[2] == -1).all()
    got = vote(E, eng, codes, clab, x, None, knn)
    same(got, witness(oracle, codes, clab, x, None, knn), "no data labels, knn %d" % knn)
    assert (got[2] == -1).all()


@pytest.mark.gpu
def test_patch_storage(E, eng, oracle):
    """a 16 x 8 hexa map is stored in 8x8 patches: the keys' units, not the storage rows, find the labels"""
    rs = np.random.RandomState(77)
    codes = rs.randint(-3, 4, size=(128, 6)).astype(np.float32)
    clab = rs.randint(0, 4, 128).astype(np.int32)
    x = rs.randint(-3, 4, size=(33, 6)).astype(np.float32)
    xlab = rs.randint(0, 4, 33).astype(np.int32)
    for knn in (5, 20):
        got = vote(E, eng, codes, clab, x, xlab, knn, topol=TOPOL_HEXA, neigh=1, xdim=16, ydim=8)
        same(got, witness(oracle, codes, clab, x, xlab, knn), "8x8-patch map, knn %d" % knn)


@pytest.mark.gpu
def test_prefilter_route_gives_the_direct_answer(E, eng):
    """4096 x 32 against 256 samples at knn 5 takes the top-8 search behind the bf16 pre-filter (tests/test_scan_routes.py:
    rows4096_k3_fw); the vote behind its keys is the direct scan's"""
    rs = np.random.RandomState(12)
    codes = rs.standard_normal((4096, 32)).astype(np.float32)
    clab = rs.randint(0, 6, 4096).astype(np.int32)
    x = rs.standard_normal((256, 32)).astype(np.float32)
    xlab = rs.randint(0, 6, 256).astype(np.int32)
    want = vote(E, eng, codes, clab, x, xlab, 5)
    e2 = E.Engine(0)
    try:
        e2.set_scan_mode("mfma_bf16")
        cb = E.Codebook(e2, codes, labels=clab)
        ds = E.Dataset(e2, x, labels=xlab)
        assert E.scan_plan(cb, ds, 256, 8)["route"] in ("one_level", "two_level")
        got = E.knn_vote(cb, ds, knn=5)
    finally:
        e2.close()
    same(got, np.stack(want), "mfma_bf16")
    assert (got[3] == 5).all() and (got[1] >= 1).all()


@pytest.mark.gpu
def test_refusals(E, eng):
    from som_lvq_pak_amd import _lib
    rs = np.random.RandomState(1)
    codes = rs.standard_normal((128, 3)).astype(np.float32)
    clab = rs.randint(0, 3, 128).astype(np.int32)
    ds = E.Dataset(eng, rs.standard_normal((10, 3)).astype(np.float32))
    cb = E.Codebook(eng, codes, labels=clab)
    bare = E.Codebook(eng, codes)
    shard = E.Codebook(eng, codes[:64], labels=clab[:64], row_offset=0, n_global=128)
    shard2 = E.Codebook(eng, codes[64:], labels=clab[64:], row_offset=64, n_global=128)
    try:
        for knn, text in ((257, "somhip_knn_vote: knn 257 not in 1..256"), (0, "somhip_knn_vote: knn 0 not in 1..256")):
            with pytest.raises(_lib.SomhipError, match=text):
                E.knn_vote(cb, ds, knn=knn)
        with pytest.raises(_lib.SomhipError, match="somhip_knn_vote: codebook has no labels"):
            E.knn_vote(bare, ds, knn=5)
        for s in (shard, shard2):
            with pytest.raises(_lib.SomhipError, match="somhip_knn_vote: sharded codebook not supported"):
                E.knn_vote(s, ds, knn=5)
        out = np.zeros(10, np.int32)
        assert eng.lib.somhip_knn_vote(cb.h, ds.h, 0, 10, 5, None, None, None, None) != 0
        assert eng.lib.somhip_last_error().decode() == "somhip_knn_vote: null output"
        # freq, own and found may be NULL
        assert eng.lib.somhip_knn_vote(cb.h, ds.h, 0, 10, 5, out.ctypes.data_as(_lib.c_i32_p), None, None, None) == 0
        assert np.array_equal(out, E.knn_vote(cb, ds, knn=5)[0])
    finally:
        for h in (cb, bare, shard, shard2, ds):
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knn", (5, 9))
def test_find_winners_is_unchanged(E, eng, oracle, knn):
    """the search both entry points share still answers find_winners as the oracle does, before and after a vote"""
    rs = np.random.RandomState(8)
    codes = rs.standard_normal((300, 5)).astype(np.float32)
    clab = rs.randint(0, 4, 300).astype(np.int32)
    x = rs.standard_normal((33, 5)).astype(np.float32)
    widx, wdiff, wret = oracle.winners(codes, x, knn, True, None)
    cb = E.Codebook(eng, codes, labels=clab)
    ds = E.Dataset(eng, x)
    try:
        for _ in range(2):
            idx, diff, ret = E.find_winners(cb, ds, knn=knn, tie=TIE_KNN)
            assert np.array_equal(idx, widx.astype(np.int32)) and np.array_equal(ret, wret)
            assert np.array_equal(diff.view(np.uint32), wdiff.astype(np.float32).view(np.uint32))
            E.knn_vote(cb, ds, knn=knn)
    finally:
        cb.close()
        ds.close()
