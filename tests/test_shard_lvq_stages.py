"""The stages of LVQ training over a row-sharded codebook, one by one against numpy replays, bit for bit:
somhip_merge_topk_keys (k_merge_shard_topk), somhip_lvq_batch_candidates (k_lvq_cand_meta, k_lvq_cand_rows) and one edge of
somhip_lvq_batch_apply.  The first two take synthetic keys uploaded with somhip_copy_to_device -- no search and no
training loop stand between a wrong word and the assertion that names it.  Every output buffer is filled with 0xA5
bytes before the call, so a word the kernel should have written and did not shows as well.  Needs an MI355X:  pytest -m gpu."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)      # a missing entry of a top-k list (KEY_NONE)
M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def E():
    from som_lvq_pak_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    e = E.Engine(0)
    yield e
    e.close()


class DevBuf:
    """a device buffer of nbytes, filled with 0xA5 bytes or with the array given"""

    def __init__(self, eng, nbytes=None, data=None):
        self.e = eng
        self.nbytes = max(1, int(data.nbytes if data is not None else nbytes))
        self.p = eng.device_alloc(self.nbytes)
        fill = np.ascontiguousarray(data) if data is not None and data.nbytes else np.full(self.nbytes, 0xA5, dtype=np.uint8)
        assert eng.lib.somhip_copy_to_device(eng.h, self.p, fill.ctypes.data_as(C.c_void_p), fill.nbytes) == 0

    def read(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            assert self.e.lib.somhip_copy_to_host(self.e.h, out.ctypes.data_as(C.c_void_p), self.p, out.nbytes) == 0
        return out

    def free(self):
        self.e.device_free(self.p)


def error(eng):
    return eng.lib.somhip_last_error().decode()


# ------------------------------------------------------------------------------------------------ somhip_merge_topk_keys
def merge(eng, gathered, knn=None, n_shards=None, count=None):
    """somhip_merge_topk_keys on gathered [n_shards, count, K] uint64 -> [count, K]"""
    S, m, K = gathered.shape
    src, dst = DevBuf(eng, data=gathered), DevBuf(eng, nbytes=8 * m * K)
    try:
        rc = eng.lib.somhip_merge_topk_keys(eng.h, src.p, S if n_shards is None else n_shards, m if count is None else count,
                                            K if knn is None else knn, dst.p)
        assert rc == 0, error(eng)
        eng.sync()
        return dst.read(np.uint64, (m, K))
    finally:
        src.free()
        dst.free()


def replay_merge(gathered):
    S, m, K = gathered.shape
    return np.sort(gathered.transpose(1, 0, 2).reshape(m, S * K), axis=1)[:, :K]


def pack(bits, tag, inverted):
    """(distance bits << 32) | tag, or | ~tag: the complemented tags of the k-NN tie rule (SOMHIP_TIE_KNN)"""
    tag = np.asarray(tag, dtype=np.uint64)
    return (np.asarray(bits, dtype=np.uint64) << np.uint64(32)) | ((~tag & M32) if inverted else tag)


def random_lists(rs, S, m, K, inverted, nbits=6):
    """per (shard, sample) an ascending list of K keys, unique over the shards (tag = a global row of the shard's own range),
    with few distinct distance bits -- equal distances across and within shards are the rule -- and an all-ones tail of
    (shard + sample) % (K + 1) entries: every length 0 .. K"""
    bits = 0x3F000000 + rs.randint(0, nbits, size=(S, m, K))
    tag = np.arange(S)[:, None, None] * 4096 + (rs.randint(0, 4096, size=(S, m, 1)) + 17 * np.arange(K)[None, None, :]) % 4096
    g = np.sort(pack(bits, tag, inverted), axis=2)
    tail = (np.arange(S)[:, None] + np.arange(m)[None, :]) % (K + 1)
    g[np.arange(K)[None, None, :] >= (K - tail)[:, :, None]] = ALL_ONES
    return g


@pytest.mark.parametrize("inverted", [False, True], ids=["plain_tags", "complemented_tags"])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_merge_topk_equals_sorted_union(eng, K, inverted):
    rs = np.random.RandomState(100 * K + inverted)
    for S in (1, 2, 3, 8, 33):
        for m in (1, 255, 256, 257, 1025):
            g = random_lists(rs, S, m, K, inverted)
            if S > 1:
                g[1] = ALL_ONES                                     # a shard with nothing to offer
            assert (g[:, :, 1:] >= g[:, :, :-1]).all()
            if m > K:                                               # the tails were there, of every length
                assert set(np.unique((g == ALL_ONES).sum(axis=2))) == set(range(K + 1))
            got = merge(eng, g)
            want = replay_merge(g)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, "K %d, %d shards, %d samples: %d differ; first at %d: got %s, want %s" % (
                K, S, m, bad.size, bad[0], [hex(v) for v in got[bad[0]]], [hex(v) for v in want[bad[0]]])


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_merge_topk_patterns(eng, K):
    """every shard empty; a later shard wholly below the first (every insertion shifts the list), wholly above (the early
    exit), and strictly interleaved lists; equal distance bits across shards under both tag forms"""
    m = 300
    j = np.arange(m, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    first = pack(0x40000000 + (7 * j + k) * 1000, 7 * j + k + 5, False)       # [m, K], ascending in k, different per sample
    span = np.uint64((8000 << 32) + 1)                                        # more than a whole list spans
    for S in (2, 3, 8):
        empty = np.full((S, m, K), ALL_ONES, dtype=np.uint64)
        assert (merge(eng, empty) == ALL_ONES).all()
        below = np.stack([first - np.uint64(s) * span for s in range(S)])     # shard s + 1 wholly below shard s
        above = np.stack([first + np.uint64(s) * span for s in range(S)])
        i = np.arange(K)[None, :] * S + np.arange(S)[:, None]                 # [S, K]: shard s holds the s-th of every S keys
        inter = pack(0x40000000 + 3 * i[:, None, :] + j[None, :, :], np.broadcast_to(i[:, None, :], (S, m, K)), False)
        for name, g in (("below", below), ("above", above), ("interleaved", inter)):
            g = np.ascontiguousarray(g)
            assert K == 1 or (g[:, :, 1:] > g[:, :, :-1]).all(), name
            got, want = merge(eng, g), replay_merge(g)
            assert np.array_equal(got, want), (name, S, K)
        assert (below[1:, :, K - 1] < below[:-1, :, 0]).all() and (above[1:, :, 0] > above[:-1, :, K - 1]).all()
        assert np.array_equal(merge(eng, np.ascontiguousarray(below)), below[S - 1])      # the last shard's list, whole
        assert np.array_equal(merge(eng, np.ascontiguousarray(above)), first)
        flat = np.sort(inter.transpose(1, 0, 2).reshape(m, S * K), axis=1)
        assert np.array_equal(flat, inter.transpose(1, 2, 0).reshape(m, S * K))           # (strictly interleaved)
        # one distance for every key: the tags alone order them -- the lowest row first, or (complemented) the highest
        for inverted in (False, True):
            rows = np.broadcast_to(np.arange(S * K).reshape(S, 1, K), (S, m, K))
            g = np.sort(pack(np.full((S, m, K), 0x41200000), rows, inverted), axis=2)
            got = merge(eng, g)
            assert np.array_equal(got, replay_merge(g))
            got_rows = ((~got if inverted else got) & M32).astype(np.int64)
            want_rows = np.arange(S * K - 1, S * K - 1 - K, -1) if inverted else np.arange(K)
            assert np.array_equal(got_rows, np.broadcast_to(want_rows, (m, K)))


def test_merge_topk_refusals(eng):
    g = np.full((2, 4, 8), ALL_ONES, dtype=np.uint64)
    src, dst = DevBuf(eng, data=g), DevBuf(eng, nbytes=8 * 4 * 8)
    try:
        lib = eng.lib
        for knn in (3, 5, 9):
            assert lib.somhip_merge_topk_keys(eng.h, src.p, 2, 4, knn, dst.p) != 0
            assert "knn must be 1, 2, 4 or 8" in error(eng)
        assert lib.somhip_merge_topk_keys(eng.h, src.p, 0, 4, 8, dst.p) != 0
        assert "bad shape" in error(eng)
        assert lib.somhip_merge_topk_keys(eng.h, None, 2, 4, 8, dst.p) != 0
        assert "null argument" in error(eng)
        assert lib.somhip_merge_topk_keys(eng.h, src.p, 2, 4, 8, None) != 0
        assert "null argument" in error(eng)
        assert lib.somhip_merge_topk_keys(eng.h, src.p, 2, 0, 8, dst.p) == 0         # no samples: nothing to do
        eng.sync()
        assert (dst.read(np.uint8, 8 * 4 * 8) == 0xA5).all()                         # ... and nothing written
    finally:
        src.free()
        dst.free()


# ------------------------------------------------------------------------------------------------ somhip_lvq_batch_candidates
N_ROWS = 200
CUTS = [0, 1, 63, 64, 65, 137, N_ROWS]        # a cut at row 1, 63, 64, 65 and an uneven one; shards of 1 row (fewer than 8)
EDGE_ROWS = [0, 1, 2, 62, 63, 64, 65, 66, 127, 128, 136, 137, 138, N_ROWS - 1]
SPECIAL_ROWS = [5, 63, 64, 137]               # rows that hold -0.0 or a NaN (make_codebook)


def make_codebook(d):
    rs = np.random.RandomState(7000 + d)
    codes = rs.standard_normal((N_ROWS, d)).astype(np.float32)
    w = codes.view(np.uint32)
    w[5, 0] = 0x80000000                      # -0.0: a float sum over the shards would lose the sign
    w[64, d - 1] = 0x7FC12345                 # NaN with a payload
    w[137, 0] = 0xFFC00001
    w[63, d // 2] = 0x80000000
    labels = rs.randint(1, 9, size=N_ROWS).astype(np.int32)
    rates = (0.01 + 0.5 * rs.random_sample(N_ROWS)).astype(np.float32)
    return codes, labels, rates


def make_keys(rs, count, kind):
    """[count, 8] synthetic candidate keys: global rows all over the codebook, the rows at the tile and shard edges among
    them; all-ones entries as tails and, since the stage takes every slot on its own, in the middle of a list too"""
    rows = rs.randint(0, N_ROWS, size=(count, 8))
    flat = rows.reshape(-1)
    flat[rs.choice(flat.size, size=min(flat.size, len(EDGE_ROWS)), replace=False)] = EDGE_ROWS[:min(flat.size, len(EDGE_ROWS))]
    missing = rs.random_sample((count, 8)) < 0.15
    if count > 1:
        missing[1] = True                                           # a sample without any candidate
        missing[0] = False
        rows[2:2 + len(SPECIAL_ROWS), 0] = SPECIAL_ROWS             # -0.0 and the NaNs as nearest candidates: always copied
        missing[2:2 + len(SPECIAL_ROWS), 0] = False
    keys = pack(0x3F800000 + rs.randint(0, 1 << 20, size=(count, 8)), rows, kind >= 3)
    keys[missing] = ALL_ONES
    return keys


def replay_candidates(codes, labels, rates, a, b, keys, kind, xrows):
    """what the shard of rows [a, b) writes: (lab [count, 8] int32, ta [count, 8] float32 or None, rows [count, xrows, 4 ceil(d / 4)])"""
    count, d = keys.shape[0], codes.shape[1]
    tag = (keys & M32).astype(np.uint32)
    row = (~tag if kind >= 3 else tag).astype(np.int64)
    mine = (keys != ALL_ONES) & (row >= a) & (row < b)
    safe = np.where(mine, row, 0)
    lab = np.where(mine, labels[safe], 0).astype(np.int32)
    ta = np.where(mine, rates[safe], np.float32(0.0)).astype(np.float32) if kind == 2 else None
    out = np.zeros((count, xrows, 4 * ((d + 3) // 4)), dtype=np.float32)
    out.view(np.uint32)[:, :, :d] = np.where(mine[:, :xrows, None], codes.view(np.uint32)[safe[:, :xrows]], np.uint32(0))
    return lab, ta, out


def run_candidates(eng, cb, keys, kind, xrows, d):
    count = keys.shape[0]
    dpad = 4 * ((d + 3) // 4)
    kb, lb, tb, rb = DevBuf(eng, data=keys), DevBuf(eng, nbytes=4 * count * 8), DevBuf(eng, nbytes=4 * count * 8), \
        DevBuf(eng, nbytes=4 * count * xrows * dpad)
    try:
        rc = eng.lib.somhip_lvq_batch_candidates(cb.h, count, kind, kb.p, xrows, lb.p, tb.p if kind == 2 else None, rb.p)
        assert rc == 0, error(eng)
        eng.sync()
        ta = tb.read(np.float32, (count, 8))
        if kind != 2:
            assert (ta.view(np.uint8) == 0xA5).all()                 # no rates asked for: the buffer is not touched
        return lb.read(np.int32, (count, 8)), ta if kind == 2 else None, rb.read(np.float32, (count, xrows, dpad))
    finally:
        for b in (kb, lb, tb, rb):
            b.free()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("d", [1, 3, 4, 5, 50, 1028])
def test_candidates_equal_replay(E, eng, d):
    codes, labels, rates = make_codebook(d)
    shards = []
    for a, b in zip(CUTS, CUTS[1:]):
        cb = E.Codebook(eng, codes[a:b], labels=labels[a:b], row_offset=a, n_global=N_ROWS)
        E.lvq_rates_upload(cb, rates[a:b])
        shards.append((a, b, cb))
    rs = np.random.RandomState(d)
    try:
        for count in (1, 1024):
            for kind in (1, 2, 3, 4):
                keys = make_keys(rs, count, kind)
                for xrows in (1, 4, 8):
                    where = "d %d, count %d, kind %d, xrows %d" % (d, count, kind, xrows)
                    whole = replay_candidates(codes, labels, rates, 0, N_ROWS, keys, kind, xrows)
                    total = [np.zeros(w.shape, dtype=np.uint32) if w is not None else None for w in whole]
                    for a, b, cb in shards:
                        got = run_candidates(eng, cb, keys, kind, xrows, d)
                        want = replay_candidates(codes, labels, rates, a, b, keys, kind, xrows)
                        for name, g, w in zip(("labels", "rates", "rows"), got, want):
                            assert (g is None) == (w is None), (where, name)
                            if g is None:
                                continue
                            bad = np.argwhere(u32(g) != u32(w))
                            assert bad.size == 0, "%s, shard [%d, %d): %d %s words differ; first at %s: got %#x, want %#x (key %#x)" % (
                                where, a, b, len(bad), name, tuple(bad[0]), u32(g)[tuple(bad[0])], u32(w)[tuple(bad[0])],
                                int(keys[bad[0][0], bad[0][1]]))
                        # the padding components beyond dim are +0.0 (the tiles hold 0 there: k_rows_to_tiles)
                        assert (u32(got[2])[:, :, d:] == 0).all(), where
                        for t, g in zip(total, got):
                            if g is not None:
                                t += u32(g)                          # the all-reduce: a SUM of 32-bit integers
                    # ... which is the gather from the whole codebook, the bits of -0.0 and of the NaNs included
                    for name, t, w in zip(("labels", "rates", "rows"), total, whole):
                        if w is not None:
                            assert np.array_equal(t, u32(w)), (where, name)
    finally:
        for _, _, cb in shards:
            cb.close()


def test_candidates_refusals(E, eng):
    codes, labels, rates = make_codebook(5)
    cb = E.Codebook(eng, codes, labels=labels)
    bare = E.Codebook(eng, codes)
    som = E.Codebook(eng, codes[:64], E.TOPOL_HEXA, E.NEIGH_BUBBLE, 8, 8, labels=labels[:64])     # stored by 8 x 8 patches
    count = 1025
    kb, lb, tb, rb = DevBuf(eng, nbytes=8 * count * 8), DevBuf(eng, nbytes=4 * count * 8), DevBuf(eng, nbytes=4 * count * 8), \
        DevBuf(eng, nbytes=4 * count * 8 * 8)
    try:
        call = eng.lib.somhip_lvq_batch_candidates
        for args, message in (((cb.h, 1025, 1, kb.p, 4, lb.p, None, rb.p), "at most 1024 samples"),
                              ((cb.h, 8, 1, kb.p, 0, lb.p, None, rb.p), "xrows must be 1..8"),
                              ((cb.h, 8, 1, kb.p, 9, lb.p, None, rb.p), "xrows must be 1..8"),
                              ((cb.h, 8, 0, kb.p, 4, lb.p, None, rb.p), "Unknown LVQ type 0"),
                              ((cb.h, 8, 5, kb.p, 4, lb.p, None, rb.p), "Unknown LVQ type 5"),
                              ((bare.h, 8, 1, kb.p, 4, lb.p, None, rb.p), "no labels"),
                              ((cb.h, 8, 2, kb.p, 4, lb.p, tb.p, rb.p), "OLVQ1 needs rates"),          # none uploaded
                              ((som.h, 8, 1, kb.p, 4, lb.p, None, rb.p), "row order"),
                              ((cb.h, 8, 1, None, 4, lb.p, None, rb.p), "null argument"),
                              ((cb.h, 8, 1, kb.p, 4, None, None, rb.p), "null argument"),
                              ((cb.h, 8, 1, kb.p, 4, lb.p, None, None), "null argument")):
            assert call(*args) != 0, message
            assert message in error(eng), (message, error(eng))
        E.lvq_rates_upload(cb, rates)
        assert call(cb.h, 8, 2, kb.p, 4, lb.p, None, rb.p) != 0                                        # rates, but no buffer for them
        assert "OLVQ1 needs rates" in error(eng)
        eng.sync()
        for b in (lb, tb, rb):                                       # a refused call writes nothing
            assert (b.read(np.uint8, b.nbytes) == 0xA5).all()
    finally:
        for b in (kb, lb, tb, rb):
            b.free()
        for c in (cb, bare, som):
            c.close()


# ------------------------------------------------------------------------------------------------ somhip_lvq_batch_apply
# Two shards of a 130 x 5 codebook; the second one's rows lie 100 per component away, so it owns none of any batch's
# candidates: it walks every batch on the exchanged rows alone and commits nothing.  Data rows 0 and 1 are one point with
# code row 0 (wrong label) nearest and code row 1 next: the first iteration pushes row 0 to 1.5 times its distance, behind
# row 1 -- the second sample's winner is its second frozen candidate, whose row xrows = 1 did not exchange, so the first
# batch ends after one iteration (include/somhip.h: "a winner beyond the xrows exchanged rows ends the batch early").
# In a child process: torch's HIP runtime has to come up before the engine's (sharded.GpuLvqShard hands torch tensors over).
_APPLY_CHILD = r'''
import contextlib, os, sys
import ctypes as C
import numpy as np
import torch
torch.cuda.set_device(0); torch.zeros(1, device="cuda")
sys.path.insert(0, %r)
from som_lvq_pak_amd import engine as E, sharded
from som_lvq_pak_amd._lib import LvqParams


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(name, ok, detail=""):
    print("CHECK", name, "ok" if ok else "FAIL " + str(detail), flush=True)


class Group:
    """the shard object sharded.ShardedLvq drives, over the parts of ONE process; the collectives by hand; every batch's
    outcome on every part is kept"""

    def __init__(self, eng, shards, kind, mk):
        self.parts = [sharded.GpuLvqShard(eng, cb, ds, mk, kind) for cb, ds in shards]
        self.batches = []          # (count, [consumed per part], traces equal, the second part's buffers all zero)
        self.idle = True

    def topk_keys(self, first, count):
        return torch.stack([p.topk_keys(first, count) for p in self.parts], dim=0)

    def merge(self, gathered, count):
        g = gathered[0] if gathered.dim() == 4 else gathered
        outs = [p.merge(g, count) for p in self.parts]
        self.merged_equal = all(torch.equal(outs[0], o) for o in outs[1:])
        return outs[0]

    def candidates(self, keys, count, xrows):
        got = [p.candidates(keys, count, xrows) for p in self.parts]
        self.idle = all(int(t.view(torch.int32).abs().max()) == 0 for t in got[1] if t is not None)
        lab = sum(g[0].view(torch.int32) for g in got)
        ta = None if got[0][1] is None else sum(g[1].view(torch.int32) for g in got).view(torch.float32)
        rows = sum(g[2].view(torch.int32) for g in got).view(torch.float32)
        return lab, ta, rows

    def apply(self, it0, count, first, keys, lab, ta, rows, xrows):
        res = [p.apply(it0, count, first, keys, lab, ta, rows, xrows) for p in self.parts]
        same = all(np.array_equal(r[1], res[0][1]) and np.array_equal(bits(r[2]), bits(res[0][2])) for r in res)
        self.batches.append((count, [r[0] for r in res], same, self.idle, self.merged_equal))
        return res[0]

    def collective_scope(self):
        return contextlib.nullcontext()


n, d, m, cut, length, alpha = 130, 5, 150, 65, 200, 0.5
eng = E.Engine(0)
# (LVQ2 / LVQ3 correct both winners of a sample, so they get both rows exchanged: xrows 2)
for kind, xrows in ((1, 1), (2, 1), (3, 2), (4, 2)):
    tag = "kind%%d_xrows%%d" %% (kind, xrows)
    rs = np.random.RandomState(40 + kind)
    x = rs.standard_normal((m, d)).astype(np.float32)
    lab = rs.randint(1, 4, size=m).astype(np.int32)
    pick = rs.randint(2, m, n)
    codes = (x[pick] + 0.3 * rs.standard_normal((n, d))).astype(np.float32)
    clab = lab[pick].copy()
    codes[cut:] += np.float32(100.0)
    x[0] = x[1] = np.float32(10.0)                       # one point, far from every other sample and code row
    lab[0] = lab[1] = 1
    delta = np.array([0.5, -0.25, 0.125, 0.25, -0.5], dtype=np.float32)
    codes[0], clab[0] = x[0] + delta, 2                  # nearest, wrong label: pushed to 1.5 delta
    codes[1], clab[1] = x[0] + np.float32(1.25) * delta, 1
    kw = {"winlen": 0.3} if kind >= 3 else {}
    if kind == 4:
        kw["epsilon"] = 0.15
    whole = E.Codebook(eng, codes, labels=clab)
    ds = E.Dataset(eng, x, labels=lab)
    wta, wi, wd = E.lvq_train(whole, ds, kind, length, alpha, **kw)
    want = whole.download()
    whole.close()
    shards = []
    for a, b in ((0, cut), (cut, n)):
        cb = E.Codebook(eng, codes[a:b], labels=clab[a:b], row_offset=a, n_global=n)
        if kind == 2:
            E.lvq_rates_upload(cb, np.full(b - a, alpha, dtype=np.float32))
        shards.append((cb, ds))
    mk = lambda: LvqParams(kind, length, alpha, 1, kw.get("winlen", 0.0), kw.get("epsilon", 0.0), 0, 0, 0)
    group = Group(eng, shards, kind, mk)
    lv = sharded.ShardedLvq(group, kind, m, xrows=xrows, max_batch=1024)
    try:
        ti, td = lv.train(length)
    except Exception as e:
        check(tag + "_trained", False, repr(e))
        continue
    check(tag + "_trained", True)
    b = group.batches
    check(tag + "_same_consumed_on_both_shards", all(len(set(c)) == 1 for _, c, _, _, _ in b), [(cnt, c) for cnt, c, _, _, _ in b])
    check(tag + "_same_traces_on_both_shards", all(s for _, _, s, _, _ in b), [k for k, t in enumerate(b) if not t[2]])
    check(tag + "_same_merged_keys_on_both_shards", all(t[4] for t in b))
    check(tag + "_second_shard_owns_no_candidate", all(t[3] for t in b), [k for k, t in enumerate(b) if not t[3]])
    if xrows == 1:
        check(tag + "_first_batch_ends_early", b[0][0] == length and b[0][1][0] == 1, b[0][:2])
        check(tag + "_batches_continue_from_consumed", sum(c[0] for _, c, _, _, _ in b) == length and len(b) > 1, len(b))
    check(tag + "_winner_trace", np.array_equal(ti, wi), np.nonzero(ti != wi)[0][:4] if ti.shape == wi.shape else (ti.shape, wi.shape))
    check(tag + "_distance_trace", np.array_equal(bits(td), bits(wd)))
    got = [cb.download() for cb, _ in shards]
    check(tag + "_first_shard_rows", np.array_equal(bits(got[0]), bits(want[:cut])), np.argwhere(bits(got[0]) != bits(want[:cut]))[:4].tolist())
    check(tag + "_second_shard_rows_keep_their_bits", np.array_equal(bits(got[1]), bits(codes[cut:])) and np.array_equal(bits(got[1]), bits(want[cut:])))
    check(tag + "_first_shard_changed", not np.array_equal(bits(got[0]), bits(codes[:cut])))
    if kind == 2:
        tal = []
        for cb, _ in shards:
            t = np.empty(cb.n, dtype=np.float32)
            E.check(eng.lib.somhip_lvq_rates_download(cb.h, t.ctypes.data_as(C.POINTER(C.c_float))))
            tal.append(t)
        check(tag + "_rates", np.array_equal(bits(np.concatenate(tal)), bits(wta)))
        check(tag + "_second_shard_rates_keep_their_bits", np.array_equal(bits(tal[1]), bits(np.full(n - cut, alpha, dtype=np.float32))))
    for cb, _ in shards:
        cb.close()
    ds.close()
print("DONE", flush=True)
'''

APPLY_CHECKS = ["trained", "same_consumed_on_both_shards", "same_traces_on_both_shards", "same_merged_keys_on_both_shards",
                "second_shard_owns_no_candidate", "winner_trace", "distance_trace", "first_shard_rows",
                "second_shard_rows_keep_their_bits", "first_shard_changed"]


def test_apply_on_a_shard_that_owns_no_candidate_and_a_batch_cut_by_xrows():
    p = subprocess.run([sys.executable, "-c", _APPLY_CHILD % (ROOT,)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    lines = [ln.split(None, 3) for ln in p.stdout.splitlines() if ln.startswith("CHECK ")]
    seen = {ln[1]: ln[2:] for ln in lines}
    failed = ["%s: %s" % (name, " ".join(rest[1:])) for name, rest in seen.items() if rest[0] != "ok"]
    assert not failed, (failed, p.stderr[-2000:])
    want = []
    for kind, xrows in ((1, 1), (2, 1), (3, 2), (4, 2)):
        tag = "kind%d_xrows%d_" % (kind, xrows)
        want += [tag + c for c in APPLY_CHECKS]
        if xrows == 1:
            want += [tag + "first_batch_ends_early", tag + "batches_continue_from_consumed"]
        if kind == 2:
            want += [tag + "rates", tag + "second_shard_rates_keep_their_bits"]
    missing = [w for w in want if w not in seen]
    assert not missing and "DONE" in p.stdout, (missing, p.stdout[-2000:], p.stderr[-3000:])
