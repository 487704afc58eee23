"""Masked LVQ training in the exact batched engine (kernels/lvq_batch.hpp, the MASKED instantiations), one GPU and
row-sharded.

Every comparison is bit for bit: codebook bytes, OLVQ1 rates, winner indices, the bit patterns of the winners'
distances.  The witnesses are (a) the per-iteration path of the same engine (SOMHIP_LVQ_ONLINE=1 in a child process),
(b) what the REAL reference wrote for the same input files (tests/golden/masked and tests/golden/masked_batch, md5 only)
and, where oracle/_ref is built, (c) the reference's tools run on the spot.  somhip_lvq_stats proves which engine ran:
its counters only move in the batched engine."""
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, synth
from som_lvq_pak_amd import textio

MASKED = os.path.join(GOLDEN, "masked")
EXPECTED = json.load(open(os.path.join(MASKED, "expected.json")))
BATCH_EXPECTED = json.load(open(os.path.join(GOLDEN, "masked_batch", "expected.json")))
BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
REF = os.path.join(ROOT, "oracle", "_ref")
KINDS = (1, 2, 3, 4)                                           # LVQ1, OLVQ1, LVQ2.1, LVQ3


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ CPU: the code object
def test_masked_walk_and_adjacency_are_in_the_code_object_and_the_walk_has_no_fma(tmp_path):
    """The masked instantiations of the walk, of relation (*) and of rho exist for gfx950, and the body of the masked
    walk holds no v_fma / v_fmac / v_mac / v_mad _f32: its distances and corrections are the reference's separate
    sub / mul / add roundings (the method of test_build.py::test_exact_kernels_have_no_fma; a function body here ends at
    its .Lfunc_end label, so that the out-of-line quotient lvq_div_call, which ends in a return, stays apart)."""
    s = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                           "-ffp-contract=off", "--cuda-device-only", "-S", "-o", s,
                           os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")])
    txt = open(s).read()
    bodies = dict(re.findall(r"^(_ZN6somhip\w+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M))
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, flags=re.M))

    def one(prefix):
        names = [k for k in bodies if k.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        assert names[0] in kernels, names[0]                   # a kernel of the code object, not a helper
        return bodies[names[0]]

    fma = r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)_f32\b.*"
    for masked in ("Lb0", "Lb1"):
        one("_ZN6somhip14k_lvq_pair_adjI" + masked)
        one("_ZN6somhip16k_lvq_sample_rhoI" + masked)
    one("_ZN6somhip17k_lvq_batch_applyILb0")
    walk = one("_ZN6somhip17k_lvq_batch_applyILb1")
    assert "s_endpgm" in walk
    assert not re.findall(fma, walk), re.findall(fma, walk)[:3]
    assert re.search(r"v_(pk_)?mul_f32", walk) and re.search(r"v_(pk_)?add_f32", walk) and re.search(r"v_cndmask_b32", walk)
    assert not re.findall(fma, one("_ZN6somhip14k_lvq_pair_adjILb1"))
    # the quotients of the masked walk: one out-of-line IEEE division, nothing else
    div = [b for k, b in bodies.items() if "lvq_div_call" in k]
    assert len(div) == 1 and "v_div_fixup_f32" in div[0] and "s_setpc_b64" in div[0]
    assert "lvq_div_call" in walk


def test_fixtures_of_the_larger_case_are_made_again_from_the_seed(tmp_path):
    gen = _load("make_golden_masked_batch")
    gen.write_case(str(tmp_path))
    for f, want in BATCH_EXPECTED["data"].items():
        assert md5(os.path.join(str(tmp_path), f)) == want, f
    e, _ = textio.read_entries(os.path.join(str(tmp_path), "mix_masked.dat"), skip_empty=False)
    assert e.points.shape == (gen.ROWS, gen.DIM) and 0.08 < e.mask.mean() < 0.12 and not e.mask.all(axis=1).any()
    assert sorted(BATCH_EXPECTED["runs"]) == ["lvq1", "lvq2", "lvq3", "olvq1"]


# ------------------------------------------------------------------ GPU: batched against per-iteration
_TRAIN_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from som_lvq_pak_amd import engine as E

z = np.load(sys.argv[1])
eng = E.Engine(0)
ds = E.Dataset(eng, z["x"], mask=z["mask"], labels=z["lab"])
length = int(z["length"])
out = {}
for kind in (1, 2, 3, 4):
    cb = E.Codebook(eng, z["codes"], labels=z["clab"])
    s0 = eng.lvq_stats()
    ta, ti, td = E.lvq_train(cb, ds, kind, length, 0.3 if kind == 2 else 0.05, winlen=0.3 if kind >= 3 else 0.0,
                             epsilon=0.1 if kind == 4 else 0.0)
    s1 = eng.lvq_stats()
    out["cod%%d" %% kind] = cb.download()
    out["ti%%d" %% kind], out["td%%d" %% kind] = ti, td
    if kind == 2:
        out["ta"] = ta
    out["stats%%d" %% kind] = np.array([s1[k] - s0[k] for k in ("batches", "samples", "stop_list", "stop_cache", "components")],
                                     dtype=np.int64)
    cb.close()
ds.close()
eng.close()
np.savez(sys.argv[2], **out)
print("CHILD DONE")
''' % ROOT


def _train_both(tmp_path, codes, clab, x, mask, lab, length):
    """the four algorithms through somhip_lvq_train, each in its own child process: the default (batched) engine and
    SOMHIP_LVQ_ONLINE=1 (one k_lvq_online_step<true> launch per iteration)"""
    src = os.path.join(str(tmp_path), "in.npz")
    np.savez(src, codes=codes, clab=clab.astype(np.int32), x=x, mask=mask.astype(np.uint8), lab=lab.astype(np.int32),
             length=np.int64(length))
    got = {}
    for tag, env in (("batched", {}), ("online", {"SOMHIP_LVQ_ONLINE": "1"})):
        dst = os.path.join(str(tmp_path), tag + ".npz")
        child_env = {k: v for k, v in os.environ.items() if k != "SOMHIP_LVQ_ONLINE"}
        p = subprocess.run([sys.executable, "-c", _TRAIN_CHILD, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=900, env=dict(child_env, **env))
        assert p.returncode == 0 and "CHILD DONE" in p.stdout, (tag, p.stdout[-2000:], p.stderr[-3000:])
        got[tag] = dict(np.load(dst))
    return got["batched"], got["online"]


def _assert_same_run(b, o, length):
    """batched == per-iteration, bit for bit; the batched engine ran every iteration, the witness none"""
    for kind in KINDS:
        assert np.array_equal(b["ti%d" % kind], o["ti%d" % kind]), kind
        assert np.array_equal(bits(b["td%d" % kind]), bits(o["td%d" % kind])), kind
        assert np.array_equal(bits(b["cod%d" % kind]), bits(o["cod%d" % kind])), kind
        batches, samples, stop_list, stop_cache, comps = (int(v) for v in b["stats%d" % kind])
        print("kind %d: batches %d samples %d cut short %d + %d components %d" % (kind, batches, samples, stop_list, stop_cache, comps))
        assert samples == length and batches > 0 and comps >= batches, (kind, b["stats%d" % kind])
        assert not o["stats%d" % kind].any(), (kind, o["stats%d" % kind])
    assert np.array_equal(bits(b["ta"]), bits(o["ta"]))


def _garbage(x, mask, seed):
    """what a Dataset made from Python may hold at masked positions: NaN and 1e30"""
    rs = np.random.RandomState(seed)
    xs = x.copy()
    xs[mask != 0] = np.where(rs.random_sample(int((mask != 0).sum())) < 0.5, np.nan, 1e30).astype(np.float32)
    return xs


def _mixture_case(seed, n, d, m, classes, frac, spread=4.0):
    """a seeded mixture of `classes` blobs; codes = data rows plus a little noise, with exact duplicates (ties)"""
    x, lab = synth(seed, m, d, k=classes, spread=spread)
    rs = np.random.RandomState(seed + 1)
    pick = rs.randint(0, m, n)
    codes = (x[pick] + 0.05 * rs.standard_normal((n, d))).astype(np.float32)
    codes[n // 2:n // 2 + 8] = codes[:8]
    clab = lab[pick].copy()
    clab[n // 2:n // 2 + 8] = clab[:8]
    mask = (rs.random_sample((m, d)) < frac).astype(np.uint8)
    mask[mask.all(axis=1), 0] = 0                              # no fully masked row
    return codes, clab, x, mask, lab


# dims: not a multiple of 4 (13), of 4 but not 8 (20), of 8 (64, 256); codebooks of 200, 4096 and 10 000 rows; mask
# fractions 0.02, 0.15 and 0.6
SHAPES = [(200, 13, 700, 6, 0.15, 2000), (200, 20, 900, 6, 0.6, 2000), (4096, 20, 1500, 40, 0.02, 3000),
          (4096, 64, 1500, 40, 0.6, 3000), (4096, 13, 1200, 20, 0.6, 2500), (10000, 64, 2000, 100, 0.02, 3000)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m,classes,frac,length", SHAPES)
def test_batched_masked_equals_per_iteration(tmp_path, n, d, m, classes, frac, length):
    codes, clab, x, mask, lab = _mixture_case(n + d, n, d, m, classes, frac)
    b, o = _train_both(tmp_path, codes, clab, _garbage(x, mask, d), mask, lab, length)
    _assert_same_run(b, o, length)


@pytest.mark.gpu
def test_batched_masked_equals_per_iteration_at_10000_x_256(tmp_path):
    """the shape of DESIGN.md's table; batches cut short are redone by the repair path and must stay the exception here:
    fewer than half of them"""
    n, d, m, length = 10000, 256, 4000, 4000
    codes, clab, x, mask, lab = _mixture_case(77, n, d, m, 100, 0.15)
    b, o = _train_both(tmp_path, codes, clab, _garbage(x, mask, 5), mask, lab, length)
    _assert_same_run(b, o, length)
    for kind in KINDS:
        batches, _, stop_list, stop_cache, _ = (int(v) for v in b["stats%d" % kind])
        assert 2 * (stop_list + stop_cache) < batches, (kind, b["stats%d" % kind])


@pytest.mark.gpu
def test_masked_relation_separates_the_samples(tmp_path):
    """somhip_lvq_stats after a masked somhip_lvq_train: batches and components grew, and on well separated blobs the
    masked relation (*) leaves more than one component per batch (the walk did not degrade to the serial one)"""
    n, d, m, length = 4096, 64, 2000, 4000
    codes, clab, x, mask, lab = _mixture_case(909, n, d, m, 50, 0.15, spread=6.0)
    b, o = _train_both(tmp_path, codes, clab, _garbage(x, mask, 9), mask, lab, length)
    _assert_same_run(b, o, length)
    for kind in KINDS:
        batches, _, _, _, comps = (int(v) for v in b["stats%d" % kind])
        assert comps > batches, (kind, b["stats%d" % kind])


@pytest.mark.gpu
def test_blocks_of_samples_that_share_no_component(tmp_path):
    """odd samples see components 0..31 only, even samples 32..63 only: every odd-even pair has an empty intersection,
    which relation (*) must take for an edge (distance 0 over nothing)"""
    n, d, m, length = 4096, 64, 1200, 2500
    codes, clab, x, mask, lab = _mixture_case(321, n, d, m, 30, 0.05)
    mask[0::2, :32] = 1
    mask[1::2, 32:] = 1
    b, o = _train_both(tmp_path, codes, clab, _garbage(x, mask, 3), mask, lab, length)
    _assert_same_run(b, o, length)


@pytest.mark.gpu
def test_a_single_masked_sample_in_the_run_and_stored_values_do_not_matter(tmp_path):
    """one sample of the whole run carries a mask (three components); and whatever the data rows store at masked
    positions -- NaN and 1e30 here, 0 there -- the results are the same bits"""
    n, d, m, length = 4096, 64, 1200, 2500
    codes, clab, x, mask, lab = _mixture_case(654, n, d, m, 30, 0.0)
    mask[:] = 0
    mask[417, [0, 17, 63]] = 1
    os.mkdir(str(tmp_path / "a"))
    os.mkdir(str(tmp_path / "b"))
    b, o = _train_both(tmp_path / "a", codes, clab, _garbage(x, mask, 1), mask, lab, length)
    _assert_same_run(b, o, length)
    x0 = x.copy()
    x0[mask != 0] = 0.0
    b0, _ = _train_both(tmp_path / "b", codes, clab, x0, mask, lab, length)
    for k in b:
        if not k.startswith("stats"):
            assert np.array_equal(b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k],
                                  b0[k].view(np.uint32) if b0[k].dtype == np.float32 else b0[k]), k


# ------------------------------------------------------------------ GPU: the three-call protocol over row shards
_SHARDED_CHILD = r'''
import ctypes as C
import sys
import numpy as np
import torch
torch.zeros(1, device="cuda")
sys.path.insert(0, %r)
from som_lvq_pak_amd import engine as E, sharded
from som_lvq_pak_amd._lib import LvqParams

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

class LocalLvqGroup:
    """the shards of one codebook held in one process; the two collectives by hand (stack = all-gather, integer sum =
    all-reduce), so that every step runs the real kernels on one GPU"""
    def __init__(self, eng, shards, kind, mk_params):
        self.parts = [sharded.GpuLvqShard(eng, cb, ds, mk_params, kind) for cb, ds in shards]
    def topk_keys(self, first, count):
        return torch.stack([p.topk_keys(first, count) for p in self.parts], dim=0)
    def merge(self, gathered, count):
        g = gathered[0] if gathered.dim() == 4 else gathered
        outs = [p.merge(g, count) for p in self.parts]
        assert all(torch.equal(outs[0], o) for o in outs[1:])
        return outs[0]
    def candidates(self, keys, count, xrows):
        got = [p.candidates(keys, count, xrows) for p in self.parts]
        lab = sum(g[0].view(torch.int32) for g in got)
        ta = None if got[0][1] is None else sum(g[1].view(torch.int32) for g in got).view(torch.float32)
        rows = sum(g[2].view(torch.int32) for g in got).view(torch.float32)
        return lab, ta, rows
    def apply(self, it0, count, first, keys, lab, ta, rows, xrows):
        res = [p.apply(it0, count, first, keys, lab, ta, rows, xrows) for p in self.parts]
        assert all(r[0] == res[0][0] for r in res)
        assert all(np.array_equal(r[1], res[0][1]) and np.array_equal(bits(r[2]), bits(res[0][2])) for r in res)
        return res[0]
    def collective_scope(self):
        import contextlib
        return contextlib.nullcontext()

z = np.load(sys.argv[1])
codes, clab, x, mask, lab = z["codes"], z["clab"], z["x"], z["mask"], z["lab"]
n, m, length = codes.shape[0], x.shape[0], int(z["length"])
eng = E.Engine(0)
ok = True
if sys.argv[2] == "equal":
    ds = E.Dataset(eng, x, mask=mask, labels=lab)
    for kind in (1, 2, 3, 4):
        alpha = 0.3 if kind == 2 else 0.05
        kw = dict(winlen=0.3 if kind >= 3 else 0.0, epsilon=0.1 if kind == 4 else 0.0)
        whole = E.Codebook(eng, codes, labels=clab)
        wta, wti, wtd = E.lvq_train(whole, ds, kind, length, alpha, **kw)       # somhip_lvq_train, unsharded
        want = whole.download()
        whole.close()
        for cuts in ([0, 400, n], [0, 260, 700, n]):
            shards = []
            for a, b in zip(cuts, cuts[1:]):
                cb = E.Codebook(eng, codes[a:b], labels=clab[a:b], row_offset=a, n_global=n)
                if kind == 2:
                    ta0 = np.full(b - a, alpha, dtype=np.float32)
                    E.check(eng.lib.somhip_lvq_rates_upload(cb.h, ta0.ctypes.data_as(C.POINTER(C.c_float))))
                shards.append((cb, ds))
            mk = lambda: LvqParams(kind, length, alpha, 1, kw["winlen"], kw["epsilon"], 0, 0, 0)
            lv = sharded.ShardedLvq(LocalLvqGroup(eng, shards, kind, mk), kind, m, xrows=4, max_batch=512)
            ti, td = lv.train(length)
            got = np.concatenate([cb.download() for cb, _ in shards])
            good = np.array_equal(ti, wti) and np.array_equal(bits(td), bits(wtd)) and np.array_equal(bits(got), bits(want))
            if kind == 2:
                tal = []
                for cb, _ in shards:
                    t = np.empty(cb.n, dtype=np.float32)
                    E.check(eng.lib.somhip_lvq_rates_download(cb.h, t.ctypes.data_as(C.POINTER(C.c_float))))
                    tal.append(t)
                good = good and np.array_equal(bits(np.concatenate(tal)), bits(wta))
            print("kind", kind, "shards", len(shards), "batches", lv.batches, "ok", good)
            ok = ok and good
            for cb, _ in shards:
                cb.close()
    ds.close()
else:
    # a fully masked row (7) in the batch: somhip_lvq_batch_apply refuses the batch; a batch beside it runs
    bad = mask.copy()
    bad[7] = 1
    ds = E.Dataset(eng, x, mask=bad, labels=lab)
    cb = E.Codebook(eng, codes, labels=clab, row_offset=0, n_global=n)
    mk = lambda: LvqParams(1, length, 0.05, 1, 0.0, 0.0, 0, 0, 0)
    grp = LocalLvqGroup(eng, [(cb, ds)], 1, mk)
    lv = sharded.ShardedLvq(grp, 1, m, xrows=4, max_batch=512)
    try:
        lv.batch(0, 0, 64)
        print("no refusal")
        ok = False
    except Exception as ex:
        print("refused:", ex)
        ok = ok and "somhip_lvq_batch_apply" in str(ex) and "row 7 has every component masked" in str(ex)
    ok = ok and np.array_equal(bits(cb.download()), bits(codes))             # nothing was applied
    done, ti, td = lv.batch(8, 8, 64)                                         # rows 8..71
    ok = ok and 0 < done <= 64
    print("after the refusal: consumed", done)
    cb.close()
    ds.close()
eng.close()
print("RESULT", ok)
''' % ROOT


def _run_sharded_child(tmp_path, mode, codes, clab, x, mask, lab, length):
    src = os.path.join(str(tmp_path), "in.npz")
    np.savez(src, codes=codes, clab=clab.astype(np.int32), x=x, mask=mask.astype(np.uint8), lab=lab.astype(np.int32),
             length=np.int64(length))
    p = subprocess.run([sys.executable, "-c", _SHARDED_CHILD, src, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    print(p.stdout[-3000:])
    return p


@pytest.mark.gpu
def test_batch_apply_takes_masked_data_over_two_and_three_row_shards(tmp_path):
    """somhip_lvq_batch_apply on a masked data set returns 0, and the three-call protocol over 2 and 3 row shards leaves
    the codebook, rates and traces of somhip_lvq_train on the unsharded codebook, for all four algorithms.  In a child
    process: torch's HIP runtime has to come up before the engine's."""
    n, d, m, length = 900, 50, 1500, 2500
    codes, clab, x, mask, lab = _mixture_case(4321, n, d, m, 12, 0.15, spread=2.5)
    p = _run_sharded_child(tmp_path, "equal", codes, clab, _garbage(x, mask, 2), mask, lab, length)
    assert "RESULT True" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])


# ------------------------------------------------------------------ GPU: a fully masked row
@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("masked_data")
    _load("make_golden_masked").write_masked_data(str(out))
    return str(out)


@pytest.mark.gpu
def test_a_fully_masked_row_is_refused_by_both_entry_points_and_the_engine_goes_on(tmp_path, data_dir):
    from som_lvq_pak_amd import engine as E
    tab = textio.LabelTable()
    x1, _ = textio.read_entries(os.path.join(data_dir, "ex1_masked.dat"), tab)
    ini, _ = textio.read_entries(os.path.join(MASKED, "eveninit_knn5.cod"), tab)
    lab, clab = x1.first_label.astype(np.int32), ini.first_label.astype(np.int32)
    # somhip_lvq_batch_apply (in a child: the shard object works on torch tensors)
    p = _run_sharded_child(tmp_path, "refuse", ini.points, clab, x1.points, x1.mask, lab, 5000)
    assert "RESULT True" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])
    # somhip_lvq_train
    eng = E.Engine(0)
    bad = x1.mask.copy()
    bad[7] = 1
    cb = E.Codebook(eng, ini.points, labels=clab)
    ds = E.Dataset(eng, x1.points, mask=bad, labels=lab)
    with pytest.raises(Exception, match="row 7 has every component masked"):
        E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, trace=False)
    assert np.array_equal(bits(cb.download()), bits(ini.points))        # nothing was trained
    assert eng.lvq_stats()["samples"] == 0
    E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, start_iter=0, count=5, data_first=0, trace=False)     # never reaches row 7
    assert eng.lvq_stats()["samples"] == 5
    ds.close()
    cb.upload(ini.points)
    ds = E.Dataset(eng, x1.points, mask=x1.mask, labels=lab)
    E.lvq_train(cb, ds, E.LVQ1, 5000, 0.05, trace=False)
    assert eng.lvq_stats()["samples"] == 5005                            # the batched engine, every iteration
    ini.points = cb.download()
    out = str(tmp_path / "lvq1.cod")
    textio.write_entries(out, ini, tab)
    assert md5(out) == EXPECTED["runs"]["lvq1"]["md5"]                   # the reference's bytes
    ds.close()
    cb.close()
    eng.close()


# ------------------------------------------------------------------ GPU: the tools, byte for byte
@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("lvqtrain", "lvq1", "olvq1", "lvq2", "lvq3")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["lvq1", "olvq1", "lvq2", "lvq3"])
def test_lvqtrain_gpus_on_masked_data_gives_the_reference_bytes(tools, tmp_path, data_dir, tag):
    """lvqtrain -gpus 2 on ex1_masked.dat: two row blocks, one process each (sharing this machine's GPU), the masks in
    every rank's data set.  The bytes the reference wrote (tests/golden/masked/expected.json)."""
    r = EXPECTED["runs"][tag]
    out = tmp_path / "out.cod"
    p = subprocess.run([os.path.join(BIN, "lvqtrain"), "-type", r["tool"], "-din", os.path.join(data_dir, r["din"]),
                        "-cin", os.path.join(MASKED, r["cin"]), "-cout", str(out)] + [str(a) for a in r["args"]] +
                       ["-gpus", "2", "-v", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr
    assert md5(out) == r["md5"]
    assert not os.path.exists(str(out)[:-4] + ".lra")


@pytest.fixture(scope="module")
def mix_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("mix")
    _load("make_golden_masked_batch").write_case(str(out))
    return str(out)


def _tool(exe, mix_dir, out, args):
    p = subprocess.run([exe, "-din", os.path.join(mix_dir, "mix_masked.dat"), "-cin", os.path.join(mix_dir, "mix.cod"),
                        "-cout", str(out)] + [str(a) for a in args] + ["-v", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (exe, p.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["lvq1", "olvq1", "lvq2", "lvq3"])
def test_larger_masked_case_gives_the_recorded_reference_bytes(tools, tmp_path, mix_dir, tag):
    """2 000 codes x 64 dims, 20 000 iterations, about 10 % masked: the engine's tool writes the bytes the reference
    wrote (md5 recorded by tests/golden/make_golden_masked_batch.py); the same run through the library shows in
    somhip_lvq_stats that the batched engine took every iteration, and gives the same file."""
    from som_lvq_pak_amd import engine as E
    r = BATCH_EXPECTED["runs"][tag]
    out = tmp_path / "out.cod"
    _tool(os.path.join(BIN, r["tool"]), mix_dir, out, r["args"])
    assert md5(out) == r["md5"]
    tab = textio.LabelTable()
    x, _ = textio.read_entries(os.path.join(mix_dir, "mix_masked.dat"), tab)
    ini, _ = textio.read_entries(os.path.join(mix_dir, "mix.cod"), tab)
    a = dict(zip(r["args"][0::2], r["args"][1::2]))
    kind = {"lvq1": E.LVQ1, "olvq1": E.OLVQ1, "lvq2": E.LVQ2, "lvq3": E.LVQ3}[tag]
    eng = E.Engine(0)
    cb = E.Codebook(eng, ini.points, labels=ini.first_label.astype(np.int32))
    ds = E.Dataset(eng, x.points, mask=x.mask, labels=x.first_label.astype(np.int32))
    E.lvq_train(cb, ds, kind, int(a["-rlen"]), float(a["-alpha"]), winlen=float(a.get("-win", 0.0)),
                epsilon=float(a.get("-epsilon", 0.0)), trace=False)
    s = eng.lvq_stats()
    print(tag, s)
    assert s["samples"] == int(a["-rlen"]) and s["batches"] > 0
    ini.points = cb.download()
    out2 = str(tmp_path / "lib.cod")
    textio.write_entries(out2, ini, tab)
    assert md5(out2) == r["md5"]
    ds.close()
    cb.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["lvq1", "olvq1", "lvq2", "lvq3"])
def test_larger_masked_case_equals_the_reference_tools_run_here(tools, tmp_path, mix_dir, tag):
    """the same files through oracle/_ref's own lvq1 / olvq1 / lvq2 / lvq3 (a few CPU seconds) and through the engine's:
    byte-equal codebooks.  Skips where the reference tools were not built; the md5 twin above cannot."""
    exe = os.path.join(REF, tag)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs the reference sources at build time)" % tag)
    r = BATCH_EXPECTED["runs"][tag]
    want, got = tmp_path / "ref.cod", tmp_path / "hip.cod"
    _tool(exe, mix_dir, want, r["args"])
    _tool(os.path.join(BIN, r["tool"]), mix_dir, got, r["args"])
    assert open(str(got), "rb").read() == open(str(want), "rb").read()
