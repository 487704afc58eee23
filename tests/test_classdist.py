"""mindist and stddev: LVQ_PAK's within-class nearest-neighbour medians, the self-join on the GPU, bit for bit.

The real reference enters through tests/golden/classdist (written by tests/golden/make_golden_classdist.py from the
reference's own mindist.c and stddev.c).  tests/classdist_replay.py restates the reference's arithmetic in numpy; the CPU
tests pin that replay against the recorded reference outputs, the GPU tests compare the engine's entry point with the
replay bit for bit and the tools with the recorded text byte for byte."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import classdist_replay as R
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
CLI = os.path.join(GOLDEN, "cli")
DATA = os.path.join(GOLDEN, "data")
EXPECTED = json.load(open(os.path.join(GOLDEN, "classdist", "expected.json")))
RUNS = sorted(EXPECTED["runs"])
STORED = {"lvq_olvq1.cod": CLI, "ex1.dat": DATA}


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("mindist", "stddev", "datconv")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a directory with every input of the recorded runs: the stored fixtures and the generated ones, md5 checked"""
    d = str(tmp_path_factory.mktemp("classdist_inputs"))
    R.write_generated(d, DATA)
    for name, want in EXPECTED["inputs"].items():
        if name in STORED:
            shutil.copy(os.path.join(STORED[name], name), os.path.join(d, name))
        assert md5(os.path.join(d, name)) == want, name
    return d


def run_tool(tool, args, cwd=None, bindir=BIN):
    return subprocess.run([os.path.join(bindir, tool)] + [str(a) for a in args], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, cwd=cwd)


def arg_of(args, flag):
    return args[args.index(flag) + 1] if flag in args else None


# ------------------------------------------------------------------ CPU side
@pytest.mark.parametrize("tag", RUNS)
def test_replay_reproduces_the_reference(tag, inputs):
    """the numpy float32 replay (sub, mul, add per component in order; a component masked in either row skipped) prints
    what the real reference printed, medians and deviations alike -- the scaled fixture's text carries every bit"""
    from som_lvq_pak_amd import textio
    run = EXPECTED["runs"][tag]
    table = textio.LabelTable()
    cin, din = arg_of(run["args"], "-cin"), arg_of(run["args"], "-din")
    first = cin if run["tool"] == "mindist" else din
    ent, _ = textio.read_entries(os.path.join(inputs, first), table)
    md = R.med_distances(ent.points, ent.first_label, ent.mask)
    devs = None
    if din is not None:
        dat = ent if din == first else textio.read_entries(os.path.join(inputs, din), table)[0]
        devs = R.deviations(dat.points, dat.first_label, dat.mask, md)
    assert R.report(md, devs, table.names, "min" if run["tool"] == "mindist" else "med") == run["stdout"]
    assert run["returncode"] == 0


def test_recorded_runs_cover_the_cases():
    out = {t: EXPECTED["runs"][t]["stdout"] for t in RUNS}
    assert "-1.000" in out["stddev_masked"] and out["stddev_masked"].count("\n") == 3      # the masked row of Q is dropped
    assert out["mindist_cod_din_buffer"] == out["mindist_cod_din"]                         # -buffer changes nothing
    assert out["mindist_cod_din"].endswith(" \n") and not out["mindist_cod"].endswith(" \n")
    assert out["stddev_ex1"] == out["mindist_ex1_self"].replace("min dist.", "med dist.")
    rows, labels, _ = R.scaled_case()
    min_sq, state = R.nearest_later(rows, labels)
    d = R.distances_from(min_sq, state)[state == 1]
    assert (state == 0).sum() == 5 and (d == 0).sum() == 1                                 # the duplicated row
    assert ((d >= 2.0 ** 14) & (d < 2.0 ** 24)).sum() >= 0.95 * len(d)
    meds = [float(m[2]) for m in R.med_distances(rows, labels, None, (min_sq, state))]
    assert all(2.0 ** 14 <= m < 2.0 ** 24 for m in meds[:4]) and meds[4] == 0         # every printed median carries all its bits


@pytest.mark.parametrize("tag", [t for t in RUNS if EXPECTED["runs"][t]["tool"] == "mindist"])
def test_compiled_reference_still_gives_the_recorded_text(tag, inputs):
    ref = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref, "mindist")):
        pytest.skip("oracle/_ref not built (needs the reference's sources)")
    run = EXPECTED["runs"][tag]
    p = run_tool("mindist", run["args"], cwd=inputs, bindir=ref)
    assert p.returncode == 0 and p.stdout == run["stdout"]


def test_tools_usage_and_refusals_without_a_gpu(tools, inputs):
    for t in ("mindist", "stddev"):
        p = run_tool(t, ["-help"])
        assert p.returncode == 0 and "MI355X" in p.stdout
    p = run_tool("mindist", ["-din", "a"])
    assert p.returncode == 255 and "Can't find asked option -cin" in p.stderr
    p = run_tool("stddev", ["-din", "ex1.dat", "-buffer", 10], cwd=inputs)
    assert p.returncode == 1 and "-buffer" in p.stderr and p.stdout == ""
    p = run_tool("stddev", ["-din", "gen:k=4,dim=8,n=100"])
    assert p.returncode == 1 and "labels=1" in p.stderr and p.stdout == ""
    p = run_tool("mindist", ["-cin", "gen:k=4,dim=8,n=100"])
    assert p.returncode == 1 and "labels=1" in p.stderr and p.stdout == ""
    import torch
    if not torch.cuda.is_available():
        p = run_tool("stddev", ["-din", "ex1.dat"], cwd=inputs)
        assert p.returncode == 1 and "no CPU path" in p.stderr and p.stdout == ""


def test_signature_and_kernel_name():
    import ctypes as C
    from som_lvq_pak_amd import _lib
    assert _lib.SIGNATURES["somhip_class_nearest_later"] == (C.c_int, [C.c_void_p, _lib.c_float_p, _lib.c_i32_p])
    lib = _lib.load()
    names = [lib.somhip_kernel_name(i).decode() for i in range(lib.somhip_kernel_count())]
    assert names[0] == "k_scan_exact" and names[25] == "k_sammon_error"           # the earlier ids keep their numbers
    assert names.index("k_class_nearest") == 26 and len(names) <= 64


def test_class_kernels_have_no_fma(tmp_path):
    """the self-join's sums are fp32 sub, mul, add with three roundings (lvq_pak.c:308-309): a contracted v_fma / v_fmac
    in k_class_nearest would change results, so look at the gfx950 ISA of both instantiations"""
    s = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                           "-ffp-contract=off", "--cuda-device-only", "-S", "-o", s,
                           os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")])
    txt = open(s).read()
    bodies = dict(re.findall(r"^(_ZN6somhip\w+):.*?\n(.*?)s_endpgm", txt, flags=re.S | re.M))
    checked = 0
    for name, body in bodies.items():
        if "k_class_nearest" not in name:
            continue
        checked += 1
        bad = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad)_f32\b.*", body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_(pk_)?mul_f32", body) and re.search(r"v_(pk_)?add_f32", body)
    assert checked == 2                                                              # unmasked and masked


# ------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    yield e
    e.close()


def _labels(sizes, interleave, rs):
    lab = np.concatenate([np.full(s, k + 1, dtype=np.int32) for k, s in enumerate(sizes)])
    if interleave:
        rs.shuffle(lab)
    return lab


CASES = {                                    # (n, dim, class sizes, interleaved)
    "1x3": (1, 3, (1,), False),
    "2x1": (2, 1, (2,), False),
    "65x4_two": (65, 4, (33, 32), True),
    "257x5": (257, 5, (1, 2, 63, 191), True),
    "1100x7_five": (1100, 7, (1, 2, 63, 500, 534), True),
    "1100x7_one": (1100, 7, (1100,), False),
    "300x12_singletons": (300, 12, (1,) * 300, False),
    "200x130_three": (200, 130, (50, 70, 80), True),
}


def _case(name, masked=False):
    n, dim, sizes, interleave = CASES[name]
    rs = np.random.RandomState(len(name) * 1000 + n + dim)
    labels = _labels(sizes, interleave, rs)
    if name == "65x4_two":
        labels = (np.arange(n) % 2 + 1).astype(np.int32)           # strictly alternating
    rows = (3.0 * rs.standard_normal((n, dim))).astype(np.float32)
    big = np.nonzero(labels == np.argmax(np.bincount(labels)))[0]     # the rows of the largest class
    if len(big) >= 3:
        rows[big[len(big) // 2]] = rows[big[1]]                     # a duplicated row inside a class: minimum +0
    mask, planted = None, None
    if masked:
        mask = (rs.uniform(size=(n, dim)) < 0.3).astype(np.uint8)
        a, b = big[2], big[len(big) - 2]                            # two rows of one class with disjoint unmasked components
        mask[a] = 0; mask[b] = 1
        mask[a, dim // 2:] = 1; mask[b, dim // 2:] = 0
        planted = a
    return rows, labels, mask, planted


def _check(eng, rows, labels, mask, ds=None):
    from som_lvq_pak_amd import engine as E
    want_sq, want_state = R.nearest_later(rows, labels, mask)
    own = ds is None
    if own:
        ds = E.Dataset(eng, rows, mask=mask, labels=labels)
    got_sq, got_state = E.class_nearest_later(ds)
    if own:
        ds.close()
    assert np.array_equal(got_state, want_state)
    cmp = want_state != 2                                            # (min_sq is not defined under state 2)
    assert np.array_equal(got_sq.view(np.uint32)[cmp], want_sq.view(np.uint32)[cmp])
    assert np.isinf(got_sq[want_state == 0]).all()
    return want_sq, want_state


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_point_equals_the_replay_bit_for_bit(name, eng):
    """min_sq bit patterns and states: one row, one pair, alternating classes, classes of 1 / 2 / 63 / more than a wave
    interleaved, segments that cross row blocks and register tiles, the full triangle of one class, only singletons, a
    dim that is neither a multiple of 4 nor one tile"""
    rows, labels, _, _ = _case(name)
    want_sq, want_state = _check(eng, rows, labels, None)
    n = len(labels)
    assert want_state[n - 1] == 0                                    # the last row has no later one
    if name == "300x12_singletons":
        assert (want_state == 0).all()
    if max(CASES[name][2]) >= 3:
        assert ((want_sq == 0) & (want_state == 1)).sum() >= 1       # the duplicated row


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["257x5", "1100x7_five"])
def test_masked_entry_point_equals_the_replay(name, eng):
    """about 30 % of the components masked at random, a component counts only when neither row masks it; the planted
    pair with disjoint unmasked components gives state 2"""
    rows, labels, mask, planted = _case(name, masked=True)
    _, want_state = _check(eng, rows, labels, mask)
    assert want_state[planted] == 2
    assert (want_state == 1).sum() >= 30 and (want_state == 2).sum() >= 30         # (at dim 5 random masks alone often leave a pair nothing)


@pytest.mark.gpu
def test_generated_data_set_uses_its_mixture_ids(eng):
    from som_lvq_pak_amd import engine as E
    ds = E.Dataset(eng, generate=(77, 4, 16, 0, 1000))
    rows = ds.rows(0, 1000)
    assert len(set(ds.centres.tolist())) == 4
    _check(eng, rows, ds.centres, None, ds=ds)
    ds.close()


@pytest.mark.gpu
def test_entry_point_refuses_a_data_set_without_labels(eng):
    from som_lvq_pak_amd import engine as E
    from som_lvq_pak_amd._lib import SomhipError
    ds = E.Dataset(eng, np.ones((5, 3), dtype=np.float32))
    with pytest.raises(SomhipError, match="no labels"):
        E.class_nearest_later(ds)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RUNS)
def test_tools_equal_the_reference_byte_for_byte(tag, tools, inputs):
    run = EXPECTED["runs"][tag]
    p = run_tool(run["tool"], run["args"], cwd=inputs)
    assert p.returncode == run["returncode"] == 0, p.stderr
    assert p.stdout == run["stdout"]


@pytest.mark.gpu
def test_tools_read_the_raw_and_the_generated_forms(tools, inputs, tmp_path):
    """the raw fp32 form of an input (datconv) gives the same text as its .dat; a gen: source with labels=1 gives what the
    replay gives on the same stream"""
    from som_lvq_pak_amd import engine as E
    for name in ("scaled.dat", "masked.dat"):
        raw = tmp_path / (name + ".f32")
        p = run_tool("datconv", ["-din", os.path.join(inputs, name), "-dout", raw])
        assert p.returncode == 0, p.stderr
        p = run_tool("stddev", ["-din", raw])
        assert p.returncode == 0 and p.stdout == EXPECTED["runs"]["stddev_" + name[:-4]]["stdout"], name
    p = run_tool("stddev", ["-din", "gen:k=3,dim=6,n=400,seed=5,labels=1"])
    assert p.returncode == 0, p.stderr
    rows, cen = E.gen_rows(5, 3, 6, 0, 400)
    names, labels = [""], []
    for c in cen:                                                    # "c<id>", numbered in order of first appearance
        if "c%d" % c not in names:
            names.append("c%d" % c)
        labels.append(names.index("c%d" % c))
    md = R.med_distances(rows, np.array(labels), None)
    assert p.stdout == R.report(md, R.deviations(rows, np.array(labels), None, md), names, "med")


@pytest.mark.gpu
def test_tool_refusals(tools, inputs):
    p = run_tool("mindist", ["-cin", "lvq_olvq1.cod", "-din", "ex1.dat"], cwd=inputs)   # the reference reads past its arrays
    assert p.returncode == 1 and "'F'" in p.stderr and p.stdout == ""
    p = run_tool("stddev", ["-din", "ex1.dat", "-buffer", 10], cwd=inputs)
    assert p.returncode == 1
    p = run_tool("stddev", ["-din", "gen:k=4,dim=8,n=100"])
    assert p.returncode == 1
