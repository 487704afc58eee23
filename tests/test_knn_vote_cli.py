"""The tools that consume a k-NN vote (setlabel, eveninit, propinit, balance, elimin) with more than 8 neighbours: the
vote is formed on the device (somhip_knn_vote) and the files are the bytes the REAL reference wrote for the same commands
(tests/golden/knn_vote/expected.json, recorded by tests/golden/make_golden_knn_vote.py).  The masked data files are not
stored: the fixture script's seeded write_masked_data() makes them again."""
import hashlib
import importlib.util
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "som_lvq_pak_amd", "host", "bin")
DATA = os.path.join(GOLDEN, "data")
CLI = os.path.join(GOLDEN, "cli")
FIXTURE = json.load(open(os.path.join(GOLDEN, "knn_vote", "expected.json")))
EXPECTED = FIXTURE["runs"]
CLI_EXPECTED = json.load(open(os.path.join(CLI, "expected.json")))
TAGS = ("setlabel_9", "setlabel_21", "eveninit_9", "propinit_11", "balance_9", "elimin_9", "elimin_10", "elimin_12")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _load("make_golden_knn_vote")


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("setlabel", "eveninit", "propinit", "balance", "elimin")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "som_lvq_pak_amd", "host")])
    return BIN


@pytest.fixture(scope="module")
def dirs(gen, tools, tmp_path_factory):
    """the masked data, made again by the fixture script's seeded masking, and the codebooks the recorded runs start from,
    made again by this project's tools"""
    out = {"masked": str(tmp_path_factory.mktemp("masked_data")), "made": str(tmp_path_factory.mktemp("made"))}
    gen.write_masked_data(out["masked"])
    gen.make_codebooks(lambda tool: os.path.join(BIN, tool), out["made"])
    return out


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


# ------------------------------------------------------------------------------------------------ without a GPU
def test_fixture_is_whole(gen):
    """every recorded run is one the script lists, with its command, and every run of the issue's list is there unmasked
    and -- balance apart -- masked"""
    assert set(EXPECTED) <= set(gen.RUNS) and set(FIXTURE["made"]) == set(gen.MADE)
    for tag in TAGS:
        assert tag in EXPECTED, tag
        if not tag.startswith("balance"):
            assert "masked_" + tag in EXPECTED, tag
    assert not any(t.startswith("masked_balance") for t in EXPECTED)
    for tag, r in EXPECTED.items():
        tool, din, cin, args = gen.RUNS[tag]
        assert (r["tool"], r["din"], r["cin"], r["args"]) == (tool, din, cin, list(args)), tag
        assert r["exit"] == 0 and "out.cod" in r["md5"], tag
        assert all(len(v) == 32 for v in r["md5"].values()), tag
        assert ("out.lra" in r["md5"]) == (tool == "balance"), tag
        assert (r["stdout"] != "") == (tool == "balance"), tag
    # the reference caps elimin's 12 neighbours to 10
    assert EXPECTED["elimin_12"]["md5"] == EXPECTED["elimin_10"]["md5"] != EXPECTED["elimin_9"]["md5"]
    assert EXPECTED["masked_elimin_12"]["md5"] == EXPECTED["masked_elimin_10"]["md5"]


def test_usage_names_the_limits(tools):
    for tool, limit in (("setlabel", 256), ("eveninit", 256), ("propinit", 256), ("balance", 256), ("elimin", 10), ("knntest", 8)):
        p = subprocess.run([os.path.join(BIN, tool), "-help"], stdout=subprocess.PIPE, text=True)
        assert "at most %d)" % limit in p.stdout, tool


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(EXPECTED))
def test_tools_write_the_references_bytes(tools, gen, dirs, tmp_path, tag):
    r = EXPECTED[tag]
    assert gen.md5s(dirs["made"]) == FIXTURE["made"]
    cmd = gen.command(os.path.join(BIN, r["tool"]), gen.RUNS[tag], dirs, str(tmp_path / "out.cod"))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(tmp_path))
    assert p.returncode == r["exit"], (cmd, p.stderr)
    assert p.stdout == r["stdout"]
    assert gen.md5s(str(tmp_path)) == r["md5"]
    if tag.endswith("elimin_12"):
        assert "Can use only 10 neighbors" in p.stderr


@pytest.mark.gpu
def test_small_knn_still_gives_the_recorded_bytes(tools, tmp_path):
    """-knn 3 and -knn 5 through the device vote: the md5s tests/golden/cli/expected.json already holds"""
    for tool in ("setlabel", "elimin", "initlvq", "balance"):            # ... which is where these tools get their votes
        syms = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(BIN, tool)], stdout=subprocess.PIPE, text=True)
        assert syms.returncode == 0 and "somhip_knn_vote" in syms.stdout, tool
    t = CLI_EXPECTED["lvq"]["tools"]
    ex1, ex2, cod = os.path.join(DATA, "ex1.dat"), os.path.join(DATA, "ex2.dat"), os.path.join(CLI, "lvq_olvq1.cod")

    def run(tool, *args):
        p = subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args] + ["-v", "0"], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, (tool, args, p.stderr)
        return p

    for knn in (3, 5):
        run("setlabel", "-din", ex2, "-cin", cod, "-cout", tmp_path / "sl.cod", "-knn", knn)
        assert md5(tmp_path / "sl.cod") == t["setlabel_%d_md5" % knn], knn
        run("elimin", "-din", ex1, "-cout", tmp_path / "el.cod", "-knn", knn)
        assert md5(tmp_path / "el.cod") == t["elimin_%d_md5" % knn], knn
    run("eveninit", "-din", ex1, "-cout", tmp_path / "ev.cod", "-noc", 100, "-knn", 3)
    assert md5(tmp_path / "ev.cod") == t["eveninit_knn3_100"]["md5"]
    run("eveninit", "-din", ex1, "-cout", tmp_path / "ev.cod", "-noc", 200, "-knn", 5)
    assert md5(tmp_path / "ev.cod") == CLI_EXPECTED["lvq"]["init_md5"]
    run("propinit", "-din", ex1, "-cout", tmp_path / "pr.cod", "-noc", 200, "-knn", 5)
    assert md5(tmp_path / "pr.cod") == t["propinit_200"]["md5"]
    e400 = tmp_path / "even400.cod"
    run("eveninit", "-din", ex1, "-cout", e400, "-noc", 400)
    for tag, cin, knn in (("balance_even", os.path.join(CLI, "lvq_init.cod"), 5), ("balance_even400_knn3", e400, 3)):
        out = tmp_path / (tag + ".cod")
        p = run("balance", "-din", ex1, "-cin", cin, "-cout", out, "-knn", knn)
        assert p.stdout == t[tag]["stdout"], tag
        assert md5(out) == t[tag]["md5"] and md5(tmp_path / (tag + ".lra")) == t[tag]["lra_md5"], tag
