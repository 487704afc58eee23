"""The engine's bookkeeping, checked without a GPU: every entry point that takes an engine refuses a null one with a
message that names it, and the facts the host code used to repeat (the statistics block's word indices, the re-rank
pair list's segment length, the number of scratch slots) are written once."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "som_lvq_pak_amd", "csrc")


@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


def _null_engine_calls():
    out8 = (C.c_uint64 * 8)()
    launches, ms = C.c_int64(0), C.c_double(0.0)
    ptr = C.c_void_p(None)
    buf = (C.c_char * 16)()
    return {
        "somhip_engine_set_scan_mode": (None, 0),
        "somhip_scan_stats": (None, out8),
        "somhip_timing_enable": (None, 1),
        "somhip_timing_select": (None, 1),
        "somhip_timing_reset": (None,),
        "somhip_timing_get": (None, 0, C.byref(launches), C.byref(ms)),
        "somhip_device_alloc": (None, 16, C.byref(ptr)),
        "somhip_device_free": (None, None),
        "somhip_copy_to_host": (None, buf, None, 16),
        "somhip_copy_to_device": (None, None, buf, 16),
    }


@pytest.mark.parametrize("name", sorted(_null_engine_calls()))
def test_null_engine_is_an_error_not_a_crash(built, name):
    from som_lvq_pak_amd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_null_engine_calls()[name]) != 0
    msg = lib.somhip_last_error().decode()
    assert msg.startswith(name), msg
    assert msg == "%s: null engine" % name


def _source_lines(top):
    for dirpath, _, files in os.walk(top):
        for f in sorted(files):
            path = os.path.join(dirpath, f)
            with open(path) as fh:
                for no, line in enumerate(fh, 1):
                    yield "%s:%d" % (os.path.relpath(path, ROOT), no), line


def _code(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_statistics_words_are_named_not_counted():
    bad = [where for where, line in _source_lines(CSRC) if re.search(r"d_stats\s*\+\s*\d", line)]
    assert not bad, bad
    bad = [where for where, line in _source_lines(os.path.join(CSRC, "kernels")) if re.search(r"\bstats\s*\+\s*\d", line)]
    assert not bad, bad


def test_pair_list_segment_length_is_written_once():
    code = _code(open(os.path.join(CSRC, "host_scan.inc")).read())
    assert len(re.findall(r"\b16384\b", code)) == 1


def test_engine_destroy_counts_no_slots_by_hand():
    text = open(os.path.join(CSRC, "somhip.hip")).read()
    body = re.search(r'extern "C" void somhip_engine_destroy\(.*?ABI_CATCH_VOID\(somhip_engine_destroy\)', text, flags=re.S).group(0)
    assert "SLOT_COUNT" in body
    assert not re.search(r"\b32\b", _code(body)), body


def _csrc_code():
    """path -> text without comments, for every file under csrc/"""
    out = {}
    for dirpath, _, files in os.walk(CSRC):
        for f in sorted(files):
            path = os.path.join(dirpath, f)
            out[os.path.relpath(path, CSRC)] = _code(open(path).read())
    return out


def _function_body(code, head):
    """the text of the function whose definition starts with `head`, braces matched"""
    start = code.index(head)
    i = code.index("{", start)
    depth = 0
    for j in range(i, len(code)):
        depth += code[j] == "{"
        depth -= code[j] == "}"
        if depth == 0:
            return code[start:j + 1]
    raise AssertionError(head)


def test_kernels_are_launched_from_one_place():
    sites = {f: len(re.findall(r"\bhipLaunchKernelGGL\b", t)) for f, t in _csrc_code().items()}
    assert sum(sites.values()) == 1, {f: n for f, n in sites.items() if n}
    body = _function_body(_csrc_code()["somhip.hip"], "static int launch(somhip_engine *e")
    assert "hipLaunchKernelGGL" in body and "hipGetLastError" in body and "launch failed" in body


def test_stream_copies_go_through_the_typed_helpers():
    sites = {f: len(re.findall(r"\bhipMemcpyAsync\b", t)) for f, t in _csrc_code().items()}
    assert sum(sites.values()) == 1, {f: n for f, n in sites.items() if n}
    body = _function_body(_csrc_code()["somhip.hip"], "static int copy_async(somhip_engine *e")
    assert "hipMemcpyAsync" in body and "sizeof(T) * count" in body


def test_shard_and_empty_sample_predicates_are_written_once():
    code = _csrc_code()
    create = _function_body(code["somhip.hip"], 'extern "C" int somhip_dataset_create(')
    rest = "".join(code.values()).replace(create, "")
    assert len(re.findall(r"all_masked\s*\.\s*empty\s*\(\s*\)", rest)) == 1
    # a mirror's n_global compared with its row count, either operand first (codebook_create checks its n_global
    # ARGUMENT against the map's sides before any mirror exists: that is no shard test)
    assert len(re.findall(r"->\s*n_global\s*!=|!=\s*\w+\s*->\s*n_global\b", rest)) == 1
    assert "is_shard" in _function_body(code["somhip.hip"], "static bool is_shard(")
