"""include/somhip_rslvq.h, the header of batch Robust Soft LVQ (K13) that include/somhip.h includes, held to what the suite
asks of somhip.h itself:

  * tests/test_build.py: every symbol the header declares is exported by libsomhip.so and mirrored, and the mirror
    (som_lvq_pak_amd/_lib.py RSLVQ_SIGNATURES) names nothing else;
  * tests/test_prepared_state.py: every entry point that takes a codebook it may write to is a writer or a reader of the
    tables below; a writer starts on the cached route, moves rows and must leave flags that tell the truth
    (check_state), a reader keeps the flags and the bits.  The helpers and fixtures are that file's own.

The GPU tests need an MI355X:  pytest -m gpu  (the first three do not)."""
import os
import re

import numpy as np
import pytest

import test_prepared_state as PS
from conftest import ROOT
from test_prepared_state import E, data, ds, eng  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
M = PS.M
SIGMA2 = 50.0                        # about the squared distance of a sample to the rows of its cluster (dim 32, noise 1 + 0.3)


@pytest.fixture(scope="module")
def built():
    import subprocess
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


def header():
    hdr = open(os.path.join(ROOT, "include", "somhip_rslvq.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def w_rslvq_train(E, eng, cb, ds, data):
    E.rslvq_train(cb, ds, 2, 50.0, SIGMA2, n=M, stats=False)


def w_rslvq_update(E, eng, cb, ds, data):
    G, c = E.rslvq_sums(cb, ds, E.rslvq_posterior(cb, ds, SIGMA2, n=M)["q"], n=M)
    E.rslvq_update(cb, 50.0, SIGMA2, M, G, c)


# id -> (entry points that write rows, the writer, the flags (prep_valid, rowmajor_valid) it must leave)
WRITERS = {
    "rslvq_train": (("somhip_rslvq_train",), w_rslvq_train, (0, 0)),
    "debug_rslvq_update": (("somhip_debug_rslvq_update",), w_rslvq_update, (0, 0)),
}
# id -> (entry points, the reader)
READERS = {
    "rslvq_search": (("somhip_rslvq_search",), lambda E, eng, cb, ds: E.rslvq_search(cb, ds, SIGMA2, n=M)),
    "rslvq_stages": (("somhip_debug_rslvq_posterior", "somhip_debug_rslvq_sums"),
                     lambda E, eng, cb, ds: E.rslvq_sums(cb, ds, E.rslvq_posterior(cb, ds, SIGMA2, n=M)["q"], n=M)),
}


# ------------------------------------------------------------------------------------------------ without a GPU
def test_somhip_h_includes_the_header():
    top = open(os.path.join(ROOT, "include", "somhip.h")).read()
    assert re.search(r'^#include "somhip_rslvq.h"$', top, flags=re.M)
    assert "somhip_rslvq_train" not in re.sub(r"/\*.*?\*/", "", top, flags=re.S)        # declared once, in its own header


def test_header_symbols_exported(built):
    from som_lvq_pak_amd import _lib
    declared = set(re.findall(r"\b(somhip_[a-z0-9_]+)\s*\(", header()))
    assert len(declared) == 7
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), "libsomhip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.RSLVQ_SIGNATURES[name][1], name
    assert declared == set(_lib.RSLVQ_SIGNATURES), declared ^ set(_lib.RSLVQ_SIGNATURES)
    assert not (set(_lib.RSLVQ_SIGNATURES) & set(_lib.SIGNATURES))


def test_every_writer_has_a_case():
    """every entry point of the header that takes a codebook it may write to is in the writers' table or the readers'"""
    takes = set()
    for name, args in re.findall(r"\b(somhip_[a-z0-9_]+) ?\(([^;{}]*?)\) ?;", header()):
        if re.search(r"(?<!const )somhip_codebook \*(?!\*)", args):
            takes.add(name)
    assert len(takes) == 5 and "somhip_rslvq_train" in takes and "somhip_rslvq_timing" not in takes
    writers = {s for syms, _, _ in WRITERS.values() for s in syms}
    readers = {s for syms, _ in READERS.values() for s in syms}
    assert not (writers & readers)
    assert takes == writers | readers, takes ^ (writers | readers)


# ------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("case", sorted(WRITERS))
def test_writer_leaves_a_true_state(E, eng, oracle, data, ds, case):
    _, writer, flags = WRITERS[case]
    cb = PS.make_plain(E, eng, data)
    try:
        PS.prime(E, eng, cb, ds)
        before = cb.download()
        writer(E, eng, cb, ds, data)
        after = cb.download()
        moved = (PS.bits(after) != PS.bits(before)).any(axis=1)
        assert moved.all(), "every row has a posterior: %d of %d rows moved" % (moved.sum(), len(moved))
        st = E.debug_prepared_state(cb)
        assert st["bm_open"] == 0 and (st["prep_valid"], st["rowmajor_valid"]) == flags
        PS.check_state(E, eng, oracle, cb, ds, data[0], split_rows=None)
    finally:
        cb.close()


@gpu
def test_readers_keep_the_cache(E, eng, oracle, data, ds):
    cb = PS.make_plain(E, eng, data)
    try:
        st0 = PS.prime(E, eng, cb, ds)
        rows = cb.download()
        want = None
        for case in sorted(READERS):
            READERS[case][1](E, eng, cb, ds)
            st = E.debug_prepared_state(cb)
            assert (st["prep_valid"], st["rowmajor_valid"], st["bm_open"]) == (1, 1, 0), case
            for name in ("chi", "clo"):
                assert np.array_equal(st[name], st0[name]), (case, name)
            assert np.array_equal(st["rowmajor"].view(np.uint32), st0["rowmajor"].view(np.uint32)), case
            assert np.array_equal(PS.bits(cb.download()), PS.bits(rows)), "%s moved rows" % case
            _, want = PS.check_state(E, eng, oracle, cb, ds, data[0], split_rows=rows, want=want)
    finally:
        cb.close()
