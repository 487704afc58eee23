"""CPU-side check of the ring kernel's tile epilogue on its gfx950 ISA (the compile of tests/test_build.py's
test_ring_kernel_keeps_its_asm_loads_in_place, flags of the Makefile): between the last MFMA of a tile and the first of
the next nothing covers the eight waves' work, so the epilogue must stay as short as it was made -- a tile's first stage
multiplies onto the constant 0 instead of clearing 128 accumulator registers, the tile's minima come back from LDS under
a counted wait (no drain of the ring's LDS-DMA requests), and memory is written by global_ instructions (a flat_ one
counts in lgkmcnt as well, among the fragment reads the stages count)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ring_body(tmp_path_factory):
    s = str(tmp_path_factory.mktemp("isa") / "k.s")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                          "-fno-slp-vectorize", "--cuda-device-only", "-S", "-o", s,
                          os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "somhip.hip")], stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    txt = open(s).read()
    body = re.search(r"^_ZN6somhip20k_dist_mfma_bf16_l1r\w+:.*?\n(.*?)\.Lfunc_end", txt, flags=re.S | re.M).group(1)
    return [ln.split(";")[0].strip() for ln in body.split("\n") if ln.strip() and not ln.strip().startswith((";", "."))]


def test_first_stage_of_a_tile_multiplies_onto_zero(ring_body):
    mfma = [ln for ln in ring_body if ln.startswith("v_mfma")]
    zero_c = [ln for ln in mfma if re.search(r",\s*0$", ln)]
    assert len(zero_c) >= 32 and len(zero_c) % 32 == 0, (len(zero_c), len(mfma))    # whole stages
    run = longest = 0
    for ln in ring_body:
        run = run + 1 if re.match(r"v_mov_b32(_e32)?\s+v\d+,\s*0$", ln) else 0
        longest = max(longest, run)
    assert longest < 64, "the accumulators are cleared by %d moves in a row" % longest


def test_epilogue_neither_drains_the_ring_nor_writes_flat(ring_body):
    assert not [ln for ln in ring_body if ln.startswith("flat_")]
    stores = [i for i, ln in enumerate(ring_body) if ln.startswith("global_store_dwordx2")]
    assert len(stores) == 1, stores                                      # the tile's minima: 512 contiguous bytes per wave
    assert sum(ln.startswith("global_atomic_umin") for ln in ring_body) >= 1
    barrier = max(i for i in range(stores[0]) if ring_body[i] == "s_barrier")
    assert any(ln.startswith("ds_read_b64") for ln in ring_body[barrier:stores[0]])   # (it is the epilogue's barrier)
    drains = [ln for ln in ring_body[barrier:stores[0]] if ln.startswith("s_waitcnt") and "vmcnt(0)" in ln]
    assert not drains, drains
    # and nowhere else on a tile's way: from the first stage wait to the end of the tile loop (the column's atomic
    # minimum, which follows the store) the only full wait for memory is the one in front of the exit
    first = next(i for i, ln in enumerate(ring_body) if ln.startswith("s_waitcnt vmcnt(4)"))
    last = max(i for i, ln in enumerate(ring_body) if ln.startswith("s_waitcnt") and "vmcnt(0)" in ln)
    assert [ln for ln in ring_body[last + 1:] if not ln.startswith("s_")] == [], "the last drain is not the exit's"
    drains = [ln for ln in ring_body[first:last] if ln.startswith("s_waitcnt") and "vmcnt(0)" in ln]
    assert not drains, drains
