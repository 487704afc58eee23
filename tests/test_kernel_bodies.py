"""The prototype kernels (K8 batch map, K8m, K1d map distortion, K9 glvq, K11 grlvq, K12 gmlvq) state what they share once,
as __device__ __forceinline__ bodies under csrc/kernels/.  Read from the source, without a GPU, in the manner of
test_proto_drivers.py: comments stripped, sites counted per file.

What is shared is what could be shared with the kernels' machine code left as it was (profiles/kernel_bodies_vs_parent.txt);
where a body had to stay written out per kernel, the test states what is in the tree and names the reason."""
import os
import re

from conftest import ROOT

KERNELS = os.path.join(ROOT, "som_lvq_pak_amd", "csrc", "kernels")


def _code():
    """file name -> text without comments, for every file under csrc/kernels/"""
    out = {}
    for f in sorted(os.listdir(KERNELS)):
        text = open(os.path.join(KERNELS, f), errors="replace").read()
        out[f] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    return out


def _sites(code, pattern, files=None):
    return {f: len(re.findall(pattern, t)) for f, t in code.items()
            if (files is None or f in files) and re.search(pattern, t)}


def _body(code, head):
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


def test_the_group_skip_rule_is_stated_once():
    code = _code()
    # the margin of the bubble group skip: one site in the whole directory
    assert _sites(code, r"1\.000001") == {"batchmap.hpp": 1}
    assert "1.000001" in _body(code["batchmap.hpp"], "__device__ __forceinline__ bool bm_group_skipped(")
    # ... and the three lattice GEMMs ask it
    for f, kernel in (("batchmap.hpp", "void k_batchmap_combine("), ("batchmap_missing.hpp", "void k_batchmap_combine_missing("),
                      ("map_distortion.hpp", "void k_distortion_evaluate(")):
        assert "bm_group_skipped<GAUSS>(" in _body(code[f], kernel), kernel


def test_the_lattice_gemm_frame_is_still_written_per_kernel():
    # One walk body for the three kernels (the fetch, the staging, the weights and the MFMA loop behind a source-columns
    # policy) was built and taken out again: behind a function boundary the compiler allots the bubble instantiations other
    # registers (k_batchmap_combine<false> 128 -> 140 VGPRs, 97 -> 88 SGPRs; the other two alike), which the refactor's
    # condition -- the parent's machine code -- does not allow.  So the MFMA loop stands once per kernel; when the frame is
    # unified, this becomes {"batchmap.hpp": 1} with no site in the other two files.
    code = _code()
    files = ("batchmap.hpp", "batchmap_missing.hpp", "map_distortion.hpp")
    assert _sites(code, r"__builtin_amdgcn_mfma_f64_16x16x4f64", files) == {f: 1 for f in files}


def test_the_class_scan_is_still_written_per_metric():
    # One scan body for both metrics was built and taken out again for the same reason: k_scan_class<32, 4> and
    # k_scan_class_weighted<32, 4> sit at 256 VGPRs, and behind a function boundary six more accumulator registers are
    # spilled to (36 -> 42 AGPRs).  Sharing only the label staging and the merge added a scalar instruction to all four.
    # When the scan is unified, this becomes {"glvq.hpp": 1}.
    code = _code()
    assert _sites(code, r"atomicMin\([^;]*keys2", ("glvq.hpp", "grlvq.hpp")) == {"glvq.hpp": 1, "grlvq.hpp": 1}


def test_the_row_of_a_run_sample_is_formed_in_one_place():
    code = _code()
    sums = ("batchmap.hpp", "batchmap_missing.hpp", "glvq.hpp", "grlvq.hpp")
    assert _sites(code, r"r %= n_rows", ("common.hpp",) + sums) == {"common.hpp": 1}
    assert "r %= n_rows" in _body(code["common.hpp"], "__device__ __forceinline__ int64_t run_row(")
    for f, kernel in (("batchmap.hpp", "void k_batchmap_sums("), ("batchmap_missing.hpp", "void k_batchmap_sums_missing("),
                      ("glvq.hpp", "void glvq_sums_chain(")):
        assert "run_row(first," in _body(code[f], kernel), kernel


def test_the_step_and_the_sums_of_a_chosen_row_are_formed_in_one_place():
    code = _code()
    # g = (Sp - sp W) - (Sm - sm W): one site, used by the three updates
    assert _sites(code, r"gp - gm") == {"glvq.hpp": 1}
    assert "gp - gm" in _body(code["glvq.hpp"], "__device__ __forceinline__ double glvq_step_g(")
    assert "glvq_step_g(" in _body(code["glvq.hpp"], "void glvq_update_tiles(")
    assert "glvq_step_g(" in _body(code["gmlvq.hpp"], "void k_gmlvq_update(")
    assert "glvq_update_tiles<GLVQ_THREADS, false>(" in _body(code["glvq.hpp"], "void k_glvq_update(")
    assert "glvq_update_tiles<THREADS, true>(" in _body(code["grlvq.hpp"], "void k_grlvq_update(")
    # the ordered sums of both roles, with or without the relevance chain
    assert "glvq_sums_chain<CONT, false, GLVQ_SUM_AHEAD>(" in _body(code["glvq.hpp"], "void k_glvq_sums(")
    assert "glvq_sums_chain<false, true, AHEAD>(" in _body(code["grlvq.hpp"], "void k_grlvq_sums(")
    assert _sites(code, r"rel \+= pr", ("glvq.hpp", "grlvq.hpp")) == {"glvq.hpp": 1}


def test_every_kernel_keeps_its_name():
    code = _code()
    for f, kernel in (("glvq.hpp", "k_scan_class"), ("grlvq.hpp", "k_scan_class_weighted"), ("batchmap.hpp", "k_batchmap_combine"),
                      ("batchmap_missing.hpp", "k_batchmap_combine_missing"), ("map_distortion.hpp", "k_distortion_evaluate"),
                      ("glvq.hpp", "k_glvq_update"), ("grlvq.hpp", "k_grlvq_update"), ("glvq.hpp", "k_glvq_sums"),
                      ("grlvq.hpp", "k_grlvq_sums")):
        assert len(re.findall(r"__global__\s+__launch_bounds__\([^)]*\)\s+void %s\(" % kernel, code[f])) == 1, kernel
