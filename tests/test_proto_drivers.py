"""The host drivers of the batch prototype trainers (K8 batch map, K9 glvq, K10 / K10d neural gas, K11 grlvq, K12 gmlvq,
K13 rslvq) state what they share once: csrc/host_proto.inc, and rows_written / stage_timing in csrc/somhip.hip.  Read from
the source, without a GPU, in the manner of test_build.py's test_lvq_driver_plans_once_and_launches_each_kernel_once."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "som_lvq_pak_amd", "csrc")
TRAINERS = ("host_proto.inc", "host_batchmap.inc", "host_glvq.inc", "host_grlvq.inc", "host_gmlvq.inc", "host_rslvq.inc",
            "host_ngas.inc", "host_ngas_dense.inc")


def _code():
    """file name -> text without comments, for every file under csrc/ (kernels/ under its own prefix)"""
    out = {}
    for dirpath, _, files in os.walk(CSRC):
        for f in sorted(files):
            path = os.path.join(dirpath, f)
            text = open(path, errors="replace").read()
            out[os.path.relpath(path, CSRC)] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
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


def _sites(code, pattern):
    return {f: len(re.findall(pattern, t)) for f, t in code.items() if re.search(pattern, t)}


def test_the_epoch_window_is_refused_in_one_place():
    code = _code()
    assert _sites(code, r'epochs \[[^"\n]*outside \[0, %lld\)') == {"host_proto.inc": 1}
    assert _sites(code, r"epochs %lld < 1") == {"host_proto.inc": 1}
    assert _sites(code, r"alpha %g is negative or not a number") == {"host_proto.inc": 1}
    # the rate: (float)(epochs - t) is formed in linear_rate and nowhere else
    assert _sites(code, r"\(float\)\s*\(\s*(?:p->)?epochs - t\s*\)") == {"host_proto.inc": 1}
    assert "(float)(epochs - t) / (float)epochs" in _function_body(code["host_proto.inc"], "static float linear_rate(")


def test_rows_are_declared_written_in_one_place():
    code = _code()
    # The prepared copies are dropped by rows_written.  Three more statements clear rowmajor_valid, and none of them says
    # "the rows were written": lvq_refresh_prepared keeps the re-split tiles and drops the row-major copy alone (1), and
    # somhip_debug_prepared (host_scan.inc) drops both to force the codebook pass it is asked about, writing no row and
    # closing no accumulation (1).
    assert _sites(code, r"->rowmajor_valid = false") == {"somhip.hip": 1, "host_lvq.inc": 1, "host_scan.inc": 1}
    assert "rowmajor_valid = false" in _function_body(code["somhip.hip"], "static void rows_written(")
    assert "close_accumulations(cb)" in _function_body(code["somhip.hip"], "static void rows_written(")
    lvq = _function_body(code["host_lvq.inc"], "static int lvq_refresh_prepared(")
    assert "cb->rowmajor_valid = false" in lvq and "rows_written(cb)" in lvq and "close_accumulations(cb)" in lvq
    assert "cb->rowmajor_valid = false" in _function_body(code["host_scan.inc"], 'extern "C" int somhip_debug_prepared(')
    # An accumulation is closed by close_accumulations (which rows_written calls), by codebook_release, which frees the
    # states, and nowhere else as a plain statement; the state free / end functions clear `open` together with `moved`.
    hip = code["somhip.hip"]
    for flag in ("bm_open", "gl_open"):
        assert _sites(code, r"->%s = false" % flag) == {"somhip.hip": 2}, flag
        assert ("%s = false" % flag) in _function_body(hip, "static void close_accumulations(")
        assert ("%s = false" % flag) in _function_body(hip, "static void codebook_release(somhip_codebook *cb) {")
    assert _sites(code, r"bm_open = cb->bm_moved = false") == {"host_batchmap.inc": 2}      # somhip_batchmap_end, _ranks' way out
    assert _sites(code, r"gl_open = cb->gl_moved = false") == {"host_glvq.inc": 1}          # glvq_state_free
    assert "gl_open = cb->gl_moved = false" in _function_body(code["host_glvq.inc"], "static void glvq_state_free(")
    # ... and opened by the state open functions and by the two owners that update from their own state
    assert _sites(code, r"bm_open = true") == {"host_batchmap.inc": 2}
    assert "bm_open = true" in _function_body(code["host_batchmap.inc"], "static int batchmap_state_open(")
    assert "bm_open = true" in _function_body(code["host_batchmap.inc"], 'extern "C" int somhip_batchmap_finish(')
    assert _sites(code, r"gl_open = (?:cb->gl_moved = )?true") == {"host_glvq.inc": 2}
    assert "gl_open = true" in _function_body(code["host_glvq.inc"], "static int glvq_state_open(")
    assert "gl_open = cb->gl_moved = true" in _function_body(code["host_glvq.inc"], "static int glvq_finish_state(")
    # every update stage of a trainer says so through the helper
    for f, head in (("host_batchmap.inc", "static int batchmap_combine_stage("), ("host_glvq.inc", "static int glvq_update_stage("),
                    ("host_grlvq.inc", "static int grlvq_update_stage("), ("host_gmlvq.inc", "static int gmlvq_update_stage("),
                    ("host_rslvq.inc", "static int rslvq_update_stage("), ("host_ngas.inc", "static int ng_update_stage("),
                    ("somhip.hip", "static int upload_rows(")):
        assert "rows_written(cb)" in _function_body(code[f], head), head


def _launches(code, kernel):
    """per trainer file, the LAUNCH / LAUNCH_TIMED statements whose kernel is `kernel` (a template's instantiations apart)"""
    pattern = r"\bLAUNCH(?:_TIMED\s*\(\s*[\w>-]+\s*,\s*[\w>-]+|\s*\(\s*[\w>-]+)\s*,\s*\(?\s*%s" % re.escape(kernel)
    return {f: len(re.findall(pattern, code[f])) for f in TRAINERS if re.search(pattern, code[f])}


def test_the_shared_stages_launch_from_one_site():
    code = _code()
    # one site each, in host_proto.inc: an if / else over the instantiations of one template is one site of two statements
    assert _launches(code, "k_scan_class<") == {"host_proto.inc": 2}                 # <32, 4> and <32, 1>
    assert _launches(code, "k_scan_class_weighted<") == {"host_proto.inc": 2}
    assert _launches(code, "k_glvq_pack_listed<") == {"host_proto.inc": 1}
    assert _launches(code, "k_knn_dist<SCAN_S>") == {"host_proto.inc": 1}
    assert _launches(code, "k_rslvq_sums<") == {"host_proto.inc": 2}                 # <true> and <false>: one site
    assert _launches(code, "k_pack_samples<") == {"host_proto.inc": 2}               # the scan's tiles of 32, the chunk stages' SCAN_S
    walk = _function_body(code["host_proto.inc"], "static int class_scan_walk(")
    for kernel in ("k_scan_class<GLVQ_S, GLVQ_R>", "k_scan_class<GLVQ_S, 1>", "k_scan_class_weighted<GLVQ_S, GLVQ_R>",
                   "k_scan_class_weighted<GLVQ_S, 1>", "k_glvq_pack_listed<GLVQ_S>", "k_pack_samples<GLVQ_S>"):
        assert walk.count(kernel) == 1, kernel
    assert walk.count("off += GLVQ_CHUNK") == 1 and walk.count("const bool wide =") == 1
    # the three searches walk it: K9 both ways (the run under its id, the list route's remainder untimed), K11 with the
    # relevance tile under its own id, K12 over its projected tiles under K9's
    flat = lambda f, head: re.sub(r"\s+", " ", _function_body(code[f], head))    # (the calls mark their arguments in comments)
    glvq = flat("host_glvq.inc", "static int glvq_search_stage(")
    assert glvq.count("class_scan_walk(") == 2 and "nullptr, KID_GLVQ_SEARCH, b.keys2)" in glvq and "b.rem, nullptr, -1, b.keys2)" in glvq
    assert "b.lam, KID_GRLVQ_SEARCH, b.g.keys2)" in flat("host_grlvq.inc", "static int grlvq_search_stage(")
    gmlvq = flat("host_gmlvq.inc", "static int gmlvq_search_stage(")
    assert "class_scan_walk(cb->e, b.pv, " in gmlvq and "(b.xt), nullptr, nullptr, KID_GLVQ_SEARCH, b.g.keys2)" in gmlvq
    # the decode of keys2 and the trailing column's loops are written once
    assert _sites(code, r"decode_key\(hk\[2 \* \(size_t\)s \+ 1\]") == {"host_proto.inc": 1}
    # (the batch map's debug combine keeps its own loop: its trailing column is the uint32 hit counts, converted)
    assert _sites({f: code[f] for f in TRAINERS}, r"memcpy\([^;\n]*\* \(d \+ 1\)") == {"host_proto.inc": 2, "host_batchmap.inc": 1}
    assert not re.search(r"\bmemcpy\b", code["host_rslvq.inc"])
    assert len(re.findall(r"\bchain \+= c\b", "".join(code[f] for f in TRAINERS))) == 1      # the cost figure


def test_timing_entry_points_share_one_body():
    code = _code()
    assert _sites(code, r"launches\[i\] = e->launches\[kid\[i\]\]") == {"somhip.hip": 1}
    entries = {}
    for f, t in code.items():
        for name in re.findall(r'extern "C" int (somhip_\w+_timing)\(', t):
            entries[name] = _function_body(t, 'extern "C" int %s(' % name)
    assert sorted(entries) == ["somhip_batchmap_timing", "somhip_conn_timing", "somhip_distortion_timing", "somhip_glvq_timing",
                               "somhip_gmlvq_timing", "somhip_grlvq_timing", "somhip_knn_timing", "somhip_knn_vote_timing",
                               "somhip_map_quality_timing", "somhip_mapset_timing", "somhip_ng_dense_timing", "somhip_ng_timing",
                               "somhip_rslvq_timing"]
    for name, body in entries.items():
        m = re.search(r"const int kid\[(\d)\] = \{([^}]*)\};\s*return stage_timing\(e, \"%s\", kid, (\d), launches, total_ms\);" % name, body)
        assert m and m.group(1) == m.group(3) and len(m.group(2).split(",")) == int(m.group(1)), name
