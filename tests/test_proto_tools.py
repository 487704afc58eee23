"""The six batch tools (bsom, bng, glvq, grlvq, gmlvq, rslvq) and the host-library functions behind them state what they
share once: the batch tools' front end in host/pak_io.c, the final figures and the training prologue in host/pak_engine.c,
the rank function over data blocks in host/pak_ranks.c.

Three parts, none of which needs a GPU.  (1) Read from the source, in the manner of test_proto_drivers.py.  (2) Every
refusal that moved, whole: exit status, the entire stderr and an empty stdout, against literals recorded from the build of
the commit before the move -- the tools must go on saying what they said, and refusing in the order they did.  (3) The
front end's functions that return rather than exit, as a stand-alone program under AddressSanitizer and UBSan.

Two things the tools share were left where they were, because sharing them would have reordered a refusal or made the
files longer:
  * "-gpus together with -buffer" stays in bsom.c and glvq.c.  bsom refuses "-missing together with -gpus" between the
    range checks and this one, so a shared parser that ended with the pair check would make `bsom -missing -gpus 2 -buffer 5`
    name the wrong pair.
  * the loop over the pieces of a buffered epoch stays in batchmap_training and glvq_training_buffered.  As one walk that
    hands each piece to the caller's accumulate it needs a callback type, two callbacks and a context per caller: 12 lines
    more than the two loops of six lines it replaces.  Both loops now mirror a piece through the one pak_mirror_rows."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_host_io_unit import INC, PAK_IO, SAN_ENV, SANITIZED, HELPERS

HOST = os.path.join(ROOT, "som_lvq_pak_amd", "host")
BIN = os.path.join(HOST, "bin")
TOOLS = ("bsom", "bng", "glvq", "grlvq", "gmlvq", "rslvq")


# ------------------------------------------------------------------------------------------------ stated once
def _code():
    """file name -> text without comments, for every .c file of host/ itself"""
    out = {}
    for f in sorted(os.listdir(HOST)):
        if f.endswith(".c"):
            text = open(os.path.join(HOST, f), errors="replace").read()
            out[f] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
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


def _sites(code, literal, pattern=None):
    pattern = pattern or re.escape(literal)
    return {f: len(re.findall(pattern, t)) for f, t in code.items() if re.search(pattern, t)}


def test_refusals_and_report_lines_are_written_once():
    code = _code()
    for literal in ("has no labels on row", "carries one label", "which no codebook row carries", "is negative or not a number",
                    "outside 1 .. 64", "final cost %.17g"):
        assert _sites(code, literal) == {"pak_io.c": 1}, literal
    # the per-epoch line; the final line's format ends in the same words, so that one is told apart by its first
    assert _sites(code, None, r"(?<!final )cost %\.17g accuracy") == {"pak_io.c": 1}
    assert _sites(code, "cost %.17g accuracy") == {"pak_io.c": 2}
    # masked inputs: once for codebooks, once for data -- bsom's "without -missing" is the tail it hands in
    assert _sites(code, None, r"codebook %s has masked components \(x\): not supported") == {"pak_io.c": 1}
    assert _sites(code, None, r"data %s has masked components \(x\): not supported") == {"pak_io.c": 1}
    assert _sites(code, ' without -missing"') == {"bsom.c": 1}
    masked = _function_body(code["pak_io.c"], "int pak_masked_inputs(")
    assert masked.index("io->codes->masks") < masked.index("io->data->masks")
    # the labelled-inputs check keeps its order
    lab = _function_body(code["pak_io.c"], "int pak_labelled_inputs(")
    order = [lab.index(s) for s in ('unlabelled(tool, io->codes, "codebook"', 'unlabelled(tool, io->data, "data"', "carries one label",
                                    "which no codebook row carries")]
    assert order == sorted(order)
    # -v, as the six tools read it
    verbose = _function_body(code["pak_io.c"], "int pak_batch_verbose(")
    order = [verbose.index(s) for s in ('"-v", OPTION2)', "global_options(argc, argv)", '"-v", OPTION)', "verbose_level = 1")]
    assert order == sorted(order)
    assert _sites(code, None, r'"-v", OPTION2') == {"pak_io.c": 1}
    # the two statements that end a run, in the six tools (the ports of SOM_PAK and LVQ_PAK keep theirs)
    assert "Codebook entries are saved to file" in _function_body(code["pak_io.c"], "int pak_save_codes(")
    for tool in TOOLS:
        text = code[tool + ".c"]
        assert "pak_batch_verbose(argc, argv)" in text and "pak_save_codes(" in text and "pak_masked_inputs(" in text, tool
        assert "Codebook entries are saved" not in text and "save_entries" not in text and "fprintf(stdout, \"final" not in text, tool
        assert ("pak_labelled_inputs(" in text) == (tool in ("glvq", "grlvq", "gmlvq", "rslvq")), tool
    # kept at its two sites (see the module's docstring)
    assert _sites(code, "-gpus together with -buffer") == {"bsom.c": 1, "glvq.c": 1}
    assert _sites(code, "pak_pieces_cli(argc, argv") == {"bsom.c": 1, "glvq.c": 1}
    bsom = code["bsom.c"]
    assert bsom.index("pak_pieces_cli(") < bsom.index("-missing together with -gpus") < bsom.index("-gpus together with -buffer")
    # the front end stays free of the engine
    assert "somhip_" not in code["pak_io.c"]


def test_the_rates_are_formed_in_one_place():
    code = _code()
    assert _sites(code, None, r"\(float\)\s*\(\s*(?:\w+->)?epochs - t\s*\)") == {"pak_io.c": 1}
    assert "return a * (float)(epochs - t) / (float)epochs;" in _function_body(code["pak_io.c"], "float pak_linear_rate(")
    # the radius calls the rate: 1.0f + ((r - 1.0f) * x / y) is the tree of the expression it replaces
    assert "return 1.0f + pak_linear_rate(r - 1.0f, epochs, t);" in _function_body(code["pak_io.c"], "float pak_linear_radius(")
    assert _sites(code, "pak_linear_radius(") == {"pak_io.c": 1, "bsom.c": 1, "pak_engine.c": 1}
    assert "pak_linear_rate(teach->alpha, epochs, t)" in _function_body(code["pak_engine.c"], "int glvq_training_buffered(")


def test_the_engine_side_shares_its_figures_mirrors_and_opening():
    eng = _code()["pak_engine.c"]
    assert eng.count("1.0 / (1.0 + exp(") == 1 and "1.0 / (1.0 + exp(" in _function_body(eng, "static void final_figures(")
    for head in ("int grlvq_training(", "int gmlvq_training("):
        assert _function_body(eng, head).count("final_figures(d, i, n, sigmoid_beta, final_cost, final_correct)") == 1, head
    # one body mirrors a block of rows, told whether to carry labels; labels materialise a gen: source first
    assert "pak_mirror_data_rows" not in eng and "pak_mirror_labelled_rows" not in eng
    rows = _function_body(eng, "somhip_dataset *pak_mirror_rows(")
    assert rows.index("with_labels && pak_materialize(data)") < rows.index("somhip_dataset_generate(") < rows.index("somhip_dataset_create(")
    # "can't get data" under the caller's name: pak_check_inputs says it for every batch training
    assert len(re.findall(r'"%s: can\'t get data\\n"', eng)) == 1
    opening = _function_body(eng, "static int batch_open(")
    assert opening.index("pak_check_inputs(teach, who, 0)") < opening.index("mirrors_open(")
    for head, who, labels in (("int glvq_training(", "glvq_training", 1), ("int rslvq_training(", "rslvq_training", 1),
                              ("int grlvq_training(", "grlvq_training", 1), ("int gmlvq_training(", "gmlvq_training", 1),
                              ("int ng_training(", "ng_training", 0), ("int ng_training_dense(", "ng_training_dense", 0),
                              ("static int batchmap_training(", "som_batchmap_training", 0)):
        assert 'batch_open(teach, "%s", %d, &m)' % (who, labels) in _function_body(eng, head), head
    # the buffered epochs keep their loops (see the module's docstring): two sites, one mirror function
    for head, labels in (("static int batchmap_training(", 0), ("int glvq_training_buffered(", 1)):
        body = _function_body(eng, head)
        assert body.count("first += buffer") == 1 and body.count("pak_mirror_rows(teach->data, first, c, %d)" % labels) == 1, head
    assert eng.count("pak_mirror_rows(") == 3


def test_one_rank_function_drives_the_data_blocks():
    ranks = _code()["pak_ranks.c"]
    assert ranks.count("data rows [%ld, %ld), state by %s") == 1
    body = _function_body(ranks, "static int block_training_rank(")
    assert "data rows [%ld, %ld), state by %s" in body and "rank_comm_open(" in body
    assert "m->train(m, cb, ds, r1 - r0, comm, &f)" in body and '"%s (rank %d): %s\\n", m->who' in body
    for head, who, labels, train, flags in (
            ("int som_batchmap_training_multi(", "som_batchmap_training", 0, "batchmap_over_ranks", "PAK_CHECK_SOM | PAK_CHECK_RANKS"),
            ("int glvq_training_multi(", "glvq_training", 1, "glvq_over_ranks", "PAK_CHECK_RANKS")):
        entry = _function_body(ranks, head)
        assert "pak_run_ranks(gpus, block_training_rank, &m)" in entry, head
        assert 'pak_check_inputs(teach, "%s", %s)' % (who, flags) in entry, head
        assert '"%s", %d, %s,' % (who, labels, train) in entry, head
    assert "somhip_som_batchmap_ranks(cb, ds, &p, comm, f->qerror)" in _function_body(ranks, "static int batchmap_over_ranks(")
    assert "somhip_glvq_train_ranks(cb, ds, &p, comm, f->cost, f->correct)" in _function_body(ranks, "static int glvq_over_ranks(")
    # the public signatures are the ones the tools were written against
    header = re.sub(r"\s+", " ", open(os.path.join(HOST, "pak.h")).read())
    assert ("int som_batchmap_training_multi(struct teach_params *teach, long epochs, float *qerror, int gpus, "
            "int (*after)(struct teach_params *, void *), void *arg);") in header
    assert ("int glvq_training_multi(struct teach_params *teach, long epochs, float sigmoid_beta, double *cost, int64_t *correct, int gpus, "
            "int (*after)(struct teach_params *, void *), void *arg);") in header


# ------------------------------------------------------------------------------------------------ the refusals, whole
@pytest.fixture(scope="module")
def built():
    lib = os.path.join(ROOT, "som_lvq_pak_amd", "libsomhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    return lib


@pytest.fixture(scope="module")
def tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in TOOLS):
        subprocess.check_call(["make", "-s", "-C", HOST])
    return BIN


FILES = {
    "lab.cod": "2\n0 0 a\n1 1 b\n1 0 b\n",
    "lab.dat": "2\n0 0.1 a\n1 0.9 b\n0.2 0 a\n0.9 0.2 b\n",
    "nolab.cod": "2\n0 0 a\n1 1\n1 0 b\n",
    "nolab.dat": "2\n0 0.1 a\n1 0.9 b\n0.2 0\n0.9 0.2 b\n",
    "one.cod": "2\n0 0 a\n1 1 a\n1 0 a\n",
    "unk.dat": "2\n0 0.1 a\n1 0.9 b\n0.2 0 c\n0.9 0.2 d\n",
    "x.cod": "2\n0 0 a\nx 1 b\n1 0 b\n",
    "x.dat": "2\n0 0.1 a\n1 x b\n0.2 0 a\n0.9 0.2 b\n",
    "m.cod": "2 hexa 2 2 bubble\n0 0\n1 0\n0 1\n1 1\n",
    "xm.cod": "2 hexa 2 2 bubble\nx 0\n1 0\n0 1\n1 1\n",
    "m.dat": "2\n0 0.1\n1 0.9\n0.2 0\n0.9 0.2\n",
}

# (tool, arguments, exit status, stderr): what the build of the commit before the front end was shared answered, run in a
# directory that holds FILES, with no device visible.  stdout was empty every time.  In order: each bad rate per option and
# tool, and which of several wins; -epochs below its bound, and without -rin / -oin; the tools' other numeric refusals
# around them; -buffer and -gpus out of range, together, and with -missing; masked codebooks and data; the four label
# checks and their precedence; and which missing required option is named first.
CASES = [
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -0.5', 1, 'glvq: -alpha -0.5 is negative or not a number\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha nan', 1, 'glvq: -alpha nan is negative or not a number\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigmoid -0.5', 1, 'glvq: -sigmoid -0.5 is negative or not a number\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigmoid nan', 1, 'glvq: -sigmoid nan is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -0.5 -eps 0.01', 1, 'grlvq: -alpha -0.5 is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha nan -eps 0.01', 1, 'grlvq: -alpha nan is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps -0.5', 1, 'grlvq: -eps -0.5 is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps nan', 1, 'grlvq: -eps nan is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -sigmoid -0.5', 1, 'grlvq: -sigmoid -0.5 is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -sigmoid nan', 1, 'grlvq: -sigmoid nan is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -0.5 -eps 0.01', 1, 'gmlvq: -alpha -0.5 is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha nan -eps 0.01', 1, 'gmlvq: -alpha nan is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps -0.5', 1, 'gmlvq: -eps -0.5 is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps nan', 1, 'gmlvq: -eps nan is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -sigmoid -0.5', 1, 'gmlvq: -sigmoid -0.5 is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -sigmoid nan', 1, 'gmlvq: -sigmoid nan is negative or not a number\n'),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -0.5 -sigma2 1', 1, 'rslvq: -alpha -0.5 is negative or not a number\n'),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha nan -sigma2 1', 1, 'rslvq: -alpha nan is negative or not a number\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -1 -eps -2 -sigmoid -3', 1, 'grlvq: -alpha -1 is negative or not a number\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps -2 -sigmoid -3', 1, 'gmlvq: -eps -2 is negative or not a number\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 0 -radius 2', 1, 'bsom: -epochs 0 < 1\n'),
    ('bng', '-cin m.cod -din m.dat -cout o.cod -epochs 0', 1, 'bng: -epochs 0 < 1\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 0 -alpha 0.1', 1, 'glvq: -epochs 0 < 1\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 0 -alpha -1', 1, 'glvq: -epochs 0 < 1\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs -1 -alpha 0.1 -eps 0.01', 1, 'grlvq: -epochs -1 < 0\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs -1 -alpha 0.1 -eps 0.01', 1, 'gmlvq: -epochs -1 < 0\n'),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs -1 -alpha 0.1 -sigma2 1', 1, 'rslvq: -epochs -1 < 0\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 0 -alpha 0.1 -eps 0.01', 1, 'grlvq: -epochs 0 evaluates a trained model and needs its relevances (-rin)\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 0 -alpha 0.1 -eps 0.01', 1, 'gmlvq: -epochs 0 evaluates a trained model and needs its matrix (-oin)\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 0 -alpha -1 -eps 0.01', 1, 'grlvq: -epochs 0 evaluates a trained model and needs its relevances (-rin)\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 0.5', 1, 'bsom: -radius 0.5 < 1\n'),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 0', 1, 'rslvq: -sigma2 0 is not a finite number above 0\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -rank 0', 1, 'gmlvq: -rank 0 < 1\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01 -rank 3', 1, 'gmlvq: -rank 3 is larger than the dimension 2\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -buffer -1', 1, 'bsom: -buffer -1 < 0\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -buffer -1 -gpus 0', 1, 'bsom: -buffer -1 < 0\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -gpus 0', 1, 'bsom: -gpus 0 outside 1 .. 64\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -gpus 65', 1, 'bsom: -gpus 65 outside 1 .. 64\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -gpus 2 -buffer 5', 1, 'bsom: -gpus together with -buffer is not available (give one of the two)\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -gpus 1 -buffer 5', 1, 'bsom: -gpus together with -buffer is not available (give one of the two)\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -buffer 0', 1, 'glvq: -buffer 0 < 1\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -buffer 0 -gpus 0', 1, 'glvq: -buffer 0 < 1\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -gpus 0', 1, 'glvq: -gpus 0 outside 1 .. 64\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -gpus 65', 1, 'glvq: -gpus 65 outside 1 .. 64\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -gpus 2 -buffer 5', 1, 'glvq: -gpus together with -buffer is not available (give one of the two)\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -gpus 1 -buffer 5', 1, 'glvq: -gpus together with -buffer is not available (give one of the two)\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -buffer -3 -gpus 2', 1, 'glvq: -buffer -3 < 1\n'),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha -1 -gpus 99', 1, 'glvq: -alpha -1 is negative or not a number\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing -gpus 2 -buffer 5', 1, 'bsom: -missing together with -gpus is not available (the ranks train without masks)\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing -gpus 2', 1, 'bsom: -missing together with -gpus is not available (the ranks train without masks)\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing -gpus 99 -buffer 5', 1, 'bsom: -gpus 99 outside 1 .. 64\n'),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing -buffer -2', 1, 'bsom: -buffer -2 < 0\n'),
    ('bsom', '-cin xm.cod -din m.dat -cout o.cod -epochs 2 -radius 2', 1, 'bsom: codebook xm.cod has masked components (x): not supported\n'),
    ('bsom', '-cin xm.cod -din x.dat -cout o.cod -epochs 2 -radius 2', 1, 'bsom: codebook xm.cod has masked components (x): not supported\n'),
    ('bsom', '-cin m.cod -din x.dat -cout o.cod -epochs 2 -radius 2', 1, 'bsom: data x.dat has masked components (x): not supported without -missing\n'),
    ('bng', '-cin xm.cod -din m.dat -cout o.cod -epochs 2', 1, 'bng: codebook xm.cod has masked components (x): not supported\n'),
    ('bng', '-cin xm.cod -din x.dat -cout o.cod -epochs 2', 1, 'bng: codebook xm.cod has masked components (x): not supported\n'),
    ('bng', '-cin m.cod -din x.dat -cout o.cod -epochs 2', 1, 'bng: data x.dat has masked components (x): not supported\n'),
    ('glvq', '-cin x.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: codebook x.cod has masked components (x): not supported\n'),
    ('glvq', '-cin x.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: codebook x.cod has masked components (x): not supported\n'),
    ('glvq', '-cin lab.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: data x.dat has masked components (x): not supported\n'),
    ('grlvq', '-cin x.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: codebook x.cod has masked components (x): not supported\n'),
    ('grlvq', '-cin x.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: codebook x.cod has masked components (x): not supported\n'),
    ('grlvq', '-cin lab.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: data x.dat has masked components (x): not supported\n'),
    ('gmlvq', '-cin x.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: codebook x.cod has masked components (x): not supported\n'),
    ('gmlvq', '-cin x.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: codebook x.cod has masked components (x): not supported\n'),
    ('gmlvq', '-cin lab.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: data x.dat has masked components (x): not supported\n'),
    ('rslvq', '-cin x.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: codebook x.cod has masked components (x): not supported\n'),
    ('rslvq', '-cin x.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: codebook x.cod has masked components (x): not supported\n'),
    ('rslvq', '-cin lab.cod -din x.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: data x.dat has masked components (x): not supported\n'),
    ('bsom', '-cin xm.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing', 1, 'bsom: codebook xm.cod has masked components (x): not supported\n'),
    ('bsom', '-cin xm.cod -din x.dat -cout o.cod -epochs 2 -radius 2 -missing', 1, 'bsom: codebook xm.cod has masked components (x): not supported\n'),
    ('bsom', '-cin m.cod -din x.dat -cout o.cod -epochs 2 -radius 2 -buffer 2', 1, 'bsom: data x.dat has masked components (x): not supported without -missing\n'),
    ('glvq', '-cin nolab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: codebook nolab.cod has no labels on row 1\n'),
    ('glvq', '-cin nolab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: codebook nolab.cod has no labels on row 1\n'),
    ('glvq', '-cin lab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: data nolab.dat has no labels on row 2\n'),
    ('glvq', '-cin one.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: data nolab.dat has no labels on row 2\n'),
    ('glvq', '-cin one.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('glvq', '-cin one.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('glvq', '-cin lab.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: data row 2 carries label c, which no codebook row carries\n'),
    ('glvq', '-cin x.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1', 1, 'glvq: codebook x.cod has masked components (x): not supported\n'),
    ('grlvq', '-cin nolab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: codebook nolab.cod has no labels on row 1\n'),
    ('grlvq', '-cin nolab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: codebook nolab.cod has no labels on row 1\n'),
    ('grlvq', '-cin lab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: data nolab.dat has no labels on row 2\n'),
    ('grlvq', '-cin one.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: data nolab.dat has no labels on row 2\n'),
    ('grlvq', '-cin one.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('grlvq', '-cin one.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('grlvq', '-cin lab.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: data row 2 carries label c, which no codebook row carries\n'),
    ('grlvq', '-cin x.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'grlvq: codebook x.cod has masked components (x): not supported\n'),
    ('gmlvq', '-cin nolab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: codebook nolab.cod has no labels on row 1\n'),
    ('gmlvq', '-cin nolab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: codebook nolab.cod has no labels on row 1\n'),
    ('gmlvq', '-cin lab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: data nolab.dat has no labels on row 2\n'),
    ('gmlvq', '-cin one.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: data nolab.dat has no labels on row 2\n'),
    ('gmlvq', '-cin one.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('gmlvq', '-cin one.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('gmlvq', '-cin lab.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: data row 2 carries label c, which no codebook row carries\n'),
    ('gmlvq', '-cin x.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 1, 'gmlvq: codebook x.cod has masked components (x): not supported\n'),
    ('rslvq', '-cin nolab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: codebook nolab.cod has no labels on row 1\n'),
    ('rslvq', '-cin nolab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: codebook nolab.cod has no labels on row 1\n'),
    ('rslvq', '-cin lab.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: data nolab.dat has no labels on row 2\n'),
    ('rslvq', '-cin one.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: data nolab.dat has no labels on row 2\n'),
    ('rslvq', '-cin one.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('rslvq', '-cin one.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: every row of codebook one.cod carries one label (no other class to be wrong with)\n'),
    ('rslvq', '-cin lab.cod -din unk.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: data row 2 carries label c, which no codebook row carries\n'),
    ('rslvq', '-cin x.cod -din nolab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 1, 'rslvq: codebook x.cod has masked components (x): not supported\n'),
    ('bsom', '', 255, "Can't find asked option -din\n"),
    ('bsom', '-v', 255, "Can't find asked option -din\n"),
    ('bsom', '-cin m.cod -cout o.cod -epochs 2 -radius 2', 255, "Can't find asked option -din\n"),
    ('bsom', '-din m.dat -cout o.cod -epochs 2 -radius 2', 255, "Can't find asked option -cin\n"),
    ('bsom', '-cin m.cod -din m.dat -epochs 2 -radius 2', 255, "Can't find asked option -cout\n"),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -radius 2', 255, "Can't find asked option -epochs\n"),
    ('bsom', '-cin m.cod -din m.dat -cout o.cod -epochs 2', 255, "Can't find asked option -radius\n"),
    ('bsom', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('bng', '', 255, "Can't find asked option -din\n"),
    ('bng', '-v', 255, "Can't find asked option -din\n"),
    ('bng', '-cin m.cod -cout o.cod -epochs 2', 255, "Can't find asked option -din\n"),
    ('bng', '-din m.dat -cout o.cod -epochs 2', 255, "Can't find asked option -cin\n"),
    ('bng', '-cin m.cod -din m.dat -epochs 2', 255, "Can't find asked option -cout\n"),
    ('bng', '-cin m.cod -din m.dat -cout o.cod', 255, "Can't find asked option -epochs\n"),
    ('bng', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('glvq', '', 255, "Can't find asked option -din\n"),
    ('glvq', '-v', 255, "Can't find asked option -din\n"),
    ('glvq', '-cin lab.cod -cout o.cod -epochs 2 -alpha 0.1', 255, "Can't find asked option -din\n"),
    ('glvq', '-din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 255, "Can't find asked option -cin\n"),
    ('glvq', '-cin lab.cod -din lab.dat -epochs 2 -alpha 0.1', 255, "Can't find asked option -cout\n"),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -alpha 0.1', 255, "Can't find asked option -epochs\n"),
    ('glvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2', 255, "Can't find asked option -alpha\n"),
    ('glvq', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('grlvq', '', 255, "Can't find asked option -din\n"),
    ('grlvq', '-v', 255, "Can't find asked option -din\n"),
    ('grlvq', '-cin lab.cod -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -din\n"),
    ('grlvq', '-din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -cin\n"),
    ('grlvq', '-cin lab.cod -din lab.dat -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -cout\n"),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -alpha 0.1 -eps 0.01', 255, "Can't find asked option -epochs\n"),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -eps 0.01', 255, "Can't find asked option -alpha\n"),
    ('grlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 255, "Can't find asked option -eps\n"),
    ('grlvq', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('gmlvq', '', 255, "Can't find asked option -din\n"),
    ('gmlvq', '-v', 255, "Can't find asked option -din\n"),
    ('gmlvq', '-cin lab.cod -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -din\n"),
    ('gmlvq', '-din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -cin\n"),
    ('gmlvq', '-cin lab.cod -din lab.dat -epochs 2 -alpha 0.1 -eps 0.01', 255, "Can't find asked option -cout\n"),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -alpha 0.1 -eps 0.01', 255, "Can't find asked option -epochs\n"),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -eps 0.01', 255, "Can't find asked option -alpha\n"),
    ('gmlvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 255, "Can't find asked option -eps\n"),
    ('gmlvq', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('rslvq', '', 255, "Can't find asked option -din\n"),
    ('rslvq', '-v', 255, "Can't find asked option -din\n"),
    ('rslvq', '-cin lab.cod -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 255, "Can't find asked option -din\n"),
    ('rslvq', '-din lab.dat -cout o.cod -epochs 2 -alpha 0.1 -sigma2 1', 255, "Can't find asked option -cin\n"),
    ('rslvq', '-cin lab.cod -din lab.dat -epochs 2 -alpha 0.1 -sigma2 1', 255, "Can't find asked option -cout\n"),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -alpha 0.1 -sigma2 1', 255, "Can't find asked option -epochs\n"),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -sigma2 1', 255, "Can't find asked option -alpha\n"),
    ('rslvq', '-cin lab.cod -din lab.dat -cout o.cod -epochs 2 -alpha 0.1', 255, "Can't find asked option -sigma2\n"),
    ('rslvq', '-din lab.dat -cout o.cod', 255, "Can't find asked option -cin\n"),
    ('grlvq', '-cin lab.cod -din lab.dat -epochs 0 -sigma2 1 -alpha -1', 1, 'grlvq: -epochs 0 evaluates a trained model and needs its relevances (-rin)\n'),
    ('grlvq', '-cin lab.cod -din lab.dat -epochs 1 -sigma2 1 -alpha -1', 255, "Can't find asked option -cout\n"),
    ('gmlvq', '-cin lab.cod -din lab.dat -epochs 0 -sigma2 1 -alpha -1', 1, 'gmlvq: -epochs 0 evaluates a trained model and needs its matrix (-oin)\n'),
    ('gmlvq', '-cin lab.cod -din lab.dat -epochs 1 -sigma2 1 -alpha -1', 255, "Can't find asked option -cout\n"),
    ('rslvq', '-cin lab.cod -din lab.dat -epochs 0 -sigma2 1 -alpha -1', 1, 'rslvq: -alpha -1 is negative or not a number\n'),
    ('rslvq', '-cin lab.cod -din lab.dat -epochs 1 -sigma2 1 -alpha -1', 255, "Can't find asked option -cout\n"),
]

HELP = {
    'bsom':
        'bsom - teach self-organizing map, batch map (MI355X engine)\n'
        'Required:  -cin file  -din file  -cout file  -epochs T  -radius R\n'
        'Optional:  -v (one line per epoch to stdout: epoch, radius, quantization error before it)\n'
        '           -buffer N (the device holds N data rows at a time; same result)\n'
        "           -gpus G (one process per GPU, the data's rows divided over them; same result; not with -buffer;\n"
        "                    SOMHIP_COMM=rccl|sockets in the environment names the ranks' transport and, as with vsom,\n"
        '                    sends even one rank through it)\n'
        '           -missing (take data with missing components, x: a sample is matched over the components it has, a\n'
        '                     component of a model vector becomes the mean of the samples that know it; data without x\n'
        '                     give the same map as without the option; works with -buffer, not with -gpus)\n'
        "Topology and neighbourhood come from the codebook's header.\n"
        'Files:     text (.dat/.cod), raw fp32 (a name ending in .f32; see datconv), or -din gen:k=..,dim=..,n=..,seed=..\n',
    'bng':
        'bng - train a codebook, batch neural gas (MI355X engine)\n'
        'Required:  -cin file  -din file  -cout file  -epochs T\n'
        'Optional:  -lambda L0 (the neighbourhood range in ranks the run starts from; default min(units, 256) / 2)\n'
        '           -lambda_end Le (... and ends at; default 0.01)\n'
        '           -ranks K (the nearest units every sample feeds, 1 .. 256; default 1 + floor(17 lambda), at most 256)\n'
        '           -dense (every unit is fed, whatever its rank: no truncation, at most 4096 units, no -ranks)\n'
        '           -v (one line per epoch to stdout: epoch, lambda, ranks and the quantization error before it)\n'
        'Any codebook is taken; its header and labels are written back as they were read.\n'
        'Files:     text (.dat/.cod), raw fp32 (a name ending in .f32; see datconv), or -din gen:k=..,dim=..,n=..,seed=..\n',
    'glvq':
        'glvq - train a labelled codebook, batch GLVQ (MI355X engine)\n'
        'Required:  -cin file  -din file  -cout file  -epochs T  -alpha A\n'
        'Optional:  -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n'
        '           -v (one line per epoch to stdout: epoch, alpha, cost and accuracy before it)\n'
        '           -buffer N (the device holds N data rows at a time; same result)\n'
        "           -gpus G (one process per GPU, the data's rows divided over them; same result; not with -buffer;\n"
        "                    SOMHIP_COMM=rccl|sockets in the environment names the ranks' transport and, as with bsom,\n"
        '                    sends even one rank through it)\n'
        '-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n'
        'Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n',
    'grlvq':
        'grlvq - train a labelled codebook and its relevances, batch GRLVQ (MI355X engine)\n'
        'Required:  -cin file  -din file  -cout file  -epochs T  -alpha A  -eps E\n'
        'Optional:  -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n'
        '           -rin file (the relevances to start from, taken as they are; without it 1 / dim each)\n'
        '           -rout file (the relevances the run ends with)\n'
        '           -v (one line per epoch to stdout: epoch, alpha, eps, cost and accuracy before it)\n'
        '-epochs 0 with -rin trains nothing and writes no codebook: it prints the cost and accuracy of -cin under -rin.\n'
        'A relevance file is a first line with the dimension, then one value per line.\n'
        '-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n'
        'Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n',
    'gmlvq':
        'gmlvq - train a labelled codebook and its matrix metric, batch GMLVQ (MI355X engine)\n'
        'Required:  -cin file  -din file  -cout file  -epochs T  -alpha A  -eps E\n'
        'Optional:  -rank M (the rows of Omega, 1 .. dim; without it dim, or the rows of -oin)\n'
        '           -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n'
        '           -oin file (the matrix to start from, taken as it is; without it 1 / sqrt(dim) where k mod M == r)\n'
        '           -oout file (the matrix the run ends with)\n'
        '           -pout file (the data projected by that matrix: a .dat of dimension M with the labels)\n'
        '           -v (one line per epoch to stdout: epoch, alpha, eps, cost and accuracy before it)\n'
        '-epochs 0 with -oin trains nothing and writes no codebook: it prints the cost and accuracy of -cin under -oin.\n'
        "An omega file is a first line 'M dim', then M lines of dim values.\n"
        '-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n'
        'Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n',
    'rslvq':
        'rslvq - train a labelled codebook, batch Robust Soft LVQ (MI355X engine)\n'
        'Required:  -cin file  -din file  -epochs T  -sigma2 S  (and -cout file  -alpha A  where T > 0)\n'
        'Optional:  -pout file (one line per data row: its label and P(label | x) under the codebook the tool ends with)\n'
        '           -v (one line per epoch to stdout: epoch, alpha, cost and accuracy before it)\n'
        '-epochs 0 trains nothing and writes no codebook: it prints the cost and accuracy of -cin.\n'
        "-sigma2 is the squared width of the mixture's components; -alpha has the unit of a squared distance.\n"
        'Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n',
}

NOWHERE = {"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}      # an engine, were one asked for, would fail


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("refusals")
    for name, text in FILES.items():
        (d / name).write_text(text)
    return d


def run(tool, args, cwd):
    return subprocess.run([os.path.join(BIN, tool)] + args.split(), cwd=str(cwd), env=dict(os.environ, **NOWHERE),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("tool", TOOLS)
def test_every_refusal_is_the_one_it_was(tools, workdir, tool):
    mine = [c for c in CASES if c[0] == tool]
    assert len(mine) >= 11                                      # bng: bounds, masks and required options alone
    for _, args, status, stderr in mine:
        p = run(tool, args, workdir)
        assert (p.returncode, p.stdout, p.stderr) == (status, "", stderr), (tool, args, p.returncode, p.stdout, p.stderr)
    assert not (workdir / "o.cod").exists()


def test_the_matrix_covers_what_moved():
    """the cases are there: every tool's rates, bounds, masks, labels and required options"""
    said = lambda tool, word: [c for c in CASES if c[0] == tool and word in c[3]]
    for tool, rates in (("glvq", ("-alpha", "-sigmoid")), ("grlvq", ("-alpha", "-eps", "-sigmoid")), ("gmlvq", ("-alpha", "-eps", "-sigmoid")),
                        ("rslvq", ("-alpha",))):
        for opt in rates:
            assert len(said(tool, "%s: %s " % (tool, opt))) >= 2, (tool, opt)            # negative, and not a number
        for word in ("codebook nolab.cod has no labels on row 1", "data nolab.dat has no labels on row 2", "carries one label",
                     "data row 2 carries label c, which no codebook row carries"):
            assert said(tool, word), (tool, word)
    for tool in TOOLS:
        assert said(tool, "%s: -epochs " % tool) and said(tool, "codebook") and said(tool, "data x.dat has masked components")
        assert len({c[3] for c in CASES if c[0] == tool and c[2] == 255}) >= 4, tool      # -din, -cin, -cout, -epochs, ... by name
    for tool in ("bsom", "glvq"):
        for word in ("-buffer", "-gpus 0 outside", "-gpus 65 outside", "-gpus together with -buffer"):
            assert said(tool, "%s: %s" % (tool, word)), (tool, word)
    assert ("bsom", "-cin m.cod -din m.dat -cout o.cod -epochs 2 -radius 2 -missing -gpus 2 -buffer 5", 1,
            "bsom: -missing together with -gpus is not available (the ranks train without masks)\n") in CASES
    assert said("bsom", "not supported without -missing\n") and said("grlvq", "(-rin)") and said("gmlvq", "(-oin)")


@pytest.mark.parametrize("tool", TOOLS)
def test_help_is_the_text_it_was(tools, workdir, tool):
    for args in ("-help", "-v -help -epochs 0"):                 # before any required option is looked for
        p = run(tool, args, workdir)
        assert (p.returncode, p.stdout, p.stderr) == (0, HELP[tool], ""), (tool, args)


def test_masked_data_pass_bsom_missing(tools, workdir):
    """with -missing the masked data are no reason to refuse: the run goes on to ask for an engine, which no device visible
    denies it -- in the engine's words, not the front end's"""
    p = run("bsom", "-cin m.cod -din x.dat -cout o.cod -epochs 2 -radius 2 -missing", workdir)
    assert p.returncode == 1 and p.stdout == "" and p.stderr and "masked components" not in p.stderr, p.stderr
    assert not (workdir / "o.cod").exists()


# ------------------------------------------------------------------------------------------------ under sanitizers
def test_front_end_runs_clean_under_sanitizers(tmp_path):
    """tests/helpers/batch_front_check.c, built from it and pak_io.c alone: the labelled- and masked-inputs checks on golden
    files and on files with each defect, the two rates against the written-out expressions bit for bit, the line writers
    read back, -v and the save -- the same report plain and sanitized, no failed check, not a word from the sanitizers"""
    files = [os.path.join(GOLDEN, "data", "ex1.dat"), os.path.join(GOLDEN, "data", "ex2.dat"), os.path.join(GOLDEN, "cli", "lvq_init.cod")]
    reports = {}
    for kind, flags, env in (("plain", ["-O2"], None), ("sanitized", SANITIZED, SAN_ENV)):
        work = tmp_path / kind
        work.mkdir()
        exe = str(work / "batch_front_check")
        subprocess.check_call(["gcc", *flags, *INC, "-o", exe, os.path.join(HELPERS, "batch_front_check.c"), PAK_IO, "-lm"])
        p = subprocess.run([exe] + files, cwd=work, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, (kind, p.stdout[-2000:], p.stderr[-4000:])
        assert p.stdout.strip().endswith("failed checks 0") and "FAILED" not in p.stdout, p.stdout
        reports[kind] = p
    assert reports["plain"].stdout == reports["sanitized"].stdout
    assert reports["sanitized"].stderr == ""
    out = reports["plain"].stdout
    assert "ok inputs ex2.dat ex1.dat -> 0" in out                                   # a golden pair that the tools take
    assert "ok inputs lvq_init.cod ex1.dat -> 1 tool: data row 1424 carries label F, which no codebook row carries" in out
    assert "rates 4024 each, 0 differ" in out and len(re.findall(r"^ok ", out, flags=re.M)) == 23
