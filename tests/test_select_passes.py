"""The select passes of the two-level winner search at the edges of their tiles: k_l2_select (a thread holds four
consecutive samples, a workgroup 1024, an item is 1024 samples x a chunk of row groups) and k_rerank_select_lists.

Counts that are no multiple of 4, 32, 256 or 1024 (a quad that is partly live, a last 32-sample column that is partly
live, a last sample block that is partly inside the rows of wmin), one row group and a ragged last one, a map on the
ring route, every group listed for every sample (the heaviest contention on a column's counters, and the segment
overflow), zero samples and NaN.  Each case goes through the check of tests/test_rerank_select_lists.py: selections,
counters, overflow word and statistics against the numpy replay and against the dense selection, the keys against the
oracle.  A sample k_l2_select loses never reaches level 2 and the exact re-rank, so its key differs from the oracle's;
one it files twice, or a dead one it files, changes the counters.  Needs an MI355X:  pytest -m gpu."""
import pytest

import test_rerank_select_lists as RS
from test_scan_routes import TOPOL_HEXA, Case

pytestmark = pytest.mark.gpu

TWO, RING = RS.TWO, RS.RING

CASES = [
    Case("count255", 1024, 32, 255, TWO, cls="dups"),          # 63 quads + 3 samples; 8 columns, the last with 31
    Case("count257", 1024, 32, 257, TWO, cls="dups"),          # a quad with one live sample, alone in its column
    Case("count3841", 1024, 32, 3841, TWO, cls="dups"),        # four sample blocks, the last with 769 of 1024
    Case("count3841_wrap", 1024, 32, 3841, TWO, wrap=True, ndata=5000),
    Case("rows64_c257", 64, 32, 257, TWO, cls="dups"),         # one group
    Case("rows65_c255", 65, 32, 255, TWO, cls="dups"),         # ragged last group
    Case("rows1088_c1025", 1088, 32, 1025, TWO, cls="dups"),   # 17 groups: a chunk's second trip of one group; 2 blocks
    Case("som64x64_c3999", 4096, 64, 3999, RING, som=(64, 64, TOPOL_HEXA), cls="dups"),
    Case("same448_c255", 448, 32, 255, TWO, cls="same"),       # every group listed for every sample
    Case("same576_c257", 576, 32, 257, TWO, cls="same"),       # ... and the segments overflow
    Case("zeros_c257", 1024, 32, 257, TWO, cls="zeros"),
    Case("nan_c255", 1024, 32, 255, TWO, cls="nan"),
]


@pytest.fixture(scope="module")
def eng():
    from som_lvq_pak_amd import engine as E
    e = E.Engine(0)
    e.set_scan_mode("mfma_bf16")
    yield e
    e.close()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_select_passes_at_tile_edges(eng, oracle, c):
    RS.test_both_selectors_give_the_replayed_pairs(eng, oracle, c)


def test_level2_lists_hold_each_live_sample_once(eng):
    """l2_pairs of the statistics is the sum of the lists' lengths: with one vector repeated in every row every
    (group, live sample) pair passes level 1's window, so the sum is groups x count exactly -- no dead sample of a
    partly live quad is filed, none twice."""
    from som_lvq_pak_amd import engine as E
    for c in (Case("same448_c255", 448, 32, 255, TWO, cls="same"), Case("same448_c1027", 448, 32, 1027, TWO, cls="same")):
        codes, x, _ = RS.data_of(c)
        cb, ds = E.Codebook(eng, codes), E.Dataset(eng, x)
        try:
            before = eng.scan_stats()["l2_pairs"]
            E.debug_rerank_pairs(cb, ds, c.first, c.count, True)
            assert eng.scan_stats()["l2_pairs"] - before == (c.n // 64) * c.count
        finally:
            cb.close()
            ds.close()
