"""the within-class nearest later row (mindist / stddev) at exact multiples of its blocks, at class borders on block
borders, at the farthest pair of a class, and masked over several register tiles and component chunks.

The reference is classdist_replay.nearest_later (pinned against the recorded reference runs by tests/test_classdist.py);
_check of that module compares states, and min_sq by bit pattern.  The shapes are chosen against these constants of
kernels/class_nearest.hpp and host_class.inc, read from the source by test_the_constants_are_what_the_shapes_assume:

    WAVE = 64, CLASS_ROWS = 256   positions per row group and per workgroup: n = 64, 128, 256, 512 leave no padding row, and
                                  r_last is the workgroup's own last position
    CLASS_CHUNK = 256             later positions per workgroup, counted from the block's first position; a workgroup
                                  returns at once when its chunk starts at or past seg_end[r_last]: classes that end on,
                                  one before and one after a block border
    chunks = (CLASS_ROWS - 1 + largest + CLASS_CHUNK - 1) / CLASS_CHUNK
                                  what the grid must cover: the first row of a class at position 255 of its block and its
                                  only near neighbour at the far end of the class -- grid row (255 + 257) / 256 = 2 of 3
    CLASS_S = 32, CLASS_S_MASKED = 16   later positions per register tile: classes of 16, 17, 100 and 167 rows start and end
                                  on, and off, both tile sizes
    d4 = (d + 3) / 4              float4 chunks of a row: dimensions 1, 4, 8, 9 and 130 are d4 = 1, 1, 2, 3 and 33"""
import functools
import os
import re

import numpy as np
import pytest

import classdist_replay as R
import test_classdist as TC
from test_classdist import _check, _labels, eng  # noqa: F401  (eng: the module's engine fixture)

WAVE, CLASS_ROWS, CLASS_CHUNK, CLASS_S, CLASS_S_MASKED = 64, 256, 256, 32, 16


def grid_chunks(largest):
    return (CLASS_ROWS - 1 + largest + CLASS_CHUNK - 1) // CLASS_CHUNK


def plain_rows(n, dim, seed):
    return (3.0 * np.random.RandomState(seed).standard_normal((n, dim))).astype(np.float32)


# ------------------------------------------------------------------ the cases
BORDERS = [(256, 256), (255, 257), (257, 255), (512, 1), (256, 1, 1, 254)]
FARTHEST = [(255, 258), (200, 769, 331)]             # class sizes; the equal pair sits at the ends of the second class


@functools.lru_cache(maxsize=None)
def farthest_case(sizes):
    """rows, labels, position of the planted row.  The second class: its first and last rows are equal and near the
    origin, its other rows lie 1000 away, so the first row's minimum is +0, through the pair at the class's full length"""
    n = sum(sizes)
    labels = _labels(sizes, False, None)
    rows = plain_rows(n, 3, 7 * n)
    first, last = sizes[0], sizes[0] + sizes[1] - 1
    rows[first + 1:last] += np.float32(1000.0)
    rows[last] = rows[first]
    rows.setflags(write=False)
    return rows, labels, first, last


MASK_SIZES = (16, 17, 100, 167)
MASK_DIMS = [1, 4, 8, 9, 130]
# the share of masked components.  About 30 %, except where that leaves too few rows of state 1: a pair shares no
# component with probability (1 - (1 - rate)^2)^dim, at 30 % that is 0.51 (dim 1) and 0.068 (dim 4) per later row, and a
# row has up to 166 later rows.  2 % and 10 % make it 0.04 and 0.0013.
MASK_RATE = {1: 0.02, 4: 0.1, 8: 0.3, 9: 0.3, 130: 0.3}
FULLY_MASKED_MEMBER = 40                             # which row of the class of 100 has every component masked


@functools.lru_cache(maxsize=None)
def masked_case(dim, interleave):
    """rows, labels, mask, the fully masked row, the planted pair (or None)"""
    n = sum(MASK_SIZES)
    rs = np.random.RandomState(1000 * dim + interleave)
    labels = _labels(MASK_SIZES, interleave, rs)
    rows = (3.0 * rs.standard_normal((n, dim))).astype(np.float32)
    mask = (rs.uniform(size=(n, dim)) < MASK_RATE[dim]).astype(np.uint8)
    hundred = np.nonzero(labels == 3)[0]
    full = hundred[FULLY_MASKED_MEMBER]
    mask[full] = 1
    pair = None
    if dim >= 4:                                     # disjoint unmasked components; at dim 130 across the 33 chunks
        big = np.nonzero(labels == 4)[0]
        a, b = big[2], big[len(big) - 2]
        mask[a], mask[b] = 0, 1
        mask[a, dim // 2:] = 1
        mask[b, dim // 2:] = 0
        pair = (a, b)
    for arr in (rows, labels, mask):
        arr.setflags(write=False)
    return rows, labels, mask, full, pair


def check_masked_case(dim, interleave, state):
    """what the case promises, from the replay's states"""
    rows, labels, mask, full, pair = masked_case(dim, interleave)
    hundred = np.nonzero(labels == 3)[0]
    assert (state[hundred[:FULLY_MASKED_MEMBER]] == 2).all() and state[full] == 2       # (the row has 59 later ones)
    if pair is not None:
        assert state[pair[0]] == 2 and not (mask[pair[0]] == 0)[mask[pair[1]] == 0].any()
    assert (state == 1).sum() >= 30 and (state == 2).sum() >= 10
    assert (state == 0).sum() == len(MASK_SIZES)


# ------------------------------------------------------------------ without a GPU
def test_the_constants_are_what_the_shapes_assume():
    src = os.path.join(TC.ROOT, "som_lvq_pak_amd", "csrc")
    kern = open(os.path.join(src, "kernels", "class_nearest.hpp")).read()
    assert int(re.search(r"constexpr int CLASS_ROWS = (\d+);", kern).group(1)) == CLASS_ROWS
    assert int(re.search(r"constexpr int CLASS_CHUNK = (\d+);", kern).group(1)) == CLASS_CHUNK
    assert re.search(r"if \(cs >= seg_end\[r_last\]\) return;", kern)
    host = open(os.path.join(src, "host_class.inc")).read()
    assert int(re.search(r"constexpr int CLASS_S = (\d+);", host).group(1)) == CLASS_S
    assert int(re.search(r"constexpr int CLASS_S_MASKED = (\d+);", host).group(1)) == CLASS_S_MASKED
    assert re.search(r"const int64_t chunks = \(CLASS_ROWS - 1 \+ o\.largest \+ CLASS_CHUNK - 1\) / CLASS_CHUNK;", host)
    assert re.search(r"constexpr int WAVE = (\d+);", open(os.path.join(src, "kernels", "common.hpp")).read()).group(1) == str(WAVE)


@pytest.mark.parametrize("sizes", FARTHEST, ids=["x".join(map(str, s)) for s in FARTHEST])
def test_the_farthest_pair_decides(sizes):
    """the planted row's minimum is +0 through its class's last row alone, and that pair needs the grid's last row"""
    rows, labels, first, last = farthest_case(sizes)
    min_sq, state = R.nearest_later(rows, labels)
    assert state[first] == 1 and min_sq[first:first + 1].view(np.uint32)[0] == 0
    keep = np.arange(len(labels)) != last
    short_sq, short_state = R.nearest_later(rows[keep], labels[keep])
    assert short_state[first] == 1 and short_sq[first] > 1e5
    block = first // CLASS_ROWS * CLASS_ROWS
    assert (last - block) // CLASS_CHUNK == grid_chunks(max(sizes)) - 1      # one chunk fewer would lose the pair
    if sizes == (255, 258):
        assert first % CLASS_ROWS == CLASS_ROWS - 1 and (last - block) // CLASS_CHUNK == 2 and grid_chunks(258) == 3


@pytest.mark.parametrize("interleave", [False, True], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("dim", MASK_DIMS)
def test_the_masked_cases_are_not_vacuous(dim, interleave):
    rows, labels, mask, full, pair = masked_case(dim, interleave)
    _, state = R.nearest_later(rows, labels, mask)
    check_masked_case(dim, interleave, state)


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [WAVE, 2 * WAVE, CLASS_ROWS, 2 * CLASS_ROWS])
def test_exact_multiples_of_row_groups_and_blocks(n, eng):
    want_sq, want_state = _check(eng, plain_rows(n, 3, n), _labels((n,), False, None), None)
    assert (want_state[:-1] == 1).all() and want_state[-1] == 0 and np.isfinite(want_sq[:-1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", BORDERS, ids=["x".join(map(str, s)) for s in BORDERS])
def test_classes_that_end_at_block_borders(sizes, eng):
    n = sum(sizes)
    labels = _labels(sizes, False, None)
    _, want_state = _check(eng, plain_rows(n, 3, n + len(sizes)), labels, None)
    ends = np.cumsum(sizes) - 1
    assert (want_state[ends] == 0).all() and (want_state == 0).sum() == len(sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", FARTHEST, ids=["x".join(map(str, s)) for s in FARTHEST])
def test_the_farthest_pair_of_a_class_is_reached(sizes, eng):
    rows, labels, first, _ = farthest_case(sizes)
    want_sq, want_state = _check(eng, rows, labels, None)
    assert want_state[first] == 1 and want_sq[first] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", [False, True], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("dim", MASK_DIMS)
def test_masks_over_tiles_and_component_chunks(dim, interleave, eng):
    """the masked instantiation and, on the same rows and labels, the unmasked one"""
    rows, labels, mask, _, _ = masked_case(dim, interleave)
    _, want_state = _check(eng, rows, labels, mask)
    check_masked_case(dim, interleave, want_state)
    _, plain_state = _check(eng, rows, labels, None)
    assert (plain_state == 2).sum() == 0
