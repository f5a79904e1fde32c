"""CPU: `ops._flat_layout`, the one walk over the flat parameter buffer from which both fused optimiser steps build their
range tables -- on integers, no device.  Units: inputs in floats, ranges in FOUR floats (16-byte rows)."""
import pytest

from robot_aware_control_amd import ops


def tiles_once(ranges, total):
    """The ranges are non-empty, in order, and cover [0, total) exactly once."""
    pos = 0
    for b4, n4, _ in ranges:
        assert n4 > 0 and 4 * b4 == pos, ranges
        pos += 4 * n4
    assert pos == total, ranges
    return True


def test_gaps_and_weights_tile_the_buffer():
    spans = [(8, 400), (428, 1600), (2040, 36)]  # gaps of 8, 20, 12 and a tail of 24 floats
    total = 2100
    ranges = ops._flat_layout(total, spans)
    assert tiles_once(ranges, total)
    assert [(4 * b4, 4 * n4) for b4, n4, i in ranges if i is not None] == spans
    assert [i for _, _, i in ranges] == [None, 0, None, 1, None, 2, None]
    assert [(4 * b4, 4 * n4) for b4, n4, i in ranges if i is None] == [(0, 8), (408, 20), (2028, 12), (2076, 24)]


def test_adjacent_weights_have_no_empty_gap_between_them():
    ranges = ops._flat_layout(64, [(4, 16), (20, 32)])
    assert ranges == [(0, 1, None), (1, 4, 0), (5, 8, 1), (13, 3, None)] and tiles_once(ranges, 64)
    ranges = ops._flat_layout(48, [(0, 16), (16, 32)])  # ... nor in front of a weight at element 0
    assert ranges == [(0, 4, 0), (4, 8, 1)]


def test_a_weight_ending_at_the_end_has_no_tail_range():
    ranges = ops._flat_layout(60, [(8, 12), (28, 32)])
    assert ranges == [(0, 2, None), (2, 3, 0), (5, 2, None), (7, 8, 1)] and tiles_once(ranges, 60)


def test_no_weights_is_one_gap():
    assert ops._flat_layout(40, []) == [(0, 10, None)]


@pytest.mark.parametrize("total,spans", [
    (4096, [(0, 2048), (0, 1024), (1024, 1024)]),  # the merged head next to its own two halves (flat order: by offset)
    (4096, [(0, 1024), (512, 1024)]),              # a plain overlap
    (4096, [(6, 1024)]),                           # an offset that is not whole 16-byte rows
    (4096, [(8, 1022)]),                           # a size that is not
    (4098, [(8, 1024)]),                           # a buffer that is not
    (4096, [(3584, 1024)]),                        # a span past the end
    (4096, [(4096, 4)]),
])
def test_layouts_the_tables_do_not_describe(total, spans):
    assert ops._flat_layout(total, spans) is None
