"""The bounds rule of the segmented passes (rl_paint_segment_range, device_types.h paint_segment_first -- the
function the kernels run): the segments of a step range partition it, every step exactly once and in order, for any
length including 0 and lengths below the number of segments."""
import pytest

from relate_amd import api

LENGTHS = list(range(0, 41)) + [999, 52850, 500000, 2**31 - 2]


@pytest.mark.parametrize("seg", range(1, 18))
def test_segments_partition_the_range_in_order(seg):
    for n in LENGTHS:
        for lo in (0, 1):
            if lo + n > 2**31 - 1:
                continue
            hi = lo + n
            at = lo
            for s in range(seg):
                first, last = api.paint_segment_range(lo, hi, seg, s)
                assert first == at and first <= last <= hi, (n, lo, seg, s, first, last)
                assert last - first in (n // seg, n // seg + 1), (n, lo, seg, s, first, last)
                at = last
            assert at == hi, (n, lo, seg)


def test_one_segment_is_the_whole_range():
    for lo, hi in ((0, 0), (1, 1), (1, 2), (1, 53000), (0, 2**31 - 1), (7, 3)):
        assert api.paint_segment_range(lo, hi, 1, 0) == (lo, max(lo, hi))


def test_an_inverted_range_is_empty_in_every_segment():
    for s in range(5):
        assert api.paint_segment_range(1, 0, 5, s) == (1, 1)


def test_bad_segment_index_is_refused():
    for seg, s in ((0, 0), (3, 3), (3, -1), (-2, 0)):
        with pytest.raises(api.RelateError) as e:
            api.paint_segment_range(0, 10, seg, s)
        assert "error -1" in str(e.value)  # RL_EINVAL
