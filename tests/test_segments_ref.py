"""tests/segments_ref.py, the numpy definition of dflow_segment_filter, on hand-made fields whose results are written out by hand,
and on the committed sparse fields (CPU only).  The device is compared with this reference in tests/test_gpu_segments.py."""
import numpy as np
import pytest

import segments_ref as R
from segments_ref import golden_fields, uvv

NAN, INF = float("nan"), float("inf")


def test_three_by_three():
    # U:  0 0 5      segments: {0,1,3} id 0; {2,5} id 2; {4} id 4; {6,7,8} id 6
    #     0 9 5
    #     3 3 3
    f = uvv([[0, 0, 5], [0, 9, 5], [3, 3, 3]])
    out, seg, size, counts = R.segment_filter(f, 1, 3)
    assert seg.tolist() == [[0, 0, 2], [0, 4, 2], [6, 6, 6]]
    assert size.tolist() == [[3, 3, 2], [3, 1, 2], [3, 3, 3]]
    assert counts == [4, 2, 9, 3]
    assert out[..., 2].tolist() == [[1, 1, 0], [1, 0, 0], [1, 1, 1]]
    assert out[..., 0].tolist() == [[0, 0, 0], [0, 0, 0], [3, 3, 3]]
    # the singleton stays with the flag; the pair does not
    out, seg2, size2, counts = R.segment_filter(f, 1, 3, R.KEEP_SINGLETONS)
    assert out[..., 2].tolist() == [[1, 1, 0], [1, 1, 0], [1, 1, 1]] and out[1, 1].tolist() == [9, 0, 1]
    assert counts == [4, 1, 9, 2] and np.array_equal(seg, seg2) and np.array_equal(size, size2)
    # thresh 2: 5 and 3 join, so {2,5,6,7,8} becomes one segment with id 2; 0 and 3 differ by 3
    _, seg, size, counts = R.segment_filter(f, 2, 3)
    assert seg.tolist() == [[0, 0, 2], [0, 4, 2], [2, 2, 2]] and size[2].tolist() == [5, 5, 5] and counts == [3, 1, 9, 1]


def test_one_by_five_and_the_join_is_the_sum_of_both_components():
    f = uvv([[1, 2, 3, 7, 8]], [[0, 0, 1, 0, 0]])      # 2 -> 3 costs |1| + |1| = 2
    out, seg, size, counts = R.segment_filter(f, 1, 2)
    assert seg.tolist() == [[0, 0, 2, 3, 3]] and size.tolist() == [[2, 2, 1, 2, 2]] and counts == [3, 1, 5, 1]
    assert out[0].tolist() == [[1, 0, 1], [2, 0, 1], [0, 0, 0], [7, 0, 1], [8, 0, 1]]
    _, seg, size, _ = R.segment_filter(f, 2, 2)
    assert seg.tolist() == [[0, 0, 0, 3, 3]] and size.tolist() == [[3, 3, 3, 2, 2]]
    # a column is the same
    _, seg, _, _ = R.segment_filter(np.ascontiguousarray(f.transpose(1, 0, 2)), 1, 2)
    assert seg.ravel().tolist() == [0, 0, 2, 3, 3]


def test_threshold_is_inclusive_to_the_ulp():
    t = np.float32(0.7)
    up = np.nextafter(t, np.float32(1))
    for a, b, joins in ((t, 0, True), (up, 0, False), (0, t, True), (0, up, False)):
        f = uvv([[0, a]], [[0, b]])
        assert (R.segment_filter(f, t, 0)[3][0] == 1) == joins, (a, b)
        assert (R.segment_filter(f[:, ::-1].copy(), t, 0)[3][0] == 1) == joins, "symmetric"
    # the sum is rounded once: 0.5 + 2^-25 is 0.5 in float32, so two halves' worth joins at thresh 0.5
    f = uvv([[0, 0.5]], [[0, 2.0 ** -25]])
    assert R.segment_filter(f, 0.5, 0)[3][0] == 1
    # thresh 0 joins equal vectors only, and -0.0 equals 0.0
    assert R.segment_filter(uvv([[0.0, -0.0, 1e-45]]), 0, 0)[1].tolist() == [[0, 0, 2]]
    # a difference that overflows does not join, whatever thresh is
    big = uvv([[3e38, -3e38]])
    assert R.segment_filter(big, 3.4e38, 0)[3][0] == 2


def test_min_size_boundaries():
    f = uvv([[1, 1, 1, 1, 9, 5, 5]])                    # sizes 4, 1, 2
    for min_size, kept in ((0, 7), (1, 7), (2, 6), (3, 4), (4, 4), (5, 0), (2 ** 31 - 1, 0)):
        out, _, size, counts = R.segment_filter(f, 0, min_size)
        assert int(out[..., 2].sum()) == kept and counts[2] == 7 and counts[3] == 7 - kept, min_size
        assert size.tolist() == [[4, 4, 4, 4, 1, 2, 2]], "sizes describe the input"
    for min_size, kept in ((0, 7), (2, 7), (3, 5), (5, 1), (2 ** 31 - 1, 1)):
        out, _, _, counts = R.segment_filter(f, 0, min_size, R.KEEP_SINGLETONS)
        assert int(out[..., 2].sum()) == kept and counts[3] == 7 - kept, min_size
        if min_size >= 5:
            assert out[0, 4].tolist() == [9, 0, 1]


def test_non_members():
    f = uvv([[1, 1, 1, 1, 1, 1, 1]])
    f[0, 1, 0] = NAN
    f[0, 3, 1] = INF
    f[0, 5, 2] = 0.5                                    # valid must be above 0.5
    out, seg, size, counts = R.segment_filter(f, 10, 0)
    assert seg.tolist() == [[0, -1, 2, -1, 4, -1, 6]] and size.tolist() == [[1, 0, 1, 0, 1, 0, 1]] and counts == [4, 0, 4, 0]
    assert out[0, 1].tolist() == [0, 0, 0] and out[0, 3].tolist() == [0, 0, 0] and out[0, 5].tolist() == [0, 0, 0]
    f[0, 5, 2] = NAN
    assert R.segment_filter(f, 10, 0)[3] == [4, 0, 4, 0]
    f[0, 5, 2] = np.nextafter(np.float32(0.5), np.float32(1))
    assert R.segment_filter(f, 10, 0)[1].tolist() == [[0, -1, 2, -1, 4, 4, 4]]
    # [dy,dx] has no valid plane: every finite vector is a member, and U is the second component
    d = np.zeros((1, 4, 2), np.float32)
    d[0, :, 1] = [0, 1, 5, NAN]
    out, seg, _, counts = R.segment_filter(d, 1, 0)
    assert seg.tolist() == [[0, 0, 2, -1]] and counts == [2, 0, 3, 0]
    assert out[0].tolist() == [[0, 0, 1], [1, 0, 1], [5, 0, 1], [0, 0, 0]]


def test_both_layouts_agree():
    rng = np.random.default_rng(5)
    f = uvv(rng.integers(-2, 3, (9, 11)), rng.integers(-2, 3, (9, 11)))
    want = R.segment_filter(f, 1, 4)
    got = R.segment_filter(np.ascontiguousarray(f[..., 1::-1]), 1, 4)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,field,thresh,min_size", golden_fields(), ids=[g[0].replace(" ", "-") for g in golden_fields()])
def test_golden_fields(name, field, thresh, min_size):
    out, seg, size, counts = R.segment_filter(field, thresh, min_size)
    assert 0 < counts[1] < counts[0], "segments are both removed and kept"
    if name == "a40x48_c5x6 sparse_t1":
        assert counts == [26, 21, 1318, 69]
    _, _, mem = R.members(field)
    # counts add up
    assert counts[2] == int(mem.sum()) == int((seg >= 0).sum()) and counts[0] == len(np.unique(seg[seg >= 0]))
    assert counts[3] == counts[2] - int(out[..., 2].sum())
    roots = seg.ravel() == np.arange(seg.size)
    assert counts[0] == int(roots.sum()) and int(size.ravel()[roots].sum()) == counts[2]
    assert counts[1] == int((size.ravel()[roots] < min_size).sum())
    # an id is the smallest raster index of its segment and the size its pixel count
    for sid in np.unique(seg[seg >= 0]):
        idx = np.flatnonzero(seg.ravel() == sid)
        assert idx[0] == sid and (size.ravel()[idx] == len(idx)).all()
    # kept pixels carry their own bits, everything else is zero
    kept = out[..., 2] == 1
    assert np.array_equal(out[kept].view(np.uint32)[:, :2], field[kept].view(np.uint32)[:, :2]) and not out[~kept].any()
    assert np.array_equal(kept, mem & (size >= min_size))
    # idempotence: removing segments joins no others
    again = R.segment_filter(out, thresh, min_size)
    assert np.array_equal(again[0].view(np.uint32), out.view(np.uint32)) and again[3][1] == 0 and again[3][3] == 0
    assert again[3][0] == counts[0] - counts[1]
