"""The definition of dflow_flow_consistency (tests/consistency_ref.py) pinned by hand (CPU only): what the classes are, where
the nearest and the bilinear lookup draw their lines, and what sets the check apart from the reference's transposed one."""
import numpy as np
import pytest

import consistency_ref as R

F = np.float32
NAN, INF = np.nan, np.inf


def uvv(h, w, u=0.0, v=0.0, valid=1.0):
    f = np.zeros((h, w, 3), np.float32)
    f[..., 0], f[..., 1], f[..., 2] = u, v, valid
    return f


def dydx(h, w, dy=0.0, dx=0.0):
    f = np.zeros((h, w, 2), np.float32)
    f[..., 0], f[..., 1] = dy, dx
    return f


def cls_of(fwd, bwd, y, x, thresh=1.0, flags=0):
    return R.classify(np.asarray(fwd, np.float32), np.asarray(bwd, np.float32), y, x, F(thresh), flags)[0]


def test_q13_discriminator(oracle):
    """6x9, forward (0,+3) everywhere, backward (0,-3): the natural check keeps the 6x6 pixels whose target is inside and calls
    the last 3 COLUMNS outside; the reference's check on the same fields kills the last 3 ROWS."""
    fwd, bwd = dydx(6, 9, 0, 3), dydx(6, 9, 0, -3)
    for flags in (0, R.BILINEAR):
        out, err, counts, cls = R.one_direction(fwd, bwd, 10, flags)
        assert out[:, :6, 2].all() and not out[:, 6:, 2].any()
        assert (cls[:, :6] == R.CONSISTENT).all() and (cls[:, 6:] == R.OUTSIDE).all()
        assert counts == [36, 0, 0, 18, 0]
        assert (out[:, :6, 0] == 3).all() and (out[:, :6, 1] == 0).all() and (out[:, 6:] == 0).all()
        assert (err[:, :6] == 0).all() and (err[:, 6:] == -1).all()
    s = oracle.fb_consistency(fwd.astype(np.float64), bwd.astype(np.float64), 10)
    assert s[:3, :, 2].all() and not s[3:, :, 2].any()


def test_err_equal_to_thresh_is_consistent():
    fwd, bwd = uvv(4, 5), uvv(4, 5)
    fwd[0, 0, :2] = (3, 0)                       # U = 3: the target is (0,3)
    bwd[0, 3, :2] = (0, 4)                       # du = 3, dv = 4: err = 5
    for flags in (0, R.BILINEAR):
        k, e = R.classify(fwd, bwd, 0, 0, F(5), flags)
        assert k == R.CONSISTENT and e == F(5)
        k, e = R.classify(fwd, bwd, 0, 0, F(np.nextafter(F(5), F(0))), flags)
        assert k == R.ABOVE and e == F(5)
    out, err, counts, _ = R.one_direction(fwd, bwd, 5)
    assert out[0, 0].tolist() == [3, 0, 1] and err[0, 0] == 5 and counts == [20, 0, 0, 0, 0]


@pytest.mark.parametrize("v,target", [(0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (0.49999997, 0), (0.50000006, 1)])
def test_nearest_rounds_ties_to_even(v, target):
    h = w = 7
    fwd, bwd = uvv(h, w, valid=0), uvv(h, w, valid=0)
    for axis in (0, 1):
        fwd[...] = 0
        bwd[...] = 0
        fwd[3, 3, axis], fwd[3, 3, 2] = v, 1                           # axis 0: U moves the column; axis 1: V moves the row
        t = (3, 3 + target) if axis == 0 else (3 + target, 3)
        assert cls_of(fwd, bwd, 3, 3) == R.BWD_INVALID                 # every backward pixel is invalid ...
        bwd[t[0], t[1], 2] = 1                                         # ... but the one the rounded vector points at
        bwd[t[0], t[1], axis] = -v
        assert cls_of(fwd, bwd, 3, 3) == R.CONSISTENT


def test_nearest_range_of_a_rounded_component():
    fwd, bwd = uvv(1, 1), uvv(1, 1)
    for v, want in ((32767.4, R.OUTSIDE), (32767.5, R.OUTSIDE), (-32767.5, R.OUTSIDE), (-32768.0, R.OUTSIDE), (3e38, R.OUTSIDE)):
        fwd[0, 0, 0] = v
        assert cls_of(fwd, bwd, 0, 0) == want                          # 32767.4 is in range but leaves a 1x1 frame
    # in range and inside: x + rx within a frame 8192 wide can only be reached by small vectors, so the range rule itself never
    # decides for a legal frame; what it guarantees is that the integer sum cannot overflow
    assert int(np.rint(F(32767.4))) == 32767 and int(np.rint(F(32767.5))) == 32768


def test_nearest_targets_on_the_frame():
    h, w = 4, 5
    bwd = uvv(h, w)
    for y, x, v, u, want in ((0, 0, -1, 0, R.OUTSIDE), (0, 0, 0, -1, R.OUTSIDE), (0, 0, 0, 0, R.CONSISTENT),
                             (0, 0, h - 1, w - 1, R.ABOVE), (0, 0, h, 0, R.OUTSIDE), (0, 0, 0, w, R.OUTSIDE),
                             (3, 4, -3, -4, R.ABOVE), (3, 4, -4, 0, R.OUTSIDE), (3, 4, 0.4, 0.4, R.CONSISTENT), (3, 4, 0.6, 0, R.OUTSIDE)):
        fwd = uvv(h, w)
        fwd[y, x, :2] = (u, v)
        assert cls_of(fwd, bwd, y, x) == want, (y, x, v, u)


def test_bilinear_at_the_frame():
    h, w = 4, 5
    bwd = uvv(h, w)
    top = np.nextafter(F(h - 1), F(INF))
    for y, v, want in ((0, -0.0, R.CONSISTENT), (0, -1e-30, R.OUTSIDE), (1, -1.0, R.ABOVE), (0, h - 1, R.ABOVE),
                       (0, top, R.OUTSIDE), (h - 1, 0.0, R.CONSISTENT), (h - 1, 1e-3, R.OUTSIDE), (1, 1.5, R.ABOVE), (1, 2.0, R.ABOVE)):
        fwd = uvv(h, w)
        fwd[y, 2, 1] = v
        assert cls_of(fwd, bwd, y, 2, thresh=0.5, flags=R.BILINEAR) == want, (y, v)
    for x, u, want in ((0, -0.0, R.CONSISTENT), (0, w - 1, R.ABOVE), (0, np.nextafter(F(w - 1), F(INF)), R.OUTSIDE),
                       (w - 1, 0.0, R.CONSISTENT), (w - 1, 1e-3, R.OUTSIDE), (0, -1e-30, R.OUTSIDE)):
        fwd = uvv(h, w)
        fwd[1, x, 0] = u
        assert cls_of(fwd, bwd, 1, x, thresh=0.5, flags=R.BILINEAR) == want, (x, u)
    # (float)y + V rounds: at y = 3 a V of -1e-30 is absorbed and the target is row 3 itself
    fwd = uvv(h, w)
    fwd[3, 2, 1] = -1e-30
    assert cls_of(fwd, bwd, 3, 2, flags=R.BILINEAR) == R.CONSISTENT


def test_bilinear_corners_and_weights():
    h, w = 5, 6
    fwd, bwd = uvv(h, w), uvv(h, w)
    bwd[2, 3, 2] = 0                                                   # one invalid backward pixel
    # an integer target next to it: its row / column neighbours have weight zero and are not looked at
    for y, x, v, u in ((1, 3, 0, 0), (2, 2, 0, 0), (0, 0, 1, 3), (3, 3, 0, 0), (2, 4, 0, 0), (0, 0, 3, 3)):
        fwd[...] = uvv(h, w)
        fwd[y, x, :2] = (u, v)
        assert cls_of(fwd, bwd, y, x, thresh=10, flags=R.BILINEAR) == R.CONSISTENT, (y, x)
    fwd[...] = uvv(h, w)
    assert cls_of(fwd, bwd, 2, 3, flags=R.BILINEAR) == R.BWD_INVALID   # the target itself
    # a positive weight, however small, makes the corner count: each of the four positions around it
    for y, x, v, u in ((1, 3, 0.001, 0), (2, 2, 0, 0.001), (1, 2, 0.5, 0.5), (2, 3, 0.25, 0.25), (2, 3, -0.25, -0.25), (3, 4, -0.999, -0.999)):
        fwd[...] = uvv(h, w)
        fwd[y, x, :2] = (u, v)
        assert cls_of(fwd, bwd, y, x, flags=R.BILINEAR) == R.BWD_INVALID, (y, x, v, u)
        assert cls_of(fwd, bwd, y, x, thresh=2, flags=0) == (R.BWD_INVALID if (y + round(v), x + round(u)) == (2, 3) else R.CONSISTENT)
    # the interpolated value, in the written order
    bwd = uvv(h, w)
    bwd[1, 1, :2], bwd[1, 2, :2], bwd[2, 1, :2], bwd[2, 2, :2] = (1, 10), (2, 20), (3, 30), (5, 50)
    fwd = uvv(h, w)
    fwd[1, 1, :2] = (0.25, 0.5)                                        # ax = 0.25, ay = 0.5
    k, e = R.classify(fwd, bwd, 1, 1, F(100), R.BILINEAR)
    bu = F(1.25) + F(0.5) * (F(3.5) - F(1.25))
    bv = F(12.5) + F(0.5) * (F(35) - F(12.5))
    assert k == R.CONSISTENT and e == np.sqrt(F((F(0.25) + bu) ** 2 + (F(0.5) + bv) ** 2))


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_vectors_that_are_not_finite(bad):
    h, w = 3, 4
    for layout in (uvv, dydx):
        for comp in (0, 1):
            for flags in (0, R.BILINEAR):
                fwd, bwd = layout(h, w), layout(h, w)
                fwd[1, 1, comp] = bad
                assert cls_of(fwd, bwd, 1, 1, flags=flags) == R.FWD_INVALID
                assert cls_of(bwd, fwd, 1, 1, flags=flags) == R.BWD_INVALID
    f = uvv(h, w)
    f[1, 1, 2] = bad                                                   # valid: NaN and -inf compare false, +inf is > 0.5
    assert cls_of(f, uvv(h, w), 1, 1) == (R.CONSISTENT if bad == INF else R.FWD_INVALID)


def test_large_components_overflow_into_above():
    h, w = 3, 4
    fwd, bwd = uvv(h, w), uvv(h, w)
    bwd[..., 0] = 3e38
    fwd[1, 1, 0] = 3e38                                                # finite, but it leaves the frame
    for flags in (0, R.BILINEAR):
        assert cls_of(fwd, bwd, 1, 1, flags=flags) == R.OUTSIDE
        k, e = R.classify(fwd, bwd, 0, 0, F(3e38), flags)              # U = 0 + 3e38: du*du overflows, err = inf is above
        assert k == R.ABOVE and np.isinf(e)
    out, err, counts, _ = R.one_direction(fwd, bwd, 3e38)
    assert counts == [0, 11, 0, 1, 0] and not out.any() and np.isinf(err).sum() == 11 and err[1, 1] == -1
    # two large corners whose difference overflows: a NaN or infinite err is above
    bwd = uvv(h, w)
    bwd[0, 0, 0], bwd[0, 1, 0] = 3e38, -3e38
    fwd = uvv(h, w)
    fwd[0, 0, 0] = 0.5
    k, e = R.classify(fwd, bwd, 0, 0, F(3e38), R.BILINEAR)
    assert k == R.ABOVE and not np.isfinite(e)


def random_fields(h, w, seed, integer, p_invalid=0.3, amp=3.0):
    """A forward field in [U,V,valid] and a backward one that mostly undoes it, with noise; 30 % invalid pixels in either."""
    rng = np.random.default_rng(seed)
    f = np.zeros((2, h, w, 3), np.float32)
    f[0, ..., :2] = rng.normal(0, amp, (h, w, 2))
    f[1, ..., :2] = -f[0, ..., :2] + rng.normal(0, 1.0, (h, w, 2))
    if integer:
        f[..., :2] = np.rint(f[..., :2])
    f[..., 2] = rng.random((2, h, w)) >= p_invalid
    return f[0], f[1]


def test_bilinear_equals_nearest_on_an_integer_field():
    fwd, bwd = random_fields(9, 11, 5, integer=True)
    fwd[0, 0, :2], fwd[8, 10, :2] = (-0.0, -0.0), (-0.0, 0.0)
    a = R.flow_consistency(fwd, bwd, 1.5, 0, both=True)
    b = R.flow_consistency(fwd, bwd, 1.5, R.BILINEAR, both=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a[4] == b[4] and min(a[4][:4]) > 0, a[4]
    fr, br = random_fields(9, 11, 5, integer=False)
    assert R.flow_consistency(fr, br, 1.5, 0)[2] != R.flow_consistency(fr, br, 1.5, R.BILINEAR)[2], "fractional fields do differ"


@pytest.mark.parametrize("flags", [0, R.BILINEAR])
@pytest.mark.parametrize("integer", [True, False])
def test_counts_add_up_and_both_equals_two_single_calls(flags, integer):
    h, w = 8, 13
    fwd, bwd = random_fields(h, w, 9, integer)
    bwd = np.ascontiguousarray(bwd[..., 1::-1])                        # the backward field as [dy,dx]: every pixel valid
    of, ob, ef, eb, counts = R.flow_consistency(fwd, bwd, 2.0, flags, both=True)
    assert sum(counts[:5]) == h * w and sum(counts[5:]) == h * w
    assert counts[4] > 0 and counts[9] == 0 and counts[2] == 0 and counts[7] > 0      # [dy,dx] has no invalid pixel
    one = R.flow_consistency(fwd, bwd, 2.0, flags)
    two = R.flow_consistency(bwd, fwd, 2.0, flags)
    assert np.array_equal(of.view(np.uint32), one[0].view(np.uint32)) and np.array_equal(ef.view(np.uint32), one[1].view(np.uint32))
    assert np.array_equal(ob.view(np.uint32), two[0].view(np.uint32)) and np.array_equal(eb.view(np.uint32), two[1].view(np.uint32))
    assert counts == one[2] + two[2]
    # the output carries the forward vector's own bits, as [U,V,1], and the count of valid outputs is the first count
    keep = of[..., 2] == 1
    assert keep.sum() == counts[0] and np.array_equal(of[keep][:, :2].view(np.uint32), fwd[keep][:, :2].view(np.uint32))
    assert np.array_equal(ob[ob[..., 2] == 1][:, :2], bwd[ob[..., 2] == 1][:, ::-1])
    assert ((ef >= 0) | np.isnan(ef)).sum() == counts[0] + counts[1] and (ef[~keep & (ef >= 0)] > 2.0).all()


def test_nearest_on_integer_fields_is_the_reference_check_untransposed(oracle):
    """On integer [dy,dx] fields the reference's check differs only in where it looks: fed the transposed fields it gives the
    transposed answer.  Square frame, so that its bounds test is the same one."""
    n = 12
    rng = np.random.default_rng(3)
    fwd = np.rint(rng.normal(0, 2.5, (n, n, 2))).astype(np.float32)
    bwd = (-fwd + np.rint(rng.normal(0, 1.2, (n, n, 2)))).astype(np.float32)
    out = R.one_direction(fwd, bwd, 2)[0]
    t = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)).astype(np.float64)
    s = oracle.fb_consistency(t(fwd), t(bwd), 2)
    got = s.transpose(1, 0, 2)
    assert 0 < out[..., 2].sum() < n * n
    assert np.array_equal(got, out)
