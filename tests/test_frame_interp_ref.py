"""frame_interp_ref.py, the numpy definition of dflow_frame_interp (include/dflow.h), pinned by hand on small cases, and
synth.make_mid with the quality floor of the interpolated frame against the plain blend.  CPU only."""
import numpy as np
import pytest

import frame_interp_ref as R
from conftest import pkg

F = np.float32
FREE = int(R.FREE)


def uvv(h, w, U=0.0, V=0.0, valid=1.0):
    f = np.zeros((h, w, 3), F)
    f[..., 0], f[..., 1], f[..., 2] = U, V, valid
    return f


def grey(h, w, value):
    return np.full((h, w, 3), value, np.uint8)


def key(e, idx):
    return (int(np.array(e, F).view(np.uint32)) << 32) | idx


def test_identical_frames_and_a_zero_flow_give_the_frame_back():
    img = R.images(6, 7, 1)[0]
    for t in (0.5, 0.25):
        for bwd in (None, uvv(6, 7)):
            r = R.frame_interp(img, img, uvv(6, 7), bwd, t=t)
            assert np.array_equal(r["out"], img)
            assert (r["source"] == 1).all() and r["counts"][:4] == [42, 0, 0, 0] and r["counts"][4:7] == [42, 0, 0]
            assert r["counts"][7] == (0 if bwd is None else 42)          # every source of frame 2 lost against frame 1's
            assert np.array_equal(r["keys"], np.arange(42, dtype=np.uint64).reshape(6, 7))


def test_shift_by_four_lands_two_columns_on_and_the_holes_fill_from_inside():
    h, w = 4, 9
    a = np.zeros((h, w, 3), np.uint8)
    a[...] = (np.arange(w) * 20)[None, :, None]
    b = np.roll(a, 4, axis=1)
    fwd = uvv(h, w, U=4.0)
    r0 = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=0)
    # sources x = 0..4 end inside the frame and land on x + 2; columns 0-1 (and 7-8, whose sources leave the frame) get nobody
    assert np.array_equal(r0["source"], np.tile(np.array([0, 0, 1, 1, 1, 1, 1, 0, 0], np.uint8), (h, 1)))
    assert np.array_equal(r0["keys"][:, 2:7] & np.uint64(0xFFFFFFFF), (np.arange(h)[:, None] * w + np.arange(5)[None, :]).astype(np.uint64))
    assert (r0["keys"][:, :2] == R.FREE).all() and (r0["keys"][:, 7:] == R.FREE).all()
    assert np.array_equal(r0["out"][:, 2:7], a[:, 0:5])                    # column x of frame 1 at x + 2
    blend = np.floor(F(0.5) * a.astype(F) + F(0.5) * b.astype(F) + F(0.5)).astype(np.uint8)
    assert np.array_equal(r0["out"][:, :2], blend[:, :2]) and np.array_equal(r0["out"][:, 7:], blend[:, 7:])
    assert r0["counts"] == [20, 0, 0, 16, 20, 0, 16, 0]
    r1 = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=1)
    assert np.array_equal(r1["source"][0], np.array([0, 3, 1, 1, 1, 1, 1, 3, 0], np.uint8))
    r2 = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=2)
    assert np.array_equal(r2["source"][0], np.array([3, 3, 1, 1, 1, 1, 1, 3, 3], np.uint8))
    assert (r2["motion"] == np.array([4, 0, 1], F)).all()
    # a filled pixel of column 1 samples frame 1 at x = -1 (not inside) and frame 2 at x = 3: one-sided, frame 2
    assert np.array_equal(r2["out"][:, 1], b[:, 3]) and np.array_equal(r2["out"][:, 7], a[:, 5])
    assert r2["counts"] == [20, 0, 16, 0, 20, 16, 0, 0]


def two_claimants(e_first, e_second):
    """1 x 7: source 0 (U = +4) and source 4 (U = -4) both land on pixel 2 at t = 0.5, with errors e_first and e_second."""
    a, b = grey(1, 7, 100), grey(1, 7, 100)
    b[0, 4] = 100 + e_first            # source 0 is compared with frame 2 at x = 4
    b[0, 0] = 100 + e_second           # source 4 with frame 2 at x = 0
    fwd = uvv(1, 7, valid=0.0)
    fwd[0, 0] = (4, 0, 1)
    fwd[0, 4] = (-4, 0, 1)
    return a, b, fwd


def test_the_lower_error_wins_and_at_equal_error_the_smaller_index():
    for e0, e4, winner in ((9, 3, 4), (3, 9, 0), (6, 6, 0), (0, 0, 0)):
        a, b, fwd = two_claimants(e0, e4)
        r = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=0)
        assert int(r["keys"][0, 2]) == key(F(min(e0, e4)), winner)         # ((e + e) + e) / 3 = e for these integers
        assert np.array_equal(r["motion"][0, 2], np.array([4 if winner == 0 else -4, 0, 1], F))
        assert r["counts"][0] == 1 and r["counts"][7] == 1
        assert (r["keys"].ravel()[[0, 1, 3, 4, 5, 6]] == R.FREE).all()


def test_at_equal_error_frame_one_beats_frame_two_whatever_the_indices():
    a, b = grey(1, 7, 50), grey(1, 7, 50)
    fwd, bwd = uvv(1, 7, valid=0.0), uvv(1, 7, valid=0.0)
    fwd[0, 6] = (-4, 0, 1)             # source 6 of frame 1 lands on 4
    bwd[0, 2] = (4, 0, 1)              # source 2 of frame 2 lands on 4 too, with the smaller raster index
    r = R.frame_interp(a, b, fwd, bwd, t=0.5, fill_rounds=0)
    assert int(r["keys"][0, 4]) == key(F(0), 6) and r["source"][0, 4] == 1
    assert r["counts"][0] == 1 and r["counts"][1] == 0 and r["counts"][7] == 1
    # alone, the frame-2 source wins with key n + j and carries the negated vector
    r = R.frame_interp(a, b, uvv(1, 7, valid=0.0), bwd, t=0.5, fill_rounds=0)
    assert int(r["keys"][0, 4]) == key(F(0), 7 + 2) and r["source"][0, 4] == 2
    assert np.array_equal(r["motion"][0, 4].view(np.uint32), np.array([-4, -0.0, 1], F).view(np.uint32))
    # the two sources form the same pair of pixels (a[6], b[2]): their errors stay equal whatever the pixels hold
    a[0, 6], b[0, 2] = 61, 50
    r = R.frame_interp(a, b, fwd, bwd, t=0.5, fill_rounds=0)
    assert int(r["keys"][0, 4]) == key(F(11), 6) and r["source"][0, 4] == 1


def test_a_frame_two_source_with_the_lower_error_wins():
    a, b = grey(1, 7, 50), grey(1, 7, 50)
    fwd, bwd = uvv(1, 7, valid=0.0), uvv(1, 7, valid=0.0)
    fwd[0, 0] = (4, 0, 1)              # frame 1's source 0 -> end point 4, lands on 2; compares a[0] with b[4]
    bwd[0, 5] = (-6, 0, 1)             # frame 2's source 5 -> end point -1: no part
    bwd[0, 6] = (-6, 0, 1)             # frame 2's source 6 -> end point 0, place rint(6 - 3) = 3 ... not 2
    bwd[0, 4] = (-4, 0, 1)             # frame 2's source 4 -> end point 0, lands on 2; compares b[4] with a[0]: the same pair
    bwd[0, 3] = (-2, 0, 1)             # frame 2's source 3 -> end point 1, lands on 2; compares b[3] with a[1]
    b[0, 4] = 59                       # the pair (a[0], b[4]) differs by 9, the pair (a[1], b[3]) by 0
    r = R.frame_interp(a, b, fwd, bwd, t=0.5, fill_rounds=0)
    assert int(r["keys"][0, 2]) == key(F(0), 7 + 3) and r["source"][0, 2] == 2
    assert np.array_equal(r["motion"][0, 2], np.array([2, 0, 1], F))
    assert r["counts"][:2] == [0, 2] and r["counts"][7] == 2              # targets 2 and 3 claimed; sources 0 and 4 lost


def test_a_half_way_place_rounds_to_even():
    a = grey(1, 6, 0)
    fwd = uvv(1, 6, U=1.0)
    r = R.frame_interp(a, a, fwd, t=0.5, fill_rounds=0)
    # x + 0.5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4; source 5 leaves the frame
    assert [int(k) for k in r["keys"][0]] == [key(F(0), 0), FREE, key(F(0), 1), FREE, key(F(0), 3), FREE]
    assert r["counts"][0] == 3 and r["counts"][7] == 2


def test_the_fill_takes_up_before_left_before_right_before_down_and_reads_the_previous_round():
    m = np.zeros((3, 3, 3), F)
    m[0, 1], m[1, 0], m[1, 2], m[2, 1] = (1, 1, 1), (2, 2, 1), (3, 3, 1), (4, 4, 1)
    for gone, want in (((), 1), (((0, 1),), 2), (((0, 1), (1, 0)), 3), (((0, 1), (1, 0), (1, 2)), 4)):
        q = m.copy()
        for g in gone:
            q[g] = 0
        assert R.fill_round(q)[1, 1, 0] == want
    row = np.zeros((1, 5, 3), F)
    row[0, 0] = (7, 0, 1)
    one = R.fill_round(row)
    assert one[0, :, 2].tolist() == [1, 1, 0, 0, 0]                       # not the whole row: only what was known before
    assert R.fill_round(one)[0, :, 2].tolist() == [1, 1, 1, 0, 0]
    # through the call: one claimed pixel, k rounds reach Manhattan distance k
    fwd = uvv(5, 5, valid=0.0)
    fwd[2, 2, 2] = 1
    img = grey(5, 5, 9)
    for k in (0, 1, 2, 4):
        r = R.frame_interp(img, img, fwd, t=0.5, fill_rounds=k)
        yy, xx = np.mgrid[0:5, 0:5]
        dist = abs(yy - 2) + abs(xx - 2)
        assert np.array_equal(r["source"], np.where(dist == 0, 1, np.where(dist <= k, 3, 0)).astype(np.uint8))


def test_the_occlusion_switch_by_provenance():
    a, b = grey(3, 3, 10), grey(3, 3, 40)               # every sample pair differs by d = 30
    zero, none = uvv(3, 3), uvv(3, 3, valid=0.0)
    one = none.copy()
    one[1, 1, 2] = 1
    below = float(np.nextafter(F(30), F(0)))
    for t, mixed in ((0.5, 25), (0.25, 18), (0.75, 33)):                   # 0.75*10 + 0.25*40 = 17.5 -> 18; 32.5 -> 33
        r = R.frame_interp(a, b, zero, t=t, occl_thresh=30.0)
        assert (r["out"] == mixed).all() and r["counts"][4:7] == [9, 0, 0]          # d == occl_thresh: blended
        r = R.frame_interp(a, b, zero, t=t, occl_thresh=below)
        assert (r["out"] == 10).all() and r["counts"][4:7] == [0, 9, 0]             # src 1: frame 1
        r = R.frame_interp(a, b, none, zero, t=t, occl_thresh=below)
        assert (r["out"] == 40).all() and (r["source"] == 2).all()                  # src 2: frame 2
        r = R.frame_interp(a, b, one, t=t, occl_thresh=below, fill_rounds=4)
        assert r["source"][1, 1] == 1 and (r["source"] == 3).sum() == 8
        want = np.full((3, 3), 10 if t <= 0.5 else 40)                              # src 3: the frame nearer in time
        want[1, 1] = 10
        assert np.array_equal(r["out"][..., 0], want)


def test_one_sided_at_the_border_and_the_fallback_when_no_side_is_usable():
    a, b = R.images(1, 9, 5)
    fwd = uvv(1, 9, valid=0.0)
    fwd[0, 0] = (2, 0, 1)                               # lands on 1 with motion (2, 0)
    r = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=1, occl_thresh=3e38)
    assert r["source"][0].tolist() == [3, 1, 3, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(r["out"][0, 0], b[0, 1])      # side 1 at x = -1 is outside: frame 2 at x = 1
    blend = np.floor(F(0.5) * a.astype(F) + F(0.5) * b.astype(F) + F(0.5)).astype(np.uint8)
    assert np.array_equal(r["out"][0, 3:], blend[0, 3:])
    assert r["counts"][4:7] == [2, 1, 6]
    # a diagonal motion filled into a corner: side 1 leaves the frame in x, side 2 in y: known, but the fallback
    a, b = R.images(3, 3, 6)
    fwd = uvv(3, 3, valid=0.0)
    fwd[2, 0] = (2, -2, 1)                              # from (x, y) = (0, 2) to (2, 0): lands on (1, 1)
    r = R.frame_interp(a, b, fwd, t=0.5, fill_rounds=2, occl_thresh=3e38)
    assert (r["source"] == np.array([[3, 3, 3], [3, 1, 3], [3, 3, 3]])).all()
    blend = np.floor(F(0.5) * a.astype(F) + F(0.5) * b.astype(F) + F(0.5)).astype(np.uint8)
    assert np.array_equal(r["out"][0, 0], blend[0, 0]) and np.array_equal(r["out"][2, 2], blend[2, 2])   # (-1, 1) and (1, -1)
    assert np.array_equal(r["out"][2, 0], b[1, 1]) and np.array_equal(r["out"][0, 2], a[1, 1])   # the other corners: one side
    assert r["counts"][:4] == [1, 0, 8, 0] and r["counts"][6] >= 2 and sum(r["counts"][4:7]) == 9


def test_the_crafted_border_case_samples_where_it_says():
    """edge_case, the GPU tests' border field: at t = 0.5 its sampling positions include -0.5, the last row / column exactly
    and half a pixel beyond it, forward only and two-sided."""
    a, b, fwd, bwd = R.edge_case()
    h, w = a.shape[:2]
    yi, xi = np.mgrid[0:h, 0:w]
    for back in (None, bwd):
        m = R.frame_interp(a, b, fwd, back, t=0.5, fill_rounds=1, occl_thresh=3e38)["motion"]
        known = m[..., 2] != 0
        ys = np.concatenate([(yi - F(0.5) * m[..., 1])[known], (yi + F(0.5) * m[..., 1])[known]])
        xs = np.concatenate([(xi - F(0.5) * m[..., 0])[known], (xi + F(0.5) * m[..., 0])[known]])
        for v in (-0.5, h - 1, h - 0.5):
            assert (ys == v).any(), v
        for v in (-0.5, w - 1, w - 0.5):
            assert (xs == v).any(), v


def test_vectors_that_are_not_good_take_no_part():
    a, b = R.images(3, 4, 2)
    for layout in (R.UVV, R.DYDX):
        for bad in (np.nan, np.inf, -np.inf):
            for comp in (0, 1):
                f = uvv(3, 4)
                f[1, 2, comp] = bad
                r = R.frame_interp(a, b, R.as_layout(f, layout) if layout == R.UVV else np.ascontiguousarray(f[..., [1, 0]]), t=0.5, fill_rounds=0)
                assert r["source"][1, 2] == 0 and r["counts"][:4] == [11, 0, 0, 1] and r["counts"][7] == 0
    for valid in (0.0, 0.5, np.nan, -1.0):
        f = uvv(3, 4)
        f[0, 0, 2] = valid
        assert R.frame_interp(a, b, f, t=0.5, fill_rounds=0)["source"][0, 0] == 0
    f = uvv(3, 4)
    f[0, 0, 2] = 0.50001
    assert R.frame_interp(a, b, f, t=0.5, fill_rounds=0)["source"][0, 0] == 1


@pytest.mark.parametrize("kind", ["int", "frac", "one", "none"])
def test_the_count_identities_hold(kind):
    h, w = 13, 17
    a, b = R.images(h, w, 3)
    fwd, bwd = R.flow_field(h, w, 10, kind), R.flow_field(h, w, 11, kind)
    for back in (None, bwd):
        for rounds in (0, 3):
            r = R.frame_interp(a, b, fwd, back, t=0.5, fill_rounds=rounds)
            c = r["counts"]
            assert sum(c[:4]) == h * w and sum(c[4:7]) == h * w and min(c) >= 0
            took_part = sum(R.claims(x.astype(F), y.astype(F), f, F(0.5), 0)[2] for x, y, f in ((a, b, fwd), (b, a, back)) if f is not None)
            assert c[0] + c[1] + c[7] == took_part
            assert c[:4] == [int((r["source"] == k).sum()) for k in (1, 2, 3, 0)]
            assert ((r["motion"][..., 2] != 0) == (r["source"] != 0)).all()
    if kind == "one":
        r = R.frame_interp(a, b, fwd, None, t=0.5, fill_rounds=0)
        assert r["counts"][0] == 1 and r["counts"][7] > 50
    if kind == "none":
        r = R.frame_interp(a, b, fwd, bwd, t=0.5, fill_rounds=8)
        assert r["counts"] == [0, 0, 0, h * w, 0, 0, h * w, 0] and (r["keys"] == R.FREE).all()


def test_forward_only_equals_a_backward_field_that_takes_no_part():
    h, w = 9, 12
    a, b = R.images(h, w, 4)
    fwd = R.flow_field(h, w, 12, "frac")
    r0 = R.frame_interp(a, b, fwd, None, t=0.25, fill_rounds=2)
    r1 = R.frame_interp(a, b, fwd, uvv(h, w, valid=0.0), t=0.25, fill_rounds=2)
    for k in ("out", "keys", "source"):
        assert np.array_equal(r0[k], r1[k])
    assert r0["motion"].tobytes() == r1["motion"].tobytes() and r0["counts"] == r1["counts"]
    # both layouts of one field give the same bytes
    r2 = R.frame_interp(a, b, R.as_layout(fwd, R.DYDX), None, t=0.25, fill_rounds=2)
    assert r0["out"].tobytes() == r2["out"].tobytes() and r0["keys"].tobytes() == r2["keys"].tobytes()


# ---------------------------------------------------------------------------------- synth.make_mid and the quality floor
def test_make_mid_ends_in_the_two_frames():
    synth = pkg("synth")
    H, W = 60, 80
    for style in synth.STYLES:
        img1, img2, gt = synth.make_pair(H, W, seed=3, amp_x=12, amp_y=6, noise=0, style=style)
        m0, k0 = synth.make_mid(H, W, seed=3, t=0.0, amp_x=12, amp_y=6, style=style)
        # synth._warp keeps its source 0.001 px inside the last row and column: a grey level at most there
        assert np.array_equal(m0[:-1, :-1], img1[:-1, :-1]) and np.abs(m0.astype(int) - img1.astype(int)).max() <= 1 and k0.all()
        m1, k1 = synth.make_mid(H, W, seed=3, t=1.0, amp_x=12, amp_y=6, style=style)
        d = np.abs(m1.astype(int) - img2.astype(int))[k1]
        # the same warp as make_pair's; "low_texture" keeps a noise of 0.4 grey levels on its road band whatever `noise` is
        assert (d.max() == 0 if style == "dense" else d.max() <= 2 and d.mean() < 0.2) and 0.8 < k1.mean() < 1
        # the mask at t = 1 is where forward_gt's inverse lies inside: the pixels of image 2 that image 1 shows
        mh, kh = synth.make_mid(H, W, seed=3, t=0.5, amp_x=12, amp_y=6, style=style)
        assert mh.dtype == np.uint8 and mh.shape == (H, W, 3) and kh.dtype == bool and kh.mean() > 0.9
    with pytest.raises(ValueError):
        synth.make_mid(H, W, seed=3, t=1.5)


@pytest.mark.parametrize("seed", [3, 7])
@pytest.mark.parametrize("style", ["dense", "low_texture"])
def test_the_true_flow_gains_six_db_over_the_blend(seed, style):
    """120 x 160, amp 12 / 6, no noise, t = 0.5, the true forward flow, forward only: the interpolated frame's PSNR against the
    true middle frame, over make_mid's mask, is at least 6 dB above the plain blend's (a forward-only prototype's smallest gain
    was 9.4 dB)."""
    synth = pkg("synth")
    H, W = 120, 160
    img1, img2, gt = synth.make_pair(H, W, seed=seed, amp_x=12, amp_y=6, noise=0, style=style)
    truth, mask = synth.make_mid(H, W, seed=seed, t=0.5, amp_x=12, amp_y=6, style=style)
    r = R.frame_interp(img1, img2, gt.astype(F), None, t=0.5)
    blend = np.floor(F(0.5) * img1.astype(F) + F(0.5) * img2.astype(F) + F(0.5)).astype(np.uint8)
    p, pb = R.psnr(r["out"], truth, mask), R.psnr(blend, truth, mask)
    print("seed %d %s: interpolated %.2f dB, blend %.2f dB, gain %.2f dB" % (seed, style, p, pb, p - pb))
    assert p >= pb + 6.0
