"""tests/pyramid_ref.py, the numpy statement of dflow_pyr_down and dflow_flow_upsample (include/dflow.h), pinned by hand:
every expectation here is a literal worked out from the definitions, not from the code (CPU only)."""
import numpy as np

import pyramid_ref as R

NAN, INF = np.nan, np.inf


def test_literal_3x4_image():
    img = np.array([[[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]],
                    [[5, 15, 25], [35, 45, 55], [65, 75, 85], [95, 105, 115]],
                    [[200, 210, 220], [230, 240, 250], [0, 1, 2], [255, 254, 253]]], np.uint8)
    # out[0][0], channel 0: rows clamp(-2..2) = 0,0,0,1,2 -> weights 11, 4, 1; columns likewise.  Row sums over the columns:
    # 11*10 + 4*40 + 70 = 340, 11*5 + 4*35 + 65 = 260, 11*200 + 4*230 + 0 = 3120; 11*340 + 4*260 + 3120 = 7900; (7900 + 128) >> 8 = 31
    want = [[[31, 41, 51], [72, 82, 91]], [[139, 149, 159], [123, 128, 134]]]
    assert R.pyr_down(img).tolist() == want
    # out[1][1], channel 2: rows clamp(0..4) = 0,1,2,2,2 -> weights 1, 4, 11; columns clamp(0..4) = 0,1,2,3,3 -> 1, 4, 6, 5
    rows = [30 + 4 * 60 + 6 * 90 + 5 * 120, 25 + 4 * 55 + 6 * 85 + 5 * 115, 220 + 4 * 250 + 6 * 2 + 5 * 253]
    assert (rows[0] + 4 * rows[1] + 11 * rows[2] + 128) >> 8 == 134


def test_constant_images_stay_constant():
    for h, w in ((1, 1), (2, 3), (7, 9), (16, 33)):
        for v in (0, 1, 127, 254, 255):
            out = R.pyr_down(np.full((h, w, 3), v, np.uint8))
            assert out.shape == ((h + 1) // 2, (w + 1) // 2, 3) and out.dtype == np.uint8 and (out == v).all(), (h, w, v)


def test_single_bright_pixel_gives_the_footprint_and_the_rounding():
    img = np.zeros((9, 9, 3), np.uint8)
    img[4, 4] = (255, 200, 7)
    out = R.pyr_down(img)
    assert out.shape == (5, 5, 3)
    # centre (2,2) sees weight 6*6, its neighbours 6*1 and 1*1; 36*255 = 9180 -> 36, 6*255 = 1530 -> 6, 255 -> (255 + 128) >> 8 = 1
    assert out[..., 0].tolist() == [[0, 0, 0, 0, 0], [0, 1, 6, 1, 0], [0, 6, 36, 6, 0], [0, 1, 6, 1, 0], [0, 0, 0, 0, 0]]
    # 7200 / 256 = 28.125 -> 28; 1200 / 256 = 4.69 -> 5; 200 / 256 = 0.78 -> 1: rounding to nearest, not truncation
    assert out[..., 1].tolist() == [[0, 0, 0, 0, 0], [0, 1, 5, 1, 0], [0, 5, 28, 5, 0], [0, 1, 5, 1, 0], [0, 0, 0, 0, 0]]
    # 36*7 = 252 -> (252 + 128) >> 8 = 1; 42 and 7 -> 0
    assert out[..., 2].tolist() == [[0] * 5, [0] * 5, [0, 0, 1, 0, 0], [0] * 5, [0] * 5]
    # an odd position is seen by the even samples next to it with weight 4: (1,1) -> 4*4*255 = 4080 -> 16 at four outputs
    img = np.zeros((4, 4, 3), np.uint8)
    img[1, 1, 0] = 255
    assert R.pyr_down(img)[..., 0].tolist() == [[16, 16], [16, 16]]


def test_one_by_one_and_one_by_five():
    assert R.pyr_down(np.array([[[3, 200, 255]]], np.uint8)).tolist() == [[[3, 200, 255]]]
    row = np.array([[[1, 2, 3], [9, 9, 9], [100, 0, 0], [0, 50, 0], [7, 7, 255]]], np.uint8)
    # h = 1: every row tap is row 0, vertical weight 16.  x = 0: columns 0,0,0,1,2 -> 11, 4, 1; x = 1 (centre 2): 1,4,6,4,1;
    # x = 2 (centre 4): columns 2,3,4,4,4 -> 1, 4, 11.  Channel 0: 16 * (11 + 36 + 100) = 2352 -> 9; 16 * (1 + 36 + 600 + 0 + 7) =
    # 10304 -> 40; 16 * (100 + 0 + 77) = 2832 -> 11
    assert R.pyr_down(row).tolist() == [[[9, 4, 4], [40, 15, 18], [11, 17, 175]]]
    assert (16 * (0 + 4 * 0 + 11 * 255) + 128) >> 8 == 175 and (16 * (2 + 36 + 0 + 200 + 7) + 128) >> 8 == 15


C22 = np.array([[[1, 2], [3, -4]], [[5, 6], [-7, 8.5]]], np.float32)         # [dy,dx]: U = [[2,-4],[6,8.5]], V = [[1,3],[5,-7]]
U33 = [[4, -2, -8], [8, 6.25, 4.5], [12, 14.5, 17]]                           # 2a at even/even, a + b between two, sum/2 of four
V33 = [[2, 4, 6], [6, 1, -4], [10, -2, -14]]


def grow(m, h, w):
    """A 3x3 expectation at the four parities: the fine pixels of the last odd row / column see the clamped corner twice."""
    m = [r + [r[2]] * (w - 3) for r in m]
    return m + [m[2]] * (h - 3)


def test_literal_2x2_flow_at_the_four_parities():
    for h, w in ((3, 3), (3, 4), (4, 3), (4, 4)):
        out, counts = R.flow_upsample(C22, (h, w))
        assert out.dtype == np.float32 and out.shape == (h, w, 3)
        assert out[..., 0].tolist() == grow(U33, h, w) and out[..., 1].tolist() == grow(V33, h, w), (h, w)
        assert (out[..., 2] == 1).all() and counts == [h * w, 0, 0]
        uvv = np.concatenate([C22[..., ::-1], np.ones((2, 2, 1), np.float32)], axis=-1)
        out2, counts2 = R.flow_upsample(np.ascontiguousarray(uvv), (h, w))
        assert out2.tobytes() == out.tobytes() and counts2 == counts, "the two layouts say the same"


def test_invalid_corners():
    uvv = np.concatenate([C22[..., ::-1], np.ones((2, 2, 1), np.float32)], axis=-1)
    a = uvv.copy()
    a[0, 1, 2] = 0.0                                    # corner (0,1) invalid
    out, counts = R.flow_upsample(a, (3, 3))
    # (0,0) and row 2 left do not touch it: BILINEAR; (0,1), (1,1): (y0,x0) = (0,0) is good: NEAREST 2 * [2, 1];
    # (0,2), (1,2): (y0,x0) = (0,1) itself: INVALID
    assert out[0].tolist() == [[4, 2, 1], [4, 2, 1], [0, 0, 0]]
    assert out[1].tolist() == [[8, 6, 1], [4, 2, 1], [0, 0, 0]]
    assert out[2].tolist() == [[12, 10, 1], [14.5, -2, 1], [17, -14, 1]]
    assert counts == [5, 2, 2]
    for bad in (0.5, NAN, -1.0):                        # valid must exceed 0.5; a NaN compares false
        b = uvv.copy()
        b[0, 0, 2] = bad
        out, counts = R.flow_upsample(b, (3, 3))
        assert out[0, 0].tolist() == [0, 0, 0] and out[0, 1].tolist() == [0, 0, 0] and out[1, 1].tolist() == [0, 0, 0]
        assert out[0, 2].tolist() == [-8, 6, 1] and counts == [5, 0, 4]
    b = uvv.copy()
    b[0, 0, 2] = 0.50001
    assert R.flow_upsample(b, (3, 3))[1] == [9, 0, 0]


def test_non_finite_and_overflowing_components():
    for bad in (NAN, INF, -INF):
        for comp in (0, 1):
            c = C22.copy()
            c[1, 1, comp] = bad                         # under [dy,dx] every pixel is valid, but this one is not good
            out, counts = R.flow_upsample(c, (3, 3))
            assert np.isfinite(out).all()
            assert out[2, 2].tolist() == [0, 0, 0] and out[1, 1].tolist() == [4, 2, 1] and out[2, 1].tolist() == [12, 10, 1]
            assert out[1, 2].tolist() == [-8, 6, 1] and counts == [5, 3, 1]
    big = np.float32(3e38)
    c = np.zeros((2, 2, 2), np.float32)
    c[0, 0] = (1.0, big)                                # U = [[3e38, 0], [0, 0]]: good, but 2a overflows
    out, counts = R.flow_upsample(c, (3, 3))
    # (0,0): (a + a) + (a + a) and 2a are both inf: INVALID.  (0,1): y1 = y0, so the corners are a, b, a, b and the written sum is
    # (a + b) + (a + b) = 3e38 + 3e38 = inf although a + b fits: one IEEE operation per written operation; 2a is inf too: INVALID.
    # (1,0) likewise.  (1,1): four different corners, ((a + 0) + (0 + 0)) * 0.5 = 1.5e38: BILINEAR
    assert out[0, 0].tolist() == [0, 0, 0] and out[0, 1].tolist() == [0, 0, 0] and out[1, 0].tolist() == [0, 0, 0]
    assert out[1, 1].tolist() == [float(big * np.float32(0.5)), 0.5, 1] and out[0, 2].tolist() == [0, 0, 1]
    assert counts == [6, 0, 3]
    c[0, 1] = (0.0, big)                                # U = [[3e38, 3e38], [0, 0]]: now a + b overflows wherever row 0 is seen
    out, counts = R.flow_upsample(c, (3, 3))
    assert not out[:2].any() and out[2].tolist() == [[0, 0, 1]] * 3 and counts == [3, 0, 6]
    c = np.zeros((2, 2, 2), np.float32)
    c[0, 0] = (-big, 2.0)
    c[0, 1] = (big, 4.0)                                # V = -3e38 and 3e38: their sum is 0, BILINEAR between them
    out, counts = R.flow_upsample(c, (3, 3))
    assert out[0, 1].tolist() == [6, 0, 1] and out[0, 0].tolist() == [0, 0, 0] and out[0, 2].tolist() == [0, 0, 0]
    c = np.zeros((2, 2, 2), np.float32)
    c[0, 0] = (0.0, 1.5e38)
    c[0, 1] = (0.0, big)                                # a + b = 4.5e38 overflows, 2a = 3e38 does not: NEAREST at (0,1)
    out, counts = R.flow_upsample(c, (3, 3))
    assert out[0, 1].tolist() == [float(np.float32(1.5e38) * np.float32(2)), 0, 1] and out[0, 0].tolist() == out[0, 1].tolist()
    # (1,0): (a + a) + 0 = 3e38, half of it 1.5e38: BILINEAR; (1,1): (a + b) is inf: NEAREST 2a; (0,2), (1,2): b + b is inf: INVALID
    assert out[1, 0].tolist() == [float(np.float32(1.5e38)), 0, 1] and out[1, 1].tolist() == out[0, 1].tolist()
    assert counts == [4, 3, 2]                          # (0,0) is NEAREST too: (a + a) + (a + a) overflows; row 2 is BILINEAR


def test_counts_add_up():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (2, 3), (7, 9), (45, 35)):
        hc, wc = R.coarse_size(h, w)
        c = rng.normal(0, 5, (hc, wc, 3)).astype(np.float32)
        c[..., 2] = rng.random((hc, wc)) > 0.3
        out, counts = R.flow_upsample(c, (h, w))
        assert sum(counts) == h * w and counts[0] + counts[1] == int(out[..., 2].sum())
        assert (out[out[..., 2] == 0] == 0).all()
