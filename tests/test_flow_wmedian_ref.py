"""Facts about the definition of dflow_flow_wmedian, checked on its numpy restatement (tests/flow_wmedian_ref.py), which the GPU
tests compare the kernel with byte for byte (CPU only)."""
import numpy as np

import flow_wmedian_ref as R

F = np.float32
H, W = 17, 19


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def good_field(u, v):
    f = np.ones(u.shape + (3,), F)
    f[..., 0], f[..., 1] = u, v
    return f


def test_radius_one_is_the_plain_median_of_the_3x3_window():
    rng = np.random.default_rng(1)
    f = good_field(rng.integers(-9, 10, (H, W)), rng.integers(-9, 10, (H, W)))
    for layout in (R.UVV, R.DYDX):
        out, counts = R.flow_wmedian(R.as_layout(f, layout), radius=1)
        for c in (0, 1):
            win = np.stack([f[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx, c] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=2)
            assert (out[1:-1, 1:-1, c] == np.median(win, axis=2)).all()
        assert (out[..., 2] == 1).all() and counts[:3] == [H * W, H * W, 0]
    # the window is clipped, not padded: a corner is the lower median of its four pixels
    assert out[0, 0, 0] == np.sort(f[:2, :2, 0].ravel())[1]


def test_outliers_leave_a_constant_field_and_are_what_reject_removes():
    f = good_field(np.full((H, W), 3.0), np.full((H, W), -2.0))
    f[::4, ::4, 0], f[::4, ::4, 1] = 40.0, 25.0
    assert f[::4, ::4, 0].size == 25
    out, counts = R.flow_wmedian(f, radius=1)
    assert (out == np.array([3, -2, 1], F)).all() and counts == [323, 323, 0, 25]
    out, counts = R.flow_wmedian(f, radius=1, reject_thresh=1.0, flags=R.REJECT)
    hit = np.zeros((H, W), bool)
    hit[::4, ::4] = True
    assert (out[hit] == 0).all() and (bits(out[~hit]) == bits(f[~hit])).all() and counts == [323, 298, 0, 25]
    # a threshold no difference exceeds keeps everything, bit for bit
    out, counts = R.flow_wmedian(f, radius=1, reject_thresh=1e30, flags=R.REJECT)
    assert (bits(out) == bits(f)).all() and counts == [323, 323, 0, 0]


def test_a_hole_is_filled_unless_it_is_kept():
    rng = np.random.default_rng(2)
    f = good_field(rng.integers(-2, 3, (H, W)), rng.integers(-2, 3, (H, W)))
    f[6:9, 7:10] = 0
    out, counts = R.flow_wmedian(f, radius=2)
    assert (out[..., 2] == 1).all() and counts[:3] == [H * W - 9, H * W, 9]
    out, counts = R.flow_wmedian(f, radius=2, flags=R.KEEP_HOLES)
    assert (out[6:9, 7:10] == 0).all() and out[..., 2].sum() == H * W - 9 and counts[:3] == [H * W - 9, H * W - 9, 0]
    out, counts = R.flow_wmedian(f, radius=2, reject_thresh=1e30, flags=R.REJECT)
    assert (out[6:9, 7:10] == 0).all() and counts == [H * W - 9, H * W - 9, 0, 0]
    # a hole wider than the window stays a hole at its centre: W == 0
    g = f.copy()
    g[2:13, 3:14] = 0
    out, _ = R.flow_wmedian(g, radius=2)
    assert (out[7, 8] == 0).all() and out[2, 3, 2] == 1
    # a NaN or an Inf under valid = 1 is a hole too, and never an output
    n = f.copy()
    n[6:9, 7:10] = (np.nan, np.inf, 1)
    out2, counts2 = R.flow_wmedian(n, radius=2)
    assert np.isfinite(out2).all() and counts2[:3] == [H * W - 9, H * W, 9]
    assert (bits(out2) == bits(R.flow_wmedian(f, radius=2)[0])).all()


def test_the_guide_pulls_a_flow_edge_onto_the_image_edge():
    img = np.zeros((H, W, 3), np.uint8)
    img[:, 10:] = 200
    f = good_field(np.where(np.arange(W) < 8, 1.0, 5.0)[None, :].repeat(H, 0), np.zeros((H, W)))
    space, color = R.tables(3, None, 10.0)
    out, _ = R.flow_wmedian(f, img, radius=3, wcolor=color)
    assert (out[:, :10, 0] == 1).all() and (out[:, 10:, 0] == 5).all()
    out, _ = R.flow_wmedian(f, radius=3)
    assert (out[:, :8, 0] == 1).all() and (out[:, 8:, 0] == 5).all()


def test_every_output_is_a_sample_of_its_window():
    for kind in ("frac", "holes", "wide", "zeros"):
        f = R.field(H, W, 3, kind)
        img = R.image(H, W, 4)
        for name, (space, color) in R.table_sets(2, 5).items():
            out, counts = R.flow_wmedian(f, img if color is not None else None, radius=2, wspace=space, wcolor=color)
            ub, vb, good = R.split(f)
            for y, x in zip(*np.nonzero(out[..., 2])):
                win = (slice(max(y - 2, 0), y + 3), slice(max(x - 2, 0), x + 3))
                assert bits(out[y, x, 0]) in ub[win][good[win]] and bits(out[y, x, 1]) in vb[win][good[win]], (kind, name, y, x)
            assert counts[1] == int(out[..., 2].sum()) and (out[out[..., 2] == 0] == 0).all()


def test_no_weight_no_output():
    # only the window's corners weigh: at the centre of a 3x3 field they all lie outside, so W == 0 at a good pixel
    f = R.field(3, 3, 6, "frac")
    space = np.zeros((3, 3), np.uint8)
    space[2, 2] = 9
    out, counts = R.flow_wmedian(f, radius=2, wspace=space)
    assert (out[1, 1] == 0).all() and (out[0, 0] == f[2, 2]).all() and counts == [9, 4, 0, 9]
    out, counts = R.flow_wmedian(f, radius=2, wspace=space, reject_thresh=1e30, flags=R.REJECT)
    assert (out[1, 1] == 0).all() and (bits(out[0, 0]) == bits(f[0, 0])).all() and counts == [9, 4, 0, 5]
    out, counts = R.flow_wmedian(R.field(3, 3, 6, "none"), radius=2)
    assert (out == 0).all() and counts == [0, 0, 0, 0]


def test_the_order_of_the_zeros_and_of_the_keys():
    assert R.keys(bits(F(-0.0))) < R.keys(bits(F(0.0)))
    v = np.array([-np.inf, -1e30, -1.5, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 1.5, 1e30, np.inf], F)
    k = R.keys(bits(v)).astype(np.int64)
    assert (np.diff(k) > 0).all()
    # two -0 and two +0 in a row: the lower median of four is the second, a -0; with one more +0 it is +0
    f = good_field(np.array([[-0.0, 0.0, -0.0, 0.0]], F), np.zeros((1, 4), F))
    out, _ = R.flow_wmedian(f, radius=8, wspace=np.ones(81, np.uint8))
    assert (bits(out[..., 0]) == 0x80000000).all()
    f = good_field(np.array([[-0.0, 0.0, -0.0, 0.0, 0.0]], F), np.zeros((1, 5), F))
    out, _ = R.flow_wmedian(f, radius=8)
    assert (bits(out[..., 0]) == 0).all()


def test_the_weights_decide():
    # three samples 1, 2, 9 in a row; at the middle pixel the weights are (left, centre, right)
    f = good_field(np.array([[1.0, 2.0, 9.0]], F), np.zeros((1, 3), F))
    for centre, side, want in ((1, 1, 2.0), (1, 3, 2.0), (0, 1, 1.0), (2, 1, 2.0)):
        out, _ = R.flow_wmedian(f, radius=1, wspace=np.array([centre, side, side, side], np.uint8))
        assert out[0, 1, 0] == want, (centre, side)
    img = np.array([[[0, 0, 0], [100, 100, 100], [100, 100, 110]]], np.uint8)
    color = np.zeros(R.NCOLOR, np.uint8)
    color[0], color[10] = 1, 3                                              # the right neighbour outweighs the pixel itself
    out, _ = R.flow_wmedian(f, img, radius=1, wcolor=color)
    assert out[0, 1, 0] == 9.0 and out[0, 0, 0] == 1.0 and out[0, 2, 0] == 2.0


def test_the_tables_of_the_restatement():
    for radius in (1, 3, 8):
        space, color = R.tables(radius, 1.5, 10.0)
        assert space[0, 0] == 255 and color[0] == 255 and (np.diff(color.astype(int)) <= 0).all()
        assert (np.diff(space.astype(int), axis=0) <= 0).all() and (np.diff(space.astype(int), axis=1) <= 0).all()
        assert abs(int(space[1, 1]) - 255 * np.exp(-2 / 4.5)) <= 1 and abs(int(color[45]) - 255 * np.exp(-1.5)) <= 1


def select_by_bits(samples):
    """The kernel's method (csrc/flow_wmedian.hip) on one window's [(weight, key)], all weights > 0: the common leading bits
    from the least and greatest key, then one bit per sweep."""
    W = sum(wq for wq, _ in samples)
    lo, hi = min(k for _, k in samples), max(k for _, k in samples)
    if lo == hi:
        return lo
    bit = 1 << ((lo ^ hi).bit_length() - 1)
    mask = ~(bit - 1) & 0xFFFFFFFF
    pre, acc = lo & (mask << 1) & 0xFFFFFFFF, 0
    while bit:
        sum0 = sum(wq for wq, k in samples if ((k ^ pre) & mask) == 0)
        if 2 * (acc + sum0) < W:
            acc += sum0
            pre |= bit
        bit >>= 1
        mask |= bit
    return pre


def test_selection_by_bits_finds_the_same_sample_as_sorting():
    h, w, r = 9, 11, 2
    img = R.image(h, w, 2).astype(int)
    for kind in R.KINDS:
        f = R.field(h, w, 1, kind)
        ub, vb, good = R.split(f)
        ku, kv = R.keys(ub), R.keys(vb)
        for name, (space, color) in R.table_sets(r, 3).items():
            out, _ = R.flow_wmedian(f, img if color is not None else None, radius=r, wspace=space, wcolor=color)
            for y in range(h):
                for x in range(w):
                    su, sv = [], []
                    for yy in range(max(y - r, 0), min(y + r, h - 1) + 1):
                        for xx in range(max(x - r, 0), min(x + r, w - 1) + 1):
                            S = 1 if space is None else int(space[abs(yy - y), abs(xx - x)])
                            C = 1 if color is None else int(color[np.abs(img[yy, xx] - img[y, x]).sum()])
                            if good[yy, xx] and S * C:
                                su.append((S * C, int(ku[yy, xx])))
                                sv.append((S * C, int(kv[yy, xx])))
                    if not su:
                        assert (out[y, x] == 0).all()
                        continue
                    got = R.keys(bits(out[y, x]))
                    assert out[y, x, 2] == 1 and int(got[0]) == select_by_bits(su) and int(got[1]) == select_by_bits(sv), (kind, name, y, x)
