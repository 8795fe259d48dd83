"""Flow pictures and the warp check without a GPU: the numpy restatements of flowpic_ref.py pinned by hand-computed values, the
committed wheel against the recipe, the inputs of tests/test_gpu_flowpic.py against the condition its colour tolerance rests
on, flowio.read_png8, and the new command-line flags."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import flowpic_ref as R
from conftest import PKG, ROOT, pkg

F = np.float32


def uvv(rows):
    return np.array(rows, F).reshape(1, -1, 3)


# ------------------------------------------------------------------------------------------------ the wheel
def test_wheel():
    w = R.wheel()
    assert w.shape == (55, 3) and tuple(w[0]) == (255, 0, 0) and tuple(w[54]) == (255, 0, 43)
    assert tuple(w[15]) == (255, 255, 0) and tuple(w[21]) == (0, 255, 0) and tuple(w[25]) == (0, 255, 255)
    assert tuple(w[36]) == (0, 0, 255) and tuple(w[49]) == (255, 0, 255) and tuple(w[1]) == (255, 17, 0)
    assert w.min() == 0 and w.max() == 255


def test_committed_wheel_is_the_recipe():
    text = open(os.path.join(ROOT, PKG, "csrc", "flow_wheel.h")).read()
    v = np.array([int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{6})u", text)], np.int64)
    assert re.search(r"#define\s+FLOW_WHEEL_N\s+55\b", text) and v.size == 55
    assert np.array_equal(np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1), R.wheel())


# ------------------------------------------------------------------------------------------------ the colour picture
def test_color_by_hand():
    w = R.wheel()
    r = R.flow_color(uvv([(0, 0, 1)]))
    assert r["maxrad"] == 1.0 and r["bgr"].tolist() == [[[255, 255, 255]]]            # zero flow: white, radius 1
    r = R.flow_color(uvv([(6, 0.0, 1), (6, -0.0, 1), (0, 6, 1), (0, 0, 1), (-0.0, -0.0, 1)]))
    assert r["maxrad"] == 6.0 and r["maxrad"].dtype == np.float32
    assert r["bgr"][0, 0].tolist() == [0, 0, 255] and r["c"][0, 0].tolist() == [0.0, 0.0, 255.0]      # entry 0 at rad = 1
    # (U > 0, V = -0): atan2(+0, -1) = +pi, fk = 54, f = 0: entry 54 = (255, 0, 43), whatever the last bits of 255 * col
    assert r["bgr"][0, 1].tolist() == [43, 0, 255] and np.allclose(r["c"][0, 1], w[54][::-1], rtol=0, atol=1e-12)
    # (U = 0, V > 0): a = -1/2, fk = 13.5: the midpoint of entries 13 and 14
    mid = (w[13] + w[14]) / 2.0
    assert np.allclose(r["c"][0, 2], mid[::-1], rtol=0, atol=1e-12) and r["bgr"][0, 2].tolist() == [0, 229, 255]
    assert r["bgr"][0, 3].tolist() == [255] * 3 and r["bgr"][0, 4].tolist() == [255] * 3
    # beyond the radius the colour is dimmed to three quarters; at half of it, half way to white
    r = R.flow_color(uvv([(12, 0.0, 1), (3, 0.0, 1)]), max_flow=6.0)
    assert r["maxrad"] == 6.0 and r["c"][0, 0].tolist() == [0.0, 0.0, 191.25] and r["c"][0, 1].tolist() == [127.5, 127.5, 255.0]


def test_color_unknown_pixels():
    nan, inf = np.nan, np.inf
    rows = [(3, 4, 1), (1e6, 1e6, 0), (nan, 0, 1), (0, inf, 1), (2e9, 0, 1), (0, -2e9, 1), (50, 50, 0.5), (50, 50, nan), (1e9, 0, 0.4)]
    r = R.flow_color(uvv(rows))
    assert r["known"][0].tolist() == [True] + [False] * 8
    assert r["maxrad"] == 5.0, "unknown pixels do not enter the automatic radius"
    assert not r["bgr"][0, 1:].any() and not r["c"][0, 1:].any() and r["bgr"][0, 0].any()
    assert R.flow_color(uvv(rows[1:]))["maxrad"] == 1.0                                # no known pixel: radius 1
    r = R.flow_color(uvv([(1e9, 0, 1), (-1e9, 1e9, 1)]))                               # 1e9 itself is known
    assert r["known"].all() and r["maxrad"] == np.sqrt(F(1e9) * F(1e9) + F(1e9) * F(1e9))
    d = R.flow_color(np.array([[[4, 3], [nan, 0]]], F))                                # [dy,dx]: U = 3, V = 4
    u = R.flow_color(uvv([(3, 4, 1), (0, nan, 1)]))
    assert np.array_equal(d["c"], u["c"]) and d["maxrad"] == 5.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_gpu_inputs_keep_out_of_the_band(H, W):
    """What the tolerance of test_gpu_flowpic.py rests on: in every field it colours, at most 1 % of the pixels have a channel
    with 0 < |c - rint(c)| <= 1e-6 (where the byte could depend on atan2's last bit)."""
    for scale in R.SCALES:
        flow, where = R.color_case(H, W, scale)
        assert len(where) == min(H * W, len(R.color_planted()))
        for field in (flow, R.dydx(flow)):
            for max_flow in (0.0, 10.0):
                r = R.flow_color(field, max_flow)
                n = int(R.near_integer(r["c"]).sum())
                print("%dx%d scale %g layout %d max_flow %g: %d of %d pixels in the band" % (H, W, scale, field.shape[2], max_flow, n, H * W))
                assert n <= 0.01 * H * W
                assert r["maxrad"] == (R.BIG if max_flow == 0 else F(max_flow))
    if H * W > 100:
        assert 0.7 * H * W < R.flow_color(flow)["known"].sum() < H * W - 5


def test_gpu_big_input_keeps_out_of_the_band():
    """The same for the one field beyond the capped grid, which test_gpu_flowpic.py colours with the automatic radius."""
    (H, W), scale = R.BIG_SHAPE, R.BIG_SCALE
    flow, where = R.color_case(H, W, scale)
    assert len(where) == len(R.color_planted())
    for field in (flow, R.dydx(flow)):
        r = R.flow_color(field)
        n = int(R.near_integer(r["c"]).sum())
        print("%dx%d scale %g layout %d: %d of %d pixels in the band" % (H, W, scale, field.shape[2], n, H * W))
        assert n <= 0.01 * H * W and r["maxrad"] == R.BIG
        if field is flow:
            assert 0.7 * H * W < r["known"].sum() < H * W - 5


# ------------------------------------------------------------------------------------------------ the warp
def test_warp_integer_flow_reproduces_shifted_pixels():
    rng = np.random.default_rng(3)
    H, W = 6, 9
    img1, img2 = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    flow = np.zeros((H, W, 3), F)
    flow[..., 0], flow[..., 1], flow[..., 2] = 2, -1, 1
    r = R.warp(img1, img2, flow)
    inside = np.zeros((H, W), bool)
    inside[1:, :W - 2] = True
    assert r["n"] == inside.sum() and r["n_outside"] == H * W - r["n"] and r["n_unknown"] == 0
    assert np.array_equal(r["warped"][1:, :W - 2], img2[:H - 1, 2:]) and not r["warped"][~inside].any()
    d = np.abs(img2[:H - 1, 2:].astype(np.int64) - img1[1:, :W - 2]).sum(axis=-1)
    assert np.array_equal(r["err"][1:, :W - 2], (d.astype(F) / F(3))) and (r["err"][~inside] == -1).all()
    assert r["max_err"] == float(F(d.max()) / F(3)) and abs(r["sum_err"] - d.sum() / 3.0) <= 1e-6 * d.sum()
    assert r["n_above"] == int((d.astype(F) / F(3) > 10).sum())
    same = R.warp(img1, img1, np.zeros((H, W, 2), F))                   # [dy,dx] zeros: every pixel onto itself
    assert same["n"] == H * W and same["sum_err"] == 0.0 and np.array_equal(same["warped"], img1)
    assert (same["bgr"] == np.array([127, 0, 0], np.uint8)).all()       # jet's first entry, (b,g,r)


def test_warp_half_pixel_on_a_two_value_image():
    H, W = 2, 4
    img2 = np.zeros((H, W, 3), np.uint8)
    img2[:, 1::2] = 100                                                  # columns 0 100 0 100
    img2[1] //= 2                                                        # second row 0 50 0 50
    img1 = np.full((H, W, 3), 50, np.uint8)
    flow = np.zeros((H, W, 3), F)
    flow[..., 2] = 1
    flow[0, 0, :2] = (0.5, 0)        # between 0 and 100: 50
    flow[0, 1, :2] = (0, 0.5)        # between 100 and 50: 75
    flow[0, 2, :2] = (0.5, 0.5)      # ((0 + 100) / 2 + (0 + 50) / 2) / 2 = 37.5 -> 38
    flow[1, 3, :2] = (0, 0.5)        # below the last row
    r = R.warp(img1, img2, flow)
    assert r["warped"][0, :3, 0].tolist() == [50, 75, 38] and r["err"][0, :3].tolist() == [0.0, 25.0, 12.5]
    assert r["err"][1, 3] == -1 and r["n"] == 7 and r["n_outside"] == 1 and r["n_above"] == 5
    assert r["err"][1].tolist()[:3] == [50.0, 0.0, 50.0]


def test_warp_edges_of_the_frame():
    H, W = 3, 5
    rng = np.random.default_rng(4)
    img1, img2 = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    up = lambda v: np.nextafter(F(v), F(np.inf))
    flow = np.zeros((H, W, 3), F)
    flow[..., 2] = 1
    flow[0, 0, 0] = W - 1            # the target is the last column exactly: inside, x1 = x0 = w - 1
    flow[1, 0, 0] = up(W - 1)        # one float32 step beyond: outside
    flow[0, 1, 1] = H - 1
    flow[0, 2, 1] = up(H - 1)
    flow[2, 2, 0] = -up(2)           # one step below 0
    flow[2, 3] = (np.nan, 0, 1)
    flow[2, 4] = (0, 0, 0)
    r = R.warp(img1, img2, flow)
    assert r["err"][0, 0] >= 0 and np.array_equal(r["warped"][0, 0], img2[0, W - 1]) and np.array_equal(r["warped"][0, 1], img2[H - 1, 1])
    assert [r["err"][p] for p in ((1, 0), (0, 2), (2, 2), (2, 3), (2, 4))] == [-1] * 5
    assert (r["n"], r["n_outside"], r["n_unknown"]) == (H * W - 5, 3, 2)
    assert not r["bgr"][1, 0].any() and not r["warped"][2, 3].any()


def test_gpu_warp_inputs_hold_every_kind():
    for H, W in R.SHAPES:
        for scale in R.SCALES:
            img1, img2, flow, where = R.warp_case(H, W, scale)
            r = R.warp(img1, img2, flow)
            assert r["n"] + r["n_outside"] + r["n_unknown"] == H * W
            if H * W > 100:
                assert min(r["n"], r["n_outside"], r["n_unknown"]) > 100 and 0 < r["n_above"] and len(where) == 14
                y, x = divmod(int(where[1]), W)
                assert r["err"][y, x] >= 0 and np.array_equal(r["warped"][y, x], img2[y, W - 1])
            y, x = divmod(int(where[0]), W)
            assert x == 0 and r["err"][y, x] == -1, "one float32 step beyond the last column is outside"


# ------------------------------------------------------------------------------------------------ files and flags
def png(path, w, h, ctype, lines):
    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(b"".join(lines))) + chunk(b"IEND", b""))


def test_read_png8(tmp_path):
    flowio = pkg("flowio")
    bgr = np.random.default_rng(5).integers(0, 256, (7, 13, 3)).astype(np.uint8)
    path = os.path.join(tmp_path, "a.png")
    flowio.write_png8(path, bgr)
    back = flowio.read_png8(path)
    assert back.dtype == np.uint8 and back.flags["C_CONTIGUOUS"] and np.array_equal(back, bgr)
    # a grey file, its second line with the Sub filter: three equal channels
    grey = np.array([[10, 20, 30], [5, 250, 7]], np.uint8)
    sub = bytes([1, 5, (250 - 5) & 255, (7 - 250) & 255])
    png(path, 3, 2, 0, [b"\x00" + grey[0].tobytes(), sub])
    assert np.array_equal(flowio.read_png8(path), np.repeat(grey[..., None], 3, axis=2))
    png(path, 2, 1, 6, [b"\x00" + bytes(8)])                             # RGBA
    with pytest.raises(ValueError, match="8-bit RGB or grey"):
        flowio.read_png8(path)
    flowio.write_png16(path, np.zeros((2, 2, 3), np.uint16))
    with pytest.raises(ValueError, match="8-bit RGB or grey"):
        flowio.read_png8(path)


def test_flowpicture_arguments_and_images(tmp_path, capsys):
    fp = pkg("flowpicture")
    a = fp.parser().parse_args(["f.flo", "p.png", "--max-flow", "8"])
    assert (a.flow, a.picture, a.max_flow, a.warp) == ("f.flo", "p.png", 8.0, None)
    a = fp.parser().parse_args(["f.npy", "--warp", "a.png", "b.ppm", "--warped", "w.png", "--error-picture", "e.ppm"])
    assert (a.picture, a.warp, a.warped, a.error_picture, a.err_thresh, a.err_max) == (None, ["a.png", "b.ppm"], "w.png", "e.ppm", 10.0, 30.0)
    for argv in (["f.flo"], ["f.flo", "--warped", "w.png"]):
        with pytest.raises(SystemExit):
            fp.main(argv)
    capsys.readouterr()
    # the three image formats give the same (H,W,3) uint8 BGR array
    bgr = np.random.default_rng(6).integers(0, 256, (4, 6, 3)).astype(np.uint8)
    paths = [os.path.join(tmp_path, "i" + ext) for ext in (".npy", ".ppm", ".png")]
    np.save(paths[0], bgr)
    pkg("flowio").write_picture(paths[1], bgr)
    pkg("flowio").write_picture(paths[2], bgr)
    for p in paths:
        assert np.array_equal(pkg("flowio").read_image(p), bgr), p
    with open(paths[1], "wb") as f:
        f.write(b"P6\n# a comment\n6 4\n255\n" + bgr[..., ::-1].tobytes())
    assert np.array_equal(pkg("flowio").read_image(paths[1]), bgr)
    with pytest.raises(ValueError):
        pkg("flowio").read_image(os.path.join(tmp_path, "i.jpg"))


def test_run_batch_flags():
    ap = pkg("run_batch").parser()
    a = ap.parse_args([])
    assert a.pictures is False and a.photo is False
    a = ap.parse_args(["--pictures", "--photo"])
    assert a.pictures is True and a.photo is True
