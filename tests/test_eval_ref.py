"""Flow evaluation without a GPU: the committed jet table, the numpy restatement eval_ref.py against evaluate.error_metrics,
what dflow_flow_eval refuses before it launches anything, flowio.write_png8, visualization.py's arguments and
run_batch --eval's flag.

Mean tolerance against evaluate.error_metrics: that function averages n float32 values with numpy's pairwise sum, whose
relative error for non-negative terms is at most ceil(log2 n) roundings, plus the division by n and the rounding of the
exact mean to float32 it is compared with: (ceil(log2 n) + 2) * 2^-24 relative."""
import ctypes as C
import math
import os
import struct
import zlib

import numpy as np
import pytest

import eval_ref as R
from conftest import GOLDEN_NAMES, pkg


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


# ------------------------------------------------------------------------------------------------ the table
def test_committed_lut_is_the_recipe():
    lut = R.committed_lut()
    assert lut.shape == (256, 3) and np.array_equal(lut, R.jet_lut())
    assert tuple(lut[0]) == (0, 0, 127) and tuple(lut[255]) == (127, 0, 0)          # dark blue .. dark red


def test_committed_lut_is_matplotlibs_jet():
    matplotlib = pytest.importorskip("matplotlib")
    jet = matplotlib.colormaps["jet"]
    assert np.array_equal(R.committed_lut(), np.uint8(jet(np.arange(256))[:, :3] * 255))
    # the float path of the definition picks the entries cmap(float32 t) picks
    e = np.concatenate([np.linspace(0, 3.5, 4001, dtype=np.float32), np.float32(3.0) * np.arange(257, dtype=np.float32) / np.float32(256)])
    t = np.minimum(e, np.float32(3.0)) / np.float32(3.0)
    idx = np.minimum(255, (t * np.float32(256.0)).astype(np.int32))
    assert np.array_equal(R.committed_lut()[idx], np.uint8(jet(t)[:, :3] * 255))


# ------------------------------------------------------------------------------------------------ the reference
def masked_fields(H, W, seed):
    rng = np.random.default_rng(seed)
    gt = np.zeros((H, W, 3), np.float32)
    gt[..., :2] = rng.normal(0, 12, (H, W, 2))
    gt[..., 2] = rng.random((H, W)) > 0.3
    test = np.zeros((H, W, 3), np.float32)
    test[..., :2] = gt[..., :2] + rng.normal(0, 2.5, (H, W, 2))
    test[..., 2] = rng.random((H, W)) > 0.3
    return test, gt


def agrees_with_error_metrics(test, gt, abs_thresh=3.0):
    ev = pkg("evaluate")
    mean, outliers, n = ev.error_metrics(test if test.shape[2] == 3 else ev.to_uv_valid(test), gt, abs_thresh)
    r = R.evaluate(test, gt, abs_thresh)
    assert r["n"] == n and r["n_nonfinite"] == 0 and n > 0
    assert r["n_out_abs"] * 100 / n == outliers
    bound = (math.ceil(math.log2(n)) + 2) * 2.0 ** -24
    assert abs(r["sum_err"] / n - mean) <= bound * mean
    assert r["n_gt_valid"] == int((gt[..., 2] > 0.5).sum())
    return r


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_reference_agrees_with_error_metrics_on_golden_fields(golden, name):
    g = golden(name)
    ev = pkg("evaluate")
    gt = ev.to_uv_valid(g["gt"], g["gt_valid"])
    for field in (g["sparse_t3"], g["sparse_t1"]):
        agrees_with_error_metrics(field, gt)
    dense = g["b0_flow00"].astype(np.float32)                          # the WTA flow, [dy,dx]
    r = agrees_with_error_metrics(dense, gt)
    assert r["n_test_valid"] == dense.shape[0] * dense.shape[1] and r["n"] == int(g["gt_valid"].sum())
    # the picture: black exactly where nothing is counted, the LUT entry elsewhere
    black = (r["bgr"] == 0).all(axis=-1)
    assert np.array_equal(black, r["err"] < 0)
    y, x = np.argwhere(~black)[0]
    t = min(r["err"][y, x], np.float32(3.0)) / np.float32(3.0)
    assert tuple(r["bgr"][y, x][::-1]) == tuple(R.jet_lut()[min(255, int(t * np.float32(256.0)))])


@pytest.mark.parametrize("shape,seed,thresh", [((37, 53), 1, 3.0), ((64, 256), 2, 1.5), ((5, 3), 3, 0.0)])
def test_reference_agrees_with_error_metrics_on_random_masked_fields(shape, seed, thresh):
    agrees_with_error_metrics(*masked_fields(*shape, seed), abs_thresh=thresh)


def test_reference_by_hand():
    gt = np.array([[[100, 0, 1], [100, 0, 1], [0, 0, 1], [0, 0, 0.5], [0, 0, 1], [0, 0, 1], [1, 1, np.nan]]], np.float32)
    test = np.array([[[104, 0, 1], [100, 6, 1], [3, 0, 1], [9, 9, 1], [np.nan, 0, 1], [np.inf, 0, 1], [5, 5, 1]]], np.float32)
    r = R.evaluate(test, gt)
    assert (r["n"], r["n_out_abs"], r["n_out_kitti"], r["n_nonfinite"], r["n_gt_valid"], r["n_test_valid"]) == (3, 2, 1, 2, 5, 7)
    assert r["sum_err"] == 13.0 and r["max_err"] == 6.0
    bits = [int(np.float32(v).view(np.uint32)) for v in (4, 6, 3, -1)]
    assert r["err"][0].view(np.uint32).tolist() == bits + [0x7FC00000, 0x7F800000, bits[3]]
    lut = R.jet_lut()
    assert r["bgr"][0, :3].tolist() == [list(lut[255][::-1])] * 3 and not r["bgr"][0, 3:].any()
    d = R.evaluate(np.ascontiguousarray(test[..., 1::-1]), gt)         # the same flow as [dy,dx]: every pixel valid
    assert d["n_test_valid"] == 7 and d["n"] == 3 and np.array_equal(d["err"].view(np.uint32), r["err"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the C-ABI on the host
def test_abi_rejections_before_any_launch(L):
    lib = L.lib()
    assert C.sizeof(L.EvalStats) == 64
    wsb = lib.dflow_eval_workspace_bytes(436, 1024)
    assert wsb > 0 and lib.dflow_eval_workspace_bytes(436, 1024) == wsb
    assert 0 < lib.dflow_eval_workspace_bytes(1, 1) <= wsb <= lib.dflow_eval_workspace_bytes(8192, 8192) <= 1 << 20
    for h, w in ((0, 8), (8, 0), (8193, 8), (8, 8193), (-1, 8)):
        assert lib.dflow_eval_workspace_bytes(h, w) == 0 and b"size" in lib.dflow_last_error()
    P = 4096                                                  # a non-NULL, aligned stand-in for every device pointer

    def call(h=436, w=1024, test=P, layout=0, gt=P, thresh=3.0, flags=0, stats=P, err=None, bgr=None, ws=P, ws_bytes=wsb):
        return lib.dflow_flow_eval(h, w, test, layout, gt, thresh, flags, stats, err, bgr, ws, ws_bytes, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 8193}, b"size"), ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
                    ({"flags": 2}, b"flags"), ({"flags": 0x80000001}, b"flags"), ({"thresh": float("nan")}, b"abs_thresh"),
                    ({"thresh": float("inf")}, b"abs_thresh"), ({"thresh": -1.0}, b"abs_thresh"),
                    ({"thresh": -1e-30}, b"abs_thresh"), ({"test": None}, b"d_test"), ({"gt": None}, b"d_gt"),
                    ({"stats": None}, b"d_stats"), ({"test": P + 4}, b"d_test"), ({"gt": P + 8}, b"d_gt"),
                    ({"err": P + 4}, b"d_err"), ({"bgr": P + 2}, b"d_err_bgr"), ({"stats": P + 4}, b"d_stats")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(ws=None) == -2 and b"workspace" in lib.dflow_last_error()
    assert call(ws_bytes=wsb - 1) == -2 and b"workspace" in lib.dflow_last_error()
    assert call(ws_bytes=0) == -2


# ------------------------------------------------------------------------------------------------ writers, command lines
def decode_png8(path):
    """(H,W,3) uint8 R,G,B of an 8-bit truecolour PNG whose lines all have filter type 0."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(typ + body) & 0xFFFFFFFF
        pos += 12 + n
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
    w, h, depth, ctype, comp, filt, interlace = hdr
    assert (depth, ctype, comp, filt, interlace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


def test_write_png8_round_trip(tmp_path):
    flowio = pkg("flowio")
    bgr = np.random.default_rng(5).integers(0, 256, (7, 13, 3)).astype(np.uint8)
    path = os.path.join(tmp_path, "e.png")
    flowio.write_png8(path, bgr)
    assert np.array_equal(decode_png8(path), bgr[..., ::-1])
    assert np.array_equal(flowio.read_png16(path), bgr[..., ::-1].astype(np.uint16))      # the package's own reader
    PIL = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(PIL.open(path)), bgr[..., ::-1])
    with pytest.raises(ValueError):
        flowio.write_png8(path, bgr.astype(np.float32))


def test_visualization_arguments(tmp_path, monkeypatch, capsys):
    vis = pkg("visualization")
    monkeypatch.chdir(tmp_path)
    for argv in ([], ["gt.flo"], ["a", "b", "c", "d"]):
        assert vis.main(argv) == 2
        assert "visualization.py <ground truth flow> <test flow>" in capsys.readouterr().err
    assert vis.parse(["gt.png", "t.flo"]) == ("gt.png", "t.flo", None)
    assert vis.parse(["gt.png", "t.flo", "e.png"]) == ("gt.png", "t.flo", "e.png")
    assert vis.parse(["gt.png", "t.flo", "E.PPM"]) == ("gt.png", "t.flo", "E.PPM")
    # any other extension needs PIL: without it, status 2 and the two formats that always work
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    assert vis.parse(["gt.png", "t.flo", "e.jpg"]) == 2
    msg = capsys.readouterr().err
    assert ".png" in msg and ".ppm" in msg
    assert vis.parse(["gt.png", "t.flo", "e.png"]) == ("gt.png", "t.flo", "e.png")
    assert not os.listdir(tmp_path), "nothing is written before the arguments are accepted"


def test_run_batch_eval_flag():
    ap = pkg("run_batch").parser()
    assert ap.parse_args([]).eval is False
    assert ap.parse_args(["--eval"]).eval is True
