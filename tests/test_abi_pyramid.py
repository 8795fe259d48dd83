"""What dflow_pyr_down and dflow_flow_upsample refuse on the host, before anything is launched, what their Python wrappers
refuse before any device is touched, and PyramidFlow's geometry rule and refusals (CPU only; no compute calls here)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import pkg

P, Q, R, S = 4096, 8192, 12288, 16384          # non-NULL, aligned stand-ins for device pointers


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_declares_both(L):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dflow.h")).read()
    for name in ("dflow_pyr_down", "dflow_flow_upsample"):
        assert "int %s(" % name in header and name in L.SYMBOLS


def test_pyr_down_rejections_before_any_launch(L):
    lib = L.lib()

    def call(h=436, w=1024, in1=P, in2=Q, out1=R, out2=S):
        return lib.dflow_pyr_down(h, w, in1, in2, out1, out2, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"h": -1}, b"size"),
                    ({"in1": None}, b"d_in1"), ({"out1": None}, b"d_out1"),
                    ({"in2": None}, b"both"), ({"out2": None}, b"both"), ({"in1": None, "in2": None, "out2": None}, b"d_in1"),
                    ({"in1": P + 1}, b"d_in1"), ({"in1": P + 2}, b"d_in1"), ({"in2": Q + 3}, b"d_in2"), ({"out1": R + 2}, b"d_out1"),
                    ({"out2": S + 1}, b"d_out2"),
                    ({"out1": P}, b"same plane"), ({"out1": Q}, b"same plane"), ({"out2": P}, b"same plane"), ({"out2": Q}, b"same plane"),
                    ({"out2": R}, b"same plane"), ({"in2": None, "out2": None, "out1": P}, b"same plane")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(h=9000) == -1 and b"dflow_pyr_down" in lib.dflow_last_error(), "the error names the function"


def test_flow_upsample_rejections_before_any_launch(L):
    lib = L.lib()

    def call(h=436, w=1024, coarse=P, layout=0, out=Q, counts=None):
        return lib.dflow_flow_upsample(h, w, coarse, layout, out, counts, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"w": -5}, b"size"),
                    ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
                    ({"coarse": None}, b"d_coarse"), ({"out": None}, b"d_out"),
                    ({"coarse": P + 2}, b"d_coarse"), ({"out": Q + 1}, b"d_out"), ({"counts": R + 2}, b"d_counts"),
                    ({"out": P}, b"same plane"), ({"counts": P}, b"same plane"), ({"counts": Q}, b"same plane")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(layout=7) == -1 and b"dflow_flow_upsample" in lib.dflow_last_error()


def test_python_wrappers_check_their_arrays_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    img = np.zeros((40, 48, 3), np.uint8)
    for bad in (img.astype(np.float32), img[..., :2], img[0]):
        with pytest.raises(ValueError, match="pyr_down: img1 must be uint8"):
            pipeline.pyr_down(bad)
    for bad in (img[:39], img[:, :47], img.astype(np.int8)):
        with pytest.raises(ValueError, match="pyr_down: img2 must be uint8"):
            pipeline.pyr_down(img, bad)
    flow = np.zeros((20, 24, 2), np.float32)
    for size in ((40, 48), (39, 47), (40, 47)):
        for bad in (flow.astype(np.float64), flow[0], np.zeros((20, 24, 4), np.float32), np.zeros((21, 24, 2), np.float32),
                    np.zeros((20, 25, 3), np.float32)):
            with pytest.raises(ValueError, match="flow_upsample: flow must be float32"):
                pipeline.flow_upsample(bad, size)
    with pytest.raises(ValueError, match="flow_upsample: flow must be float32"):
        pipeline.flow_upsample(flow, (41, 48))            # 41 rows have a 21-row level above them
    with pytest.raises(ValueError, match="flow_upsample: size"):
        pipeline.flow_upsample(flow, (0, 48))


def test_the_geometry_rule(L):
    levels = pkg("pipeline").pyramid_levels
    # half the size (rounded up) per level, the same cells in pixels: the reach in pixels of the full frame doubles
    assert levels(436, 1024, 3) == [dict(pich=436, picw=1024, cellh=27, cellw=64), dict(pich=218, picw=512, cellh=27, cellw=64),
                                    dict(pich=109, picw=256, cellh=27, cellw=64)]
    assert levels(45, 35, 2, 9, 7) == [dict(pich=45, picw=35, cellh=9, cellw=7), dict(pich=23, picw=18, cellh=9, cellw=7)]
    assert levels(40, 48, 1, 5, 6) == [dict(pich=40, picw=48, cellh=5, cellw=6)]
    # a cell larger than a coarse image is clipped to it
    assert levels(64, 40, 3, 16, 16)[1:] == [dict(pich=32, picw=20, cellh=16, cellw=16), dict(pich=16, picw=10, cellh=16, cellw=10)]
    # window: the coarse levels keep what was given, level 0 takes fine_window
    got = levels(40, 48, 3, 5, 6, fine_window=0, window=1, maxnprop=80)
    assert [g["window"] for g in got] == [0, 1, 1] and all(g["maxnprop"] == 80 for g in got)
    got = levels(40, 48, 2, 5, 6, fine_window=1)
    assert got[0]["window"] == 1 and "window" not in got[1]
    assert "window" not in levels(40, 48, 2, 5, 6)[0]


def test_refused_levels_are_named(L):
    levels = pkg("pipeline").pyramid_levels
    with pytest.raises(ValueError, match=r"level 3 \(6x5.*image size"):
        levels(40, 48, 4, 5, 6)                          # 40x48 -> 20x24 -> 10x12 -> 5x6: below 8 px
    assert len(levels(40, 48, 3, 5, 6)) == 3
    with pytest.raises(ValueError, match=r"level 0 .*fewer than knn"):
        levels(436, 1024, 2, 1, 4)
    with pytest.raises(ValueError, match=r"level 0 .*window=3"):
        levels(40, 48, 2, 5, 6, fine_window=3)
    with pytest.raises(ValueError, match=r"level 0 .*window=-1"):
        levels(40, 48, 2, 5, 6, window=-1)
    with pytest.raises(ValueError, match=r"level 1 .*window=3"):
        levels(40, 48, 2, 5, 6, fine_window=2, window=3)
    with pytest.raises(ValueError, match="levels must be >= 1"):
        levels(40, 48, 0, 5, 6)
    # the constructor refuses before it looks for a device
    with pytest.raises(ValueError, match="level 3"):
        pkg("pipeline").PyramidFlow(40, 48, 4, 5, 6)
