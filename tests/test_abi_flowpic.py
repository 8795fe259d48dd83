"""What dflow_flow_color, dflow_warp_eval and their workspace functions refuse on the host, before anything is launched
(CPU only; no compute calls here)."""
import ctypes as C
import os

import pytest

from conftest import pkg

P = 4096                      # a non-NULL, aligned stand-in for every device pointer
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


@pytest.mark.parametrize("name", ["dflow_flow_color_workspace_bytes", "dflow_warp_eval_workspace_bytes"])
def test_workspace_sizes(L, name):
    fn = getattr(L.lib(), name)
    wsb = fn(436, 1024)
    assert wsb > 0 and fn(436, 1024) == wsb, "a fixed function of the size"
    assert 0 < fn(1, 1) <= wsb <= fn(8192, 8192) <= 1 << 20
    for h, w in ((0, 8), (8, 0), (8193, 8), (8, 8193), (-1, 8), (8, -1)):
        assert fn(h, w) == 0 and b"size" in L.lib().dflow_last_error(), (h, w)


def test_flow_color_rejections_before_any_launch(L):
    lib = L.lib()
    wsb = lib.dflow_flow_color_workspace_bytes(436, 1024)

    def call(h=436, w=1024, flow=P, layout=0, max_flow=0.0, bgr=P, maxrad=None, ws=P, ws_bytes=wsb):
        return lib.dflow_flow_color(h, w, flow, layout, max_flow, bgr, maxrad, ws, ws_bytes, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"),
                    ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
                    ({"max_flow": -1.0}, b"max_flow"), ({"max_flow": -1e-30}, b"max_flow"), ({"max_flow": NAN}, b"max_flow"),
                    ({"max_flow": INF}, b"max_flow"), ({"max_flow": -INF}, b"max_flow"),
                    ({"flow": None}, b"d_flow"), ({"bgr": None}, b"d_bgr"),
                    ({"flow": P + 4}, b"d_flow"), ({"flow": P + 8}, b"d_flow"), ({"bgr": P + 2}, b"d_bgr"),
                    ({"maxrad": P + 2}, b"d_maxrad")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    for kw in ({"ws": None}, {"ws_bytes": wsb - 1}, {"ws_bytes": 0}, {"layout": 1, "max_flow": 5.0, "maxrad": P, "ws_bytes": 8}):
        assert call(**kw) == -2 and b"workspace" in lib.dflow_last_error(), kw
    # an argument error is reported before a workspace that is too small
    assert call(h=0, ws=None) == -1 and call(max_flow=NAN, ws_bytes=0) == -1


def test_warp_eval_rejections_before_any_launch(L):
    lib = L.lib()
    assert C.sizeof(L.PhotoStats) == 48 and L.WARP_FLAG_ACCUMULATE == 1
    wsb = lib.dflow_warp_eval_workspace_bytes(436, 1024)

    def call(h=436, w=1024, bgr1=P, bgr2=P, flow=P, layout=0, thresh=10.0, emax=30.0, flags=0, stats=P, warped=None, err=None,
             err_bgr=None, ws=P, ws_bytes=wsb):
        return lib.dflow_warp_eval(h, w, bgr1, bgr2, flow, layout, thresh, emax, flags, stats, warped, err, err_bgr, ws, ws_bytes, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"),
                    ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
                    ({"thresh": NAN}, b"err_thresh"), ({"thresh": INF}, b"err_thresh"), ({"thresh": -1.0}, b"err_thresh"),
                    ({"thresh": -1e-30}, b"err_thresh"),
                    ({"emax": NAN}, b"err_max"), ({"emax": INF}, b"err_max"), ({"emax": 0.0}, b"err_max"), ({"emax": -0.0}, b"err_max"),
                    ({"emax": -30.0}, b"err_max"),
                    ({"flags": 2}, b"flags"), ({"flags": 0x80000001}, b"flags"),
                    ({"bgr1": None}, b"d_bgr1"), ({"bgr2": None}, b"d_bgr2"), ({"flow": None}, b"d_flow"), ({"stats": None}, b"d_stats"),
                    ({"bgr1": P + 1}, b"d_bgr1"), ({"flow": P + 4}, b"d_flow"), ({"stats": P + 4}, b"d_stats"),
                    ({"warped": P + 2}, b"d_warped"), ({"err": P + 4}, b"d_err"), ({"err": P + 8}, b"d_err"),
                    ({"err_bgr": P + 2}, b"d_err_bgr")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    for kw in ({"ws": None}, {"ws_bytes": wsb - 1}, {"ws_bytes": 0}, {"layout": 1, "thresh": 0.0, "flags": 1, "bgr2": P + 1, "ws_bytes": 8}):
        assert call(**kw) == -2 and b"workspace" in lib.dflow_last_error(), kw
    assert call(w=0, ws=None) == -1 and call(emax=0.0, ws_bytes=0) == -1


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    import numpy as np
    pipeline = pkg("pipeline")
    for bad in (np.zeros((4, 4, 3), np.float64), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4), np.float32)):
        with pytest.raises(ValueError, match="flow must be float32"):
            pipeline.flow_color(bad)
        with pytest.raises(ValueError, match="flow must be float32"):
            pipeline.warp_eval(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), bad)
    with pytest.raises(ValueError, match="images must be"):
        pipeline.warp_eval(np.zeros((4, 5, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError, match="images must be"):
        pipeline.warp_eval(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 2), np.float32))


def test_every_image_plane_wrapper_checks_its_arrays_before_any_cuda_use(L, monkeypatch):
    """Wrong dtype, wrong rank and wrong last dimension of every array argument of the eight image-plane wrappers: a ValueError
    that names the wrapper and the argument, raised before torch.cuda is asked for anything."""
    import numpy as np
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 4, 5
    u8, f32 = (lambda *shape: np.zeros(shape, np.uint8)), (lambda *shape: np.zeros(shape, np.float32))
    wrappers = {"canny_edges": dict(bgr=u8(H, W, 3)),
                "pb_edges": dict(bgr=u8(H, W, 3)),
                "epic_interpolate": dict(sparse=f32(H, W, 3), edges=f32(H, W)),
                "epic_prefilter": dict(sparse=f32(H, W, 3), edges=f32(H, W), img1=u8(H, W, 3)),
                "variational_refine": dict(img1=u8(H, W, 3), img2=u8(H, W, 3), flow=f32(H, W, 2)),
                "flow_eval": dict(test=f32(H, W, 3), gt=f32(H, W, 3)),
                "flow_color": dict(flow=f32(H, W, 2)),
                "warp_eval": dict(img1=u8(H, W, 3), img2=u8(H, W, 3), flow=f32(H, W, 3))}
    cases = 0
    for fn, good in wrappers.items():
        for arg, a in good.items():
            for what, bad in (("dtype", a.astype(np.float64 if a.dtype == np.float32 else np.float32)), ("rank", a[0]),
                              ("last dimension", np.concatenate([a, a], axis=-1))):
                with pytest.raises(ValueError) as ei:
                    getattr(pipeline, fn)(**dict(good, **{arg: bad}))
                assert fn in str(ei.value) and arg in str(ei.value), (fn, arg, what, str(ei.value))
                cases += 1
    assert cases == 3 * 16
