"""What dflow_flow_wmedian refuses on the host, before anything is launched, what pipeline.flow_wmedian and wmedian_tables
refuse before any device is touched and what the wrapper hands to the library, and what flowfilter.py and run_batch.py
--wmedian / --wmedian-reject refuse (CPU only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FLOW, BGR, WS, WC, OUT, CNT = (4096 * k for k in range(1, 7))          # non-NULL, aligned stand-ins for device pointers
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_the_binding_and_the_makefile_name_it(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "int dflow_flow_wmedian(" in header and "dflow_flow_wmedian" in L.SYMBOLS
    assert "flow_wmedian.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert hasattr(C.CDLL(L.LIB_PATH), "dflow_flow_wmedian")
    assert "#define DFLOW_WMED_KEEP_HOLES 1u" in header and L.WMED_KEEP_HOLES == 1
    assert "#define DFLOW_WMED_REJECT 2u" in header and L.WMED_REJECT == 2
    # no workspace: the binding holds no size_t, and it is as long as the prototype
    restype, argtypes = L._SIGNATURES["dflow_flow_wmedian"]
    assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == 13
    proto = re.search(r"int dflow_flow_wmedian\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto) and len(proto.split(",")) == len(argtypes)
    # the kernel shares plane_ops.h's helpers and the one definition of a good vector
    text = open(os.path.join(ROOT, PKG, "csrc", "flow_wmedian.hip")).read()
    assert '#include "plane_ops.h"' in text and "block_count<4>(" in text and "flow_good(" in text


def test_rejections_before_any_launch(L):
    lib = L.lib()

    def call(h=436, w=1024, flow=FLOW, layout=0, bgr=BGR, radius=3, ws=WS, wc=WC, thresh=1.0, flags=0, out=OUT, cnt=CNT):
        return lib.dflow_flow_wmedian(h, w, flow, layout, bgr, radius, ws, wc, thresh, flags, out, cnt, None)
    cases = [({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"h": -1}, b"size"),
             ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
             ({"radius": 0}, b"radius"), ({"radius": 9}, b"radius"), ({"radius": -3}, b"radius"),
             ({"flags": 4}, b"flags"), ({"flags": 7}, b"flags"), ({"flags": 0x80000000}, b"flags"),
             ({"flags": 2, "thresh": NAN}, b"reject_thresh"), ({"flags": 2, "thresh": INF}, b"reject_thresh"),
             ({"flags": 3, "thresh": -INF}, b"reject_thresh"), ({"flags": 2, "thresh": -1e-30}, b"reject_thresh"),
             ({"flow": None}, b"d_flow"), ({"out": None}, b"d_out"),
             ({"bgr": None}, b"d_bgr and d_wcolor"), ({"wc": None}, b"d_bgr and d_wcolor"),
             ({"flow": FLOW + 2}, b"d_flow"), ({"out": OUT + 1}, b"d_out"), ({"cnt": CNT + 2}, b"d_counts"),
             ({"out": FLOW}, b"d_out is the same plane as d_flow"), ({"out": BGR}, b"d_out is the same plane as d_bgr"),
             ({"out": WS}, b"d_out is the same plane as d_wspace"), ({"out": WC}, b"d_out is the same plane as d_wcolor"),
             ({"cnt": FLOW}, b"d_counts is the same plane as d_flow"), ({"cnt": BGR}, b"d_counts is the same plane as d_bgr"),
             ({"cnt": WS}, b"d_counts is the same plane as d_wspace"), ({"cnt": WC}, b"d_counts is the same plane as d_wcolor"),
             ({"cnt": OUT}, b"d_counts is the same plane as d_out")]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(h=9000) == -1 and b"dflow_flow_wmedian" in lib.dflow_last_error(), "the error names the function"
    # unguided: the same refusals; reject_thresh is looked at only under DFLOW_WMED_REJECT
    for kw, msg in (({"out": FLOW}, b"d_out is the same plane as d_flow"), ({"radius": 9}, b"radius"),
                    ({"flags": 2, "thresh": NAN}, b"reject_thresh"), ({"bgr": None, "wc": WC}, b"d_bgr and d_wcolor")):
        assert call(**dict(dict(bgr=None, wc=None, ws=None, cnt=None), **kw)) == -1 and msg in lib.dflow_last_error(), kw
    # a bad threshold without the flag is not looked at: the next refusal in line is reported instead
    assert call(thresh=NAN, flags=1, out=None) == -1 and b"d_out" in lib.dflow_last_error()


def test_the_tables():
    pipeline = pkg("pipeline")
    assert pipeline.wmedian_tables(3) == (None, None)
    for radius in (1, 3, 8):
        for ss, sc in ((0.5, 1.0), (2.0, 10.0), (100.0, 1000.0)):
            space, color = pipeline.wmedian_tables(radius, ss, sc)
            assert space.dtype == np.uint8 and space.shape == (radius + 1, radius + 1) and color.dtype == np.uint8 and color.shape == (766,)
            assert space[0, 0] == 255 and color[0] == 255
            assert (np.diff(space.astype(int), axis=0) <= 0).all() and (np.diff(space.astype(int), axis=1) <= 0).all()
            assert (np.diff(color.astype(int)) <= 0).all() and (space == space.T).all()
            for dy, dx in ((0, 1), (1, 1), (radius, radius), (radius, 0)):
                assert abs(int(space[dy, dx]) - 255.0 * np.exp(-(dy * dy + dx * dx) / (2.0 * ss * ss))) <= 1
            for d in (1, 7, 30, 100, 765):
                assert abs(int(color[d]) - 255.0 * np.exp(-d / (3.0 * sc))) <= 1
    space, color = pipeline.wmedian_tables(2, None, 10.0)
    assert space is None and color[30] == 94                              # 255 / e = 93.8
    assert pipeline.wmedian_tables(2, 1.0, None)[1] is None
    for bad in (0.0, -1.0, NAN, INF, -INF, "3"):
        with pytest.raises(ValueError, match="wmedian_tables: sigma_space"):
            pipeline.wmedian_tables(3, bad, 10.0)
        with pytest.raises(ValueError, match="wmedian_tables: sigma_color"):
            pipeline.wmedian_tables(3, None, bad)
    for bad in (0, 9, -1, 2.0):
        with pytest.raises(ValueError, match="wmedian_tables: radius"):
            pipeline.wmedian_tables(bad)


@pytest.fixture()
def recorded(L, monkeypatch):
    """pipeline's wrapper on host tensors with the library call recorded: [(name, args)]."""
    import torch
    pipeline = pkg("pipeline")
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda dev: "the stream")
    monkeypatch.setattr(pipeline, "_device_of", lambda *tensors: torch.device("cpu"))
    monkeypatch.setattr(pipeline, "_wmedian_uploaded", {})
    return calls


def test_the_wrapper_hands_over_what_it_was_given(L, recorded):
    import torch
    pipeline = pkg("pipeline")
    H, W = 6, 10
    img, f2, f3 = torch.zeros((H, W, 3), dtype=torch.uint8), torch.zeros((H, W, 2)), torch.zeros((H, W, 3))
    out = pipeline.flow_wmedian(f2)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (H, W, 3)
    (name, a), = recorded
    assert name == "dflow_flow_wmedian" and len(a) == 13
    assert a == (H, W, f2.data_ptr(), L.EVAL_DYDX, None, 3, None, None, 0.0, 0, out.data_ptr(), None, "the stream")
    # guided, the default sigmas: no space table, the colour table of sigma 10; the tables are uploaded once
    del recorded[:]
    out, cnt = pipeline.flow_wmedian(f3, img, radius=5, counts=True)
    (name, a), = recorded
    assert a[:6] == (H, W, f3.data_ptr(), L.EVAL_UVV, img.data_ptr(), 5) and a[6] is None and isinstance(a[7], int) and a[7]
    assert a[8:10] == (0.0, 0) and a[10] == out.data_ptr() and a[11] == cnt.data_ptr() and cnt.dtype == torch.int32 and tuple(cnt.shape) == (4,)
    uploaded = lambda: [v for k, v in pipeline._wmedian_uploaded.items() if k[1] == 5]
    (dspace, dcolor), = uploaded()
    assert dspace is None and dcolor.data_ptr() == a[7] and (dcolor.numpy() == pipeline.wmedian_tables(5, None, 10.0)[1]).all()
    pipeline.flow_wmedian(f3, img, radius=5, sigma_color=10.0)
    assert recorded[1][1][7] == a[7] and len(uploaded()) == 1, "a repeated call uploads nothing"
    pipeline.flow_wmedian(f3, img, radius=5, sigma_space=2.0)
    assert len(uploaded()) == 2 and recorded[2][1][6] is not None
    # the flags and the threshold
    del recorded[:]
    pipeline.flow_wmedian(f3, img, keep_holes=True)
    pipeline.flow_wmedian(f3, img, reject=1.5)
    pipeline.flow_wmedian(f3, img, reject=0, keep_holes=True)
    assert [a[8:10] for _, a in recorded] == [(0.0, L.WMED_KEEP_HOLES), (1.5, L.WMED_REJECT), (0.0, L.WMED_KEEP_HOLES | L.WMED_REJECT)]
    # iterations ping-pong between two buffers; from the second pass on the input is the previous output, in UVV layout
    del recorded[:]
    out, cnt = pipeline.flow_wmedian(f2, None, radius=1, iterations=4, counts=True)
    assert len(recorded) == 4
    ins, lays, outs = ([a[i] for _, a in recorded] for i in (2, 3, 10))
    assert ins[0] == f2.data_ptr() and lays == [L.EVAL_DYDX] + [L.EVAL_UVV] * 3 and ins[1:] == outs[:3]
    assert outs[0] == outs[2] and outs[1] == outs[3] and outs[0] != outs[1] and out.data_ptr() == outs[3]
    assert all(a[11] == cnt.data_ptr() for _, a in recorded)
    # tables=(space, color) overrides the sigmas; unguided drops the colour table
    del recorded[:]
    space, color = np.full((2, 2), 7, np.uint8), np.arange(766).astype(np.uint8)
    pipeline.flow_wmedian(f3, img, radius=1, sigma_space=3.0, tables=(space, color))
    pipeline.flow_wmedian(f3, None, radius=1, tables=(space, color))
    key_sets = [k for k in pipeline._wmedian_uploaded if k[1] == 1 and k[2] == space.tobytes()]
    assert len(key_sets) == 2 and recorded[1][1][7] is None and recorded[1][1][4] is None and recorded[0][1][7] is not None
    assert pipeline.FLOW_WMEDIAN_COUNTS == ("good", "valid", "filled", "altered")


def test_the_wrapper_checks_its_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    img, f2, f3 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32), np.zeros((H, W, 1), np.float32)):
        with pytest.raises(ValueError, match="flow_wmedian: flow must be float32"):
            pipeline.flow_wmedian(bad)
    for bad in (img[:19], img.astype(np.float32), img[..., :2], img[:, :23]):
        with pytest.raises(ValueError, match="flow_wmedian: img"):
            pipeline.flow_wmedian(f3, bad)
    for radius in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="flow_wmedian: radius"):
            pipeline.flow_wmedian(f2, radius=radius)
    for n in (0, 17, -1, 1.5):
        with pytest.raises(ValueError, match="flow_wmedian: iterations"):
            pipeline.flow_wmedian(f2, iterations=n)
    for t in (NAN, INF, -1.0):
        with pytest.raises(ValueError, match="flow_wmedian: reject must"):
            pipeline.flow_wmedian(f2, reject=t)
    with pytest.raises(ValueError, match="flow_wmedian: reject cannot be combined"):
        pipeline.flow_wmedian(f2, reject=1.0, iterations=2)
    with pytest.raises(ValueError, match="wmedian_tables: sigma_space"):
        pipeline.flow_wmedian(f2, sigma_space=0.0)
    with pytest.raises(ValueError, match="wmedian_tables: sigma_color"):
        pipeline.flow_wmedian(f2, img, sigma_color=NAN)
    for tables in ((np.zeros((4, 4), np.uint8),), (np.zeros((3, 3), np.uint8), None), (np.zeros((4, 4), np.float32), None),
                   (None, np.zeros(765, np.uint8)), "ab"):
        with pytest.raises(ValueError, match="flow_wmedian: "):
            pipeline.flow_wmedian(f2, img, radius=3, tables=tables)


def test_command_line_refusals(L, capsys, tmp_path):
    ff = pkg("flowfilter")
    two = ["f.npy", "o.flo"]
    for tail in (["--radius", "0"], ["--radius", "9"], ["--sigma-space", "0"], ["--sigma-space", "nan"], ["--sigma-color", "-1"],
                 ["--sigma-color", "inf"], ["--iterations", "0"], ["--iterations", "17"], ["--reject", "-1"], ["--reject", "nan"],
                 ["--reject", "inf"], ["--reject", "1", "--iterations", "2"], ["--radius", "x"], ["--unknown"]):
        with pytest.raises(SystemExit) as e:
            ff.main(two + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    for argv in ([], ["f.npy"], ["f.npy", "o.png"]):
        with pytest.raises(SystemExit) as e:
            ff.main(argv)
        assert e.value.code == 2
    a = ff.parser().parse_args(two + ["--image", "i.png", "--keep-holes", "--counts"])
    assert (a.image, a.radius, a.sigma_space, a.sigma_color, a.iterations, a.keep_holes, a.reject, a.counts) == \
        ("i.png", 3, None, 10.0, 1, True, None, True)
    # unreadable input and inputs of different sizes: status 2 and a message, before any device is touched
    flowio = pkg("flowio")
    flowio.write_png8(str(tmp_path / "i.png"), np.zeros((6, 8, 3), np.uint8))
    np.save(tmp_path / "f.npy", np.zeros((6, 9, 2)))
    np.save(tmp_path / "g.npy", np.zeros((6, 9)))
    capsys.readouterr()
    assert ff.main([str(tmp_path / "f.npy"), str(tmp_path / "o.flo"), "--image", str(tmp_path / "i.png")]) == 2
    assert "the flow is 9x6 and the image 8x6" in capsys.readouterr().err
    assert ff.main([str(tmp_path / "g.npy"), str(tmp_path / "o.flo")]) == 2 and "expected an (H,W,2)" in capsys.readouterr().err
    assert ff.main([str(tmp_path / "missing.flo"), str(tmp_path / "o.flo")]) == 2 and "flowfilter:" in capsys.readouterr().err
    assert ff.main([str(tmp_path / "f.txt"), str(tmp_path / "o.flo")]) == 2 and "unsupported flow file" in capsys.readouterr().err
    flowio.write_flo(str(tmp_path / "f.flo"), np.arange(24, dtype=np.float32).reshape(3, 4, 2))
    assert (flowio.read_flow(str(tmp_path / "f.flo")) == np.arange(24, dtype=np.float32).reshape(3, 4, 2)).all()
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert a.wmedian is None and a.wmedian_reject is None
    assert rb.wmedian_arg("3") == 3 and rb.wmedian_reject_arg(["8", "0.5"]) == (8, 0.5)
    for argv in (["--wmedian", "0"], ["--wmedian", "9"], ["--wmedian", "x"], ["--wmedian", "1.5"], ["--wmedian-reject", "0", "1"],
                 ["--wmedian-reject", "9", "1"], ["--wmedian-reject", "3", "-1"], ["--wmedian-reject", "3", "nan"],
                 ["--wmedian-reject", "3", "inf"], ["--wmedian-reject", "3"], ["--wmedian-reject", "a", "1"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--wmedian" in capsys.readouterr().err, argv
