"""What dflow_frame_interp refuses on the host, before anything is launched, what pipeline.frame_interp and frame_sequence
refuse before any device is touched and what they hand to the library, and what midframe.py and run_batch.py --midframe refuse
(CPU only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

B1, B2, FWD, BWD, OUT, KEYS, MOT, TMP, SRC, CNT = (4096 * k for k in range(1, 11))   # non-NULL, aligned stand-ins for device pointers
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_the_binding_and_the_makefile_name_it(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "int dflow_frame_interp(" in header and "dflow_frame_interp" in L.SYMBOLS
    makefile = open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert "frame_interp.hip" in makefile
    assert hasattr(C.CDLL(L.LIB_PATH), "dflow_frame_interp")
    # no workspace: the scratch is the caller's typed planes, and the binding holds no size_t
    restype, argtypes = L._SIGNATURES["dflow_frame_interp"]
    assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == 19
    proto = re.search(r"int dflow_frame_interp\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert "size_t" not in proto and "d_ws" not in proto and len(proto.split(",")) == len(argtypes)
    # the one copy of the sample and the error lives in plane_ops.h
    csrc = os.path.join(ROOT, PKG, "csrc")
    assert "bgr_bilinear(" in open(os.path.join(csrc, "plane_ops.h")).read()
    for name in ("flow_picture.hip", "frame_interp.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "bgr_bilinear(" in text and "bgr_mean_abs_diff(" in text and "(1.0f - ax)" not in text, name


def test_rejections_before_any_launch(L):
    lib = L.lib()

    def call(h=436, w=1024, b1=B1, b2=B2, fwd=FWD, lf=0, bwd=BWD, lb=1, t=0.5, rounds=8, occl=30.0, flags=0, out=OUT, keys=KEYS,
             mot=MOT, tmp=TMP, src=SRC, cnt=CNT):
        return lib.dflow_frame_interp(h, w, b1, b2, fwd, lf, bwd, lb, t, rounds, occl, flags, out, keys, mot, tmp, src, cnt, None)
    cases = [({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"h": -1}, b"size"),
             ({"lf": 2}, b"layout_fwd"), ({"lf": -1}, b"layout_fwd"), ({"lb": 2}, b"layout_bwd"), ({"lb": -1}, b"layout_bwd"),
             ({"t": 0.0}, b"t="), ({"t": 1.0}, b"t="), ({"t": -0.5}, b"t="), ({"t": 1.5}, b"t="), ({"t": NAN}, b"t="), ({"t": INF}, b"t="),
             ({"t": -INF}, b"t="), ({"t": 1e-46}, b"t="),                     # rounds to 0 as a float32
             ({"rounds": -1}, b"fill_rounds"), ({"rounds": 65}, b"fill_rounds"),
             ({"occl": NAN}, b"occl_thresh"), ({"occl": INF}, b"occl_thresh"), ({"occl": -INF}, b"occl_thresh"), ({"occl": -1e-30}, b"occl_thresh"),
             ({"flags": 1}, b"flags"), ({"flags": 2}, b"flags"), ({"flags": 0x80000000}, b"flags"),
             ({"b1": None}, b"d_bgr1"), ({"b2": None}, b"d_bgr2"), ({"fwd": None}, b"d_fwd"), ({"out": None}, b"d_out"),
             ({"keys": None}, b"d_keys"), ({"mot": None}, b"d_motion is NULL"), ({"tmp": None}, b"d_motion_tmp"),
             ({"tmp": None, "rounds": 1}, b"d_motion_tmp"),
             ({"keys": KEYS + 4}, b"d_keys is not 8-byte"), ({"keys": KEYS + 1}, b"d_keys"), ({"fwd": FWD + 2}, b"d_fwd"),
             ({"bwd": BWD + 1}, b"d_bwd"), ({"mot": MOT + 2}, b"d_motion "), ({"tmp": TMP + 3}, b"d_motion_tmp"),
             ({"cnt": CNT + 2}, b"d_counts")]
    ins = {"b1": (B1, b"d_bgr1"), "b2": (B2, b"d_bgr2"), "fwd": (FWD, b"d_fwd"), "bwd": (BWD, b"d_bwd")}
    outs = {"out": (OUT, b"d_out"), "keys": (KEYS, b"d_keys"), "mot": (MOT, b"d_motion"), "tmp": (TMP, b"d_motion_tmp"),
            "src": (SRC, b"d_source"), "cnt": (CNT, b"d_counts")}
    # any output equal to an input, or to another output; the message names both
    cases += [({o: p}, on + b" is the same plane as " + pn) for o, (_, on) in outs.items() for p, pn in ins.values()]
    cases += [({a: pb}, b"is the same plane as") for a in outs for b, (pb, _) in outs.items() if a != b]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    for a in outs:
        for b, (pb, nb) in outs.items():
            if a != b:
                assert call(**{a: pb}) == -1 and outs[a][1] in lib.dflow_last_error() and nb in lib.dflow_last_error()
    assert call(h=9000) == -1 and b"dflow_frame_interp" in lib.dflow_last_error(), "the error names the function"
    # forward only: layout_bwd is not looked at, the other refusals stay
    for kw, msg in (({"out": FWD}, b"d_out is the same plane as d_fwd"), ({"src": KEYS}, b"same plane"), ({"t": 1.0}, b"t="),
                    ({"keys": None}, b"d_keys")):
        assert call(**dict(dict(bwd=None, lb=7), **kw)) == -1 and msg in lib.dflow_last_error(), kw
    # the same picture as both frames is no overlap of an output
    assert call(b2=B1, out=B1) == -1 and b"d_out is the same plane as d_bgr1" in lib.dflow_last_error()


@pytest.fixture()
def recorded(L, monkeypatch):
    """pipeline's wrappers on host tensors with the library call recorded: [(name, args)]."""
    import torch
    pipeline = pkg("pipeline")
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda dev: "the stream")
    monkeypatch.setattr(pipeline, "_device_of", lambda *tensors: torch.device("cpu"))
    return calls


def test_the_wrapper_hands_over_what_it_was_given(L, recorded):
    import torch
    pipeline = pkg("pipeline")
    H, W = 6, 10
    img1, img2 = torch.zeros((H, W, 3), dtype=torch.uint8), torch.ones((H, W, 3), dtype=torch.uint8)
    fwd, bwd = torch.zeros((H, W, 2)), torch.zeros((H, W, 3))
    out = pipeline.frame_interp(img1, img2, fwd)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3)
    (name, a), = recorded
    assert name == "dflow_frame_interp" and len(a) == 19
    assert a[:8] == (H, W, img1.data_ptr(), img2.data_ptr(), fwd.data_ptr(), L.EVAL_DYDX, None, 0)
    assert a[8:12] == (0.5, 8, 30.0, 0) and a[12] == out.data_ptr() and a[16] is None and a[17] is None and a[18] == "the stream"
    assert all(isinstance(p, int) and p for p in a[13:16]) and len({a[12], a[13], a[14], a[15]}) == 4
    del recorded[:]
    ret = pipeline.frame_interp(img1, img2, bwd, fwd, t=1 / 3, fill_rounds=0, occl_thresh=0, motion=True, source=True, counts=True)
    frame, motion, source, counts = ret
    assert (frame.dtype, motion.dtype, source.dtype, counts.dtype) == (torch.uint8, torch.float32, torch.uint8, torch.int32)
    assert (tuple(motion.shape), tuple(source.shape), tuple(counts.shape)) == ((H, W, 3), (H, W), (8,))
    (name, a), = recorded
    assert a[4:8] == (bwd.data_ptr(), L.EVAL_UVV, fwd.data_ptr(), L.EVAL_DYDX)
    assert a[8] == float(np.float32(1 / 3)) and a[9:12] == (0, 0.0, 0)
    assert a[14] == motion.data_ptr() and a[15] is None, "no second motion plane without fill rounds"
    assert a[16] == source.data_ptr() and a[17] == counts.data_ptr()
    del recorded[:]
    assert len(pipeline.frame_interp(img1, img2, fwd, source=True)) == 2 and len(pipeline.frame_interp(img1, img2, fwd, counts=True)) == 2
    assert pipeline.FRAME_INTERP_COUNTS == ("from1", "from2", "filled", "unknown", "blended", "one_sided", "fallback", "lost")
    # the sequence: n calls at t = k / (n + 1) as float32, one set of scratch planes
    del recorded[:]
    frames, counts = pipeline.frame_sequence(img1, img2, fwd, bwd, n=3, fill_rounds=2, counts=True)
    assert len(frames) == 3 and len(counts) == 3 and len({f.data_ptr() for f in frames}) == 3
    assert [a[8] for _, a in recorded] == [0.25, 0.5, 0.75] and len({a[13:16] for _, a in recorded}) == 1
    assert len({a[12] for _, a in recorded}) == 3 and all(a[15] for _, a in recorded)
    assert len(pipeline.frame_sequence(img1, img2, fwd, n=2)) == 2


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    i1, f2, f3 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32)
    for fn in (pipeline.frame_interp, pipeline.frame_sequence):
        who = fn.__name__
        for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32), np.zeros((H, W, 1), np.float32)):
            with pytest.raises(ValueError, match=who + ": fwd must be float32"):
                fn(i1, i1, bad)
            with pytest.raises(ValueError, match=who + ": bwd must be float32"):
                fn(i1, i1, f3, bad)
        for bad in (f2[:19], f3[:, :23]):
            with pytest.raises(ValueError, match=who + ": bwd must be float32"):
                fn(i1, i1, f2, bad)
        for bad in (i1[:19], i1.astype(np.float32), i1[..., :2]):
            with pytest.raises(ValueError, match=who + ": img1"):
                fn(bad, i1, f2)
            with pytest.raises(ValueError, match=who + ": img2"):
                fn(i1, bad, f2)
        for rounds in (-1, 65, 1.5):
            with pytest.raises(ValueError, match=who + ": fill_rounds"):
                fn(i1, i1, f2, fill_rounds=rounds)
        for occl in (NAN, INF, -1.0):
            with pytest.raises(ValueError, match=who + ": occl_thresh"):
                fn(i1, i1, f2, occl_thresh=occl)
    for t in (0.0, 1.0, -0.25, 1.25, NAN, INF, 1e-46, 1.0 - 1e-9):         # the last two round to 0 and to 1 as float32
        with pytest.raises(ValueError, match="frame_interp: t must lie"):
            pipeline.frame_interp(i1, i1, f2, t=t)
    for n in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match="frame_sequence: n must be"):
            pipeline.frame_sequence(i1, i1, f2, n=n)


def test_command_line_refusals(L, capsys, tmp_path):
    mf = pkg("midframe")
    four = ["a.png", "b.png", "f.npy", "out.png"]
    for tail in (["--t", "0"], ["--t", "1"], ["--t", "nan"], ["--t", "0.5", "--frames", "2"], ["--frames", "0"], ["--frames", "100"],
                 ["--fill-rounds", "-1"], ["--fill-rounds", "65"], ["--occl-thresh", "-1"], ["--occl-thresh", "inf"],
                 ["--occl-thresh", "nan"], ["--frames", "2", "--source", "s.png"], ["--unknown"]):
        with pytest.raises(SystemExit) as e:
            mf.main(four + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    for short in ([], four[:3]):
        with pytest.raises(SystemExit) as e:
            mf.main(short)
        assert e.value.code == 2
    a = mf.parser().parse_args(four + ["--backward", "b.npy", "--frames", "3"])
    assert (a.backward, a.frames, a.t, a.fill_rounds, a.occl_thresh, a.source) == ("b.npy", 3, None, 8, 30.0, None)
    # inputs of different sizes: status 2 and a message, before any device is touched
    flowio = pkg("flowio")
    flowio.write_png8(str(tmp_path / "a.png"), np.zeros((6, 8, 3), np.uint8))
    flowio.write_png8(str(tmp_path / "b.png"), np.zeros((6, 8, 3), np.uint8))
    np.save(tmp_path / "f.npy", np.zeros((6, 9, 2)))
    capsys.readouterr()
    assert mf.main([str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / "f.npy"), str(tmp_path / "o.png")]) == 2
    assert "differ in size" in capsys.readouterr().err
    assert mf.count_line(0.5, range(8)) == "t=0.500000 from1=0 from2=1 filled=2 unknown=3 blended=4 one_sided=5 fallback=6 lost=7"
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert a.midframe is False and rb.midframe_args(a) == (8, 30.0)
    a = rb.parser().parse_args(["--midframe", "--mid-fill-rounds", "0", "--mid-occl-thresh", "12.5"])
    assert a.midframe is True and rb.midframe_args(a) == (0, 12.5)
    for argv in (["--mid-fill-rounds", "4"], ["--mid-occl-thresh", "3"], ["--midframe", "--mid-fill-rounds", "65"],
                 ["--midframe", "--mid-fill-rounds", "-1"], ["--midframe", "--mid-occl-thresh", "-1"],
                 ["--midframe", "--mid-occl-thresh", "nan"], ["--midframe", "--mid-occl-thresh", "inf"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--mid-" in capsys.readouterr().err, argv
    m = np.zeros((2, 2), bool)
    img = np.zeros((2, 2, 3), np.uint8)
    assert rb.psnr(img, img, m) is None and rb.psnr(img, img, ~m) == float("inf")
    assert abs(rb.psnr(img, img + 5, ~m) - 10 * np.log10(255.0 ** 2 / 25)) < 1e-12
