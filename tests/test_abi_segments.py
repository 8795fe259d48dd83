"""What dflow_segment_filter refuses on the host, before anything is launched, what its Python wrapper refuses before any device
is touched, and what the command lines refuse (CPU only; no compute calls here)."""
import os

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

H, W = 436, 1024
PLANE = 8 << 20                                           # more than any plane of an HxW frame
FLOW, OUT, SEG, SIZE, CNT, WS = (PLANE * k for k in range(1, 7))      # non-NULL, aligned, disjoint stand-ins for device pointers
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_declares_it(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "int dflow_segment_filter(" in header and "size_t dflow_segment_filter_workspace_bytes(" in header
    assert "dflow_segment_filter" in L.SYMBOLS and "dflow_segment_filter_workspace_bytes" in L.SYMBOLS
    assert "#define DFLOW_SEG_KEEP_SINGLETONS 1u" in header and L.SEG_KEEP_SINGLETONS == 1
    makefile = open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert "segments.hip" in makefile
    assert "dflow_segment_filter" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the tile, border and root steps are union_find.h's, one definition each
    import component_pins
    component_pins.check(os.path.join(ROOT, PKG, "csrc"))


def test_workspace_bytes(L):
    lib = L.lib()
    for h, w in ((0, 10), (10, 0), (8193, 10), (10, 8193), (-1, 10)):
        assert lib.dflow_segment_filter_workspace_bytes(h, w) == 0 and b"size" in lib.dflow_last_error()
    # a label and a size per pixel, each region rounded up to 256 bytes
    for h, w in ((1, 1), (45, 35), (436, 1024), (8192, 8192)):
        assert lib.dflow_segment_filter_workspace_bytes(h, w) == 2 * ((4 * h * w + 255) // 256 * 256)


def test_rejections_before_any_launch(L):
    lib = L.lib()
    need = lib.dflow_segment_filter_workspace_bytes(H, W)

    def call(h=H, w=W, flow=FLOW, layout=0, thresh=1.0, min_size=20, flags=0, out=OUT, seg=SEG, size=SIZE, cnt=CNT, ws=WS, ws_bytes=need):
        return lib.dflow_segment_filter(h, w, flow, layout, thresh, min_size, flags, out, seg, size, cnt, ws, ws_bytes, None)
    cases = [({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"h": -1}, b"size"),
             ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
             ({"flags": 2}, b"flags"), ({"flags": 3}, b"flags"), ({"flags": 0x80000000}, b"flags"),
             ({"thresh": NAN}, b"thresh"), ({"thresh": INF}, b"thresh"), ({"thresh": -INF}, b"thresh"), ({"thresh": -1e-30}, b"thresh"),
             ({"min_size": -1}, b"min_size"), ({"min_size": -2 ** 31}, b"min_size"),
             ({"flow": None}, b"d_flow"), ({"out": None}, b"d_out"),
             ({"flow": FLOW + 2}, b"d_flow"), ({"out": OUT + 1}, b"d_out"), ({"seg": SEG + 3}, b"d_segment"), ({"size": SIZE + 2}, b"d_size"),
             ({"cnt": CNT + 1}, b"d_counts"), ({"ws": WS + 2}, b"d_ws")]
    # any two planes that share a byte, but for d_out == d_flow under UVV
    ptrs = {"flow": (FLOW, b"d_flow"), "out": (OUT, b"d_out"), "seg": (SEG, b"d_segment"), "size": (SIZE, b"d_size"),
            "cnt": (CNT, b"d_counts"), "ws": (WS, b"d_ws")}
    for a in ptrs:
        for b in ptrs:
            if a != b and (a, b) != ("out", "flow") and (a, b) != ("flow", "out"):
                cases.append(({a: ptrs[b][0]}, b"overlap"))
    cases += [({"out": FLOW + 4}, b"d_flow and d_out overlap"), ({"out": FLOW - 4}, b"d_flow and d_out overlap"),
              ({"out": FLOW, "layout": 1}, b"d_flow and d_out overlap"), ({"flow": OUT, "layout": 1}, b"d_flow and d_out overlap"),
              ({"seg": OUT + 12 * H * W - 4}, b"d_out and d_segment overlap"), ({"cnt": SIZE + 4 * H * W - 4}, b"d_size and d_counts overlap"),
              ({"cnt": WS - 12}, b"d_counts and d_ws overlap"), ({"size": WS + need - 4}, b"d_size and d_ws overlap")]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(h=9000) == -1 and b"dflow_segment_filter" in lib.dflow_last_error(), "the error names the function"
    # planes that end where the next one starts do not overlap: the call gets as far as the workspace check
    for kw in ({"seg": OUT + 12 * H * W}, {"cnt": WS - 16}, {"size": WS + need}, {}, {"seg": None, "size": None, "cnt": None},
               {"out": FLOW}, {"flow": OUT}, {"min_size": 0}, {"min_size": 2 ** 31 - 1}, {"thresh": 0.0}, {"flags": 1}):
        for short in ({"ws": None}, {"ws_bytes": need - 1}, {"ws_bytes": 0}):
            assert call(**dict(kw, **short)) == -2 and b"workspace" in lib.dflow_last_error(), (kw, short, lib.dflow_last_error())


def test_the_wrapper_checks_its_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    f2, f3 = np.zeros((20, 24, 2), np.float32), np.zeros((20, 24, 3), np.float32)
    for bad in (f2.astype(np.float64), f3.astype(np.float16), f2[0], np.zeros((20, 24, 4), np.float32), np.zeros((20, 24, 1), np.float32),
                np.zeros((20, 24), np.float32)):
        with pytest.raises(ValueError, match="segment_filter: flow must be float32"):
            pipeline.segment_filter(bad, 1.0, 20)
    for thresh in (NAN, INF, -INF, -1.0):
        with pytest.raises(ValueError, match="segment_filter: thresh"):
            pipeline.segment_filter(f3, thresh, 20)
    for min_size in (-1, 2 ** 31, 2.5, NAN):
        with pytest.raises(ValueError, match="segment_filter: min_size"):
            pipeline.segment_filter(f2, 1.0, min_size)


def test_command_line_refusals(L, capsys):
    spz = pkg("spremiZaEpic")
    six = ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"]
    # the three tokens are taken directly after the six positional ones (--natural-check already taken) and nowhere else
    assert spz.take_segments(six + ["--segments", "20", "1"]) == (six, (20, 1.0))
    assert spz.take_segments(six + ["--segments", "100", "2.5", "--gpu-epic", "--refine"]) == (six + ["--gpu-epic", "--refine"], (100, 2.5))
    assert spz.take_segments(six) == (six, None) and spz.take_segments(six + ["--gpu-epic"]) == (six + ["--gpu-epic"], None)
    assert spz.take_segments(spz.take_natural(six + ["--natural-check", "--segments", "0", "0"])[0]) == (six, (0, 0.0))
    for tail in (["--segments"], ["--segments", "20"], ["--segments", "20", "x"], ["--segments", "2.5", "1"], ["--segments", "-1", "1"],
                 ["--segments", "20", "-1"], ["--segments", "20", "nan"], ["--segments", "20", "inf"], ["--segments", str(2 ** 31), "1"],
                 ["--segments", "20", "--gpu-epic"], ["--segments", "20", "1", "--natural-check"], ["--gpu-epic", "--segments", "20", "1"],
                 ["--segments", "20", "1", "--segments", "20", "1"], ["--natural-check", "--gpu-epic", "--prefilter", "--segments", "20", "1"],
                 ["--segments", "20", "1", "--refine"]):
        assert spz.main(six + tail) == 2, tail
    capsys.readouterr()
    rb = pkg("run_batch")
    assert rb.parser().parse_args([]).segments is None and rb.parser().parse_args(["--segments", "20", "1"]).segments == ["20", "1"]
    assert rb.segments_arg(["20", "1"]) == (20, 1.0) and rb.segments_arg(["0", "0.5"]) == (0, 0.5)
    for tail in (["--segments"], ["--segments", "20"], ["--segments", "20", "x"], ["--segments", "2.5", "1"], ["--segments", "-1", "1"],
                 ["--segments", "20", "-1"], ["--segments", "20", "nan"], ["--segments", "20", "inf"], ["--segments", str(2 ** 31), "1"]):
        with pytest.raises(SystemExit) as e:
            rb.main(["--pairs", "1", "--size", "40x48"] + tail)
        assert e.value.code == 2, tail
    capsys.readouterr()
