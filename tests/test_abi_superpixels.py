"""What dflow_superpixels and dflow_segment_fit refuse on the host, before anything is launched, each with its status and its
text (the formats of abi.hip's shared checks, in the order the header states); what pipeline.superpixels, segment_fit and
superpixel_flow refuse before any device is touched and what they hand to the library; and what superpixels.py refuses (CPU only;
no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

# non-NULL, aligned stand-ins
BGR, LABEL, CENTERS, SLIC, CNT, SUMS, COMP, SIZE, FINAL, SCAN = (4096 * k for k in range(1, 11))
FLOW, MODELS, SEGC, OUT, CLS, ACC = (4096 * k for k in range(11, 17))
NAN, INF = float("nan"), float("inf")
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_the_binding_and_the_makefile_name_them(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    csrc = os.path.join(ROOT, PKG, "csrc")
    assert "superpixels.hip" in open(os.path.join(csrc, "Makefile")).read()
    # a table of its own: the key sets of the others are pinned by the tests that cover them
    assert list(L._SIGNATURES_SUPERPIXELS) == ["dflow_superpixels", "dflow_segment_fit"]
    others = set(L._SIGNATURES) | set(L._SIGNATURES_SHARED_GATE) | set(L._SIGNATURES_TRACKS) | set(L._SIGNATURES_EPIPOLAR)
    assert not set(L._SIGNATURES_SUPERPIXELS) & others
    assert "#define DFLOW_SEGMENTS_MAX 67108864" in header and L.SEGMENTS_MAX == 67108864 == 1 << 26
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("dflow_superpixels", 18), ("dflow_segment_fit", 16)):
        assert "int %s(" % name in header and name in L.SYMBOLS and hasattr(C.CDLL(L.LIB_PATH), name)
        # no workspace: the binding holds no size_t, and it is as long as the prototype
        restype, argtypes = L._SIGNATURES_SUPERPIXELS[name]
        assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == nargs
        proto = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto) and len(proto.split(",")) == nargs
    # the header's limits, its alignment lines and its launch counts
    block = header[header.index("/* Superpixels (DESIGN.md"):header.index("int dflow_superpixels(")]
    for words in ("step outside [4,64]", "compactness outside [0,255]", "iters outside [1,32]", "min_size outside [0,67108864]",
                  "checked in this order", "8 + 2 iters launches", "There is no d_ws", "D' < 2^12 * 2^26 + 2^16 *\n *     2^25 < 2^42"):
        assert words in block, words
    block = header[header.index("/* A robust affine flow model per segment"):header.index("int dflow_segment_fit(")]
    for words in ("n_seg outside\n * [1,67108864]", "rounds outside [1,6]", "checked in this order", "2 rounds + 1 launches", "There is no d_ws"):
        assert words in block, words
    assert "dflow_superpixels           d_label, d_centers, d_slic, d_counts, d_sums, d_comp, d_size, d_final, d_scan 4; d_bgr 1" in header
    assert "dflow_segment_fit           d_acc 8; d_flow, d_label, d_models, d_seg_counts, d_out, d_counts 4; d_class 1" in header
    # the gates add no refusal text of their own to abi.hip, and segments.hip is left alone
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("int dflow_superpixels("):abi.index("int dflow_remove_small_segments_host(")]
    assert "launch_superpixels(" in gate and "int dflow_segment_fit(" in gate and "launch_segment_fit(" in gate
    assert "dflow_set_error(" not in gate
    text = open(os.path.join(csrc, "superpixels.hip")).read()
    assert '#include "union_find.h"' in text and "superpixel" not in open(os.path.join(csrc, "segments.hip")).read()
    # and the labelling steps, the leader loop, the rank and the scan the two share are one definition each, in the headers
    import component_pins
    component_pins.check(csrc)
    # what they and the accumulation do inside a wave is wave_ops.h's
    import wave_ops_pins
    wave_ops_pins.check(csrc)
    # the segment fit's affine solve is the motion fit's step E: one definition, shared
    import fit_common_pins
    fit_common_pins.check(csrc)
    assert "fit_affine_from_sums(S, a.w, a.h, m)" in text and "fit_affine_from_sums(S, a.w, a.h," in open(os.path.join(csrc, "motion_fit.hip")).read()
    # the staged block of centres covers a tile and its neighbours at the smallest step
    tw, th, smin = (int(re.search(r"#define %s (\d+)" % n, text).group(1)) for n in ("SP_TW", "SP_TH", "SP_MIN_STEP"))
    assert smin == 4 and tw * th == 256 and "#define SP_LCW ((SP_TW - 1) / SP_MIN_STEP + 4)" in text
    for S in range(4, 65):
        for x0 in range(0, 8192, tw):
            assert (x0 + tw - 1) // S - x0 // S + 3 <= (tw - 1) // smin + 4


def test_superpixels_rejections_before_any_launch_status_text_and_order(L):
    lib = L.lib()

    def call(h=436, w=1024, bgr=BGR, step=16, m=10, iters=10, min_size=64, flags=0, label=LABEL, centers=CENTERS, slic=SLIC, cnt=CNT,
             sums=SUMS, comp=COMP, size=SIZE, final=FINAL, scan=SCAN):
        return lib.dflow_superpixels(h, w, bgr, step, m, iters, min_size, flags, label, centers, slic, cnt, sums, comp, size, final, scan,
                                     None)
    fn = "dflow_superpixels: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"h": -1}, "image size 1024x-1 outside [1,8192]"),
             ({"step": 3}, "step=3 outside [4,64]"), ({"step": 65}, "step=65 outside [4,64]"),
             ({"m": -1}, "compactness=-1 outside [0,255]"), ({"m": 256}, "compactness=256 outside [0,255]"),
             ({"iters": 0}, "iters=0 outside [1,32]"), ({"iters": 33}, "iters=33 outside [1,32]"),
             ({"min_size": -1}, "min_size=-1 outside [0,67108864]"), ({"min_size": (1 << 26) + 1}, "min_size=67108865 outside [0,67108864]"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"bgr": None}, "d_bgr is NULL"), ({"label": None}, "d_label is NULL"), ({"centers": None}, "d_centers is NULL"),
             ({"sums": None}, "d_sums is NULL"), ({"comp": None}, "d_comp is NULL"), ({"size": None}, "d_size is NULL"),
             ({"final": None}, "d_final is NULL"), ({"scan": None}, "d_scan is NULL"),
             ({"label": LABEL + 2}, "d_label is not 4-byte aligned"), ({"centers": CENTERS + 1}, "d_centers is not 4-byte aligned"),
             ({"slic": SLIC + 3}, "d_slic is not 4-byte aligned"), ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned"),
             ({"sums": SUMS + 1}, "d_sums is not 4-byte aligned"), ({"comp": COMP + 2}, "d_comp is not 4-byte aligned"),
             ({"size": SIZE + 3}, "d_size is not 4-byte aligned"), ({"final": FINAL + 1}, "d_final is not 4-byte aligned"),
             ({"scan": SCAN + 2}, "d_scan is not 4-byte aligned")]
    planes = [("d_bgr", "bgr", BGR), ("d_label", "label", LABEL), ("d_centers", "centers", CENTERS), ("d_slic", "slic", SLIC),
              ("d_counts", "cnt", CNT), ("d_sums", "sums", SUMS), ("d_comp", "comp", COMP), ("d_size", "size", SIZE),
              ("d_final", "final", FINAL), ("d_scan", "scan", SCAN)]
    for i, (name, kw, _) in enumerate(planes[1:], 1):
        cases += [({kw: p}, "%s is the same plane as %s" % (name, before)) for before, _, p in planes[:i]]
    assert len(cases) == 30 + sum(range(1, 10))
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    # the order: faults i .. n answer as fault i alone
    order = [{"h": 0}, {"step": 0}, {"m": 999}, {"iters": 0}, {"min_size": -5}, {"flags": 8}, {"bgr": None}, {"label": None},
             {"centers": None}, {"sums": None}, {"comp": None}, {"size": None}, {"final": None}, {"scan": None}, {"label": LABEL + 1},
             {"scan": SCAN + 1}, {"centers": BGR}, {"cnt": SLIC}]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)                       # an earlier entry of `order` overrides a later one's use of the same argument
        assert call(**kw) == EINVAL
        together = lib.dflow_last_error().decode()
        assert call(**order[i]) == EINVAL and lib.dflow_last_error().decode() == together, (i, kw, together)
    # the image needs no alignment, optional planes left out pass, and the ends of the ranges pass: the next refusal answers
    assert call(bgr=BGR + 1, slic=None, cnt=None, scan=None) == EINVAL and b"d_scan is NULL" in lib.dflow_last_error()
    assert call(h=1, w=1, step=4, m=0, iters=1, min_size=0, scan=None) == EINVAL and b"d_scan is NULL" in lib.dflow_last_error()
    assert call(h=8192, w=8192, step=64, m=255, iters=32, min_size=1 << 26, scan=None) == EINVAL and b"d_scan is NULL" in lib.dflow_last_error()


def test_segment_fit_rejections_before_any_launch_status_text_and_order(L):
    lib = L.lib()

    def call(h=436, w=1024, flow=FLOW, layout=0, label=LABEL, n_seg=1000, thresh=1.0, rounds=3, flags=0, models=MODELS, segc=SEGC, out=OUT,
             cls=CLS, cnt=CNT, acc=ACC):
        return lib.dflow_segment_fit(h, w, flow, layout, label, n_seg, thresh, rounds, flags, models, segc, out, cls, cnt, acc, None)
    fn = "dflow_segment_fit: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"layout": 2}, "unknown layout 2"), ({"layout": -1}, "unknown layout -1"),
             ({"n_seg": 0}, "n_seg=0 outside [1,67108864]"), ({"n_seg": (1 << 26) + 1}, "n_seg=67108865 outside [1,67108864]"),
             ({"thresh": 0.0}, "thresh=0 must be finite and > 0"), ({"thresh": -1.0}, "thresh=-1 must be finite and > 0"),
             ({"thresh": NAN}, "thresh=nan must be finite and > 0"), ({"thresh": INF}, "thresh=inf must be finite and > 0"),
             ({"rounds": 0}, "rounds=0 outside [1,6]"), ({"rounds": 7}, "rounds=7 outside [1,6]"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"flow": None}, "d_flow is NULL"), ({"label": None}, "d_label is NULL"), ({"models": None}, "d_models is NULL"),
             ({"segc": None}, "d_seg_counts is NULL"), ({"acc": None}, "d_acc is NULL"),
             ({"acc": ACC + 4}, "d_acc is not 8-byte aligned"), ({"flow": FLOW + 2}, "d_flow is not 4-byte aligned"),
             ({"label": LABEL + 1}, "d_label is not 4-byte aligned"), ({"models": MODELS + 2}, "d_models is not 4-byte aligned"),
             ({"segc": SEGC + 3}, "d_seg_counts is not 4-byte aligned"), ({"out": OUT + 1}, "d_out is not 4-byte aligned"),
             ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_flow", "flow", FLOW), ("d_label", "label", LABEL), ("d_models", "models", MODELS), ("d_seg_counts", "segc", SEGC),
              ("d_out", "out", OUT), ("d_class", "cls", CLS), ("d_counts", "cnt", CNT), ("d_acc", "acc", ACC)]
    for i, (name, kw, _) in enumerate(planes[2:], 2):
        cases += [({kw: p}, "%s is the same plane as %s" % (name, before)) for before, _, p in planes[:i]]
    assert len(cases) == 26 + sum(range(2, 8))
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    order = [{"h": 0}, {"layout": 9}, {"n_seg": 0}, {"thresh": NAN}, {"rounds": 0}, {"flags": 8}, {"flow": None}, {"label": None},
             {"models": None}, {"segc": None}, {"acc": None}, {"acc": ACC + 4}, {"flow": FLOW + 1}, {"cnt": CNT + 1}, {"models": FLOW},
             {"cnt": OUT}]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL
        together = lib.dflow_last_error().decode()
        assert call(**order[i]) == EINVAL and lib.dflow_last_error().decode() == together, (i, kw, together)
    # the class plane needs no alignment, optional planes left out pass, the ends of the ranges pass: the next refusal answers
    assert call(cls=CLS + 3, cnt=OUT) == EINVAL and lib.dflow_last_error().decode() == fn + "d_counts is the same plane as d_out"
    assert call(out=None, cls=None, cnt=None, acc=None) == EINVAL and b"d_acc is NULL" in lib.dflow_last_error()
    assert call(n_seg=1 << 26, rounds=6, thresh=1e-30, layout=1, acc=None) == EINVAL and b"d_acc is NULL" in lib.dflow_last_error()
    assert call(n_seg=1, rounds=1, thresh=3e38, acc=None) == EINVAL and b"d_acc is NULL" in lib.dflow_last_error()


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


def test_the_wrappers_hand_over_what_they_were_given(L, recorded):
    import torch
    pipeline = pkg("pipeline")
    H, W = 20, 37
    img = torch.zeros((H, W, 3), dtype=torch.uint8)
    lab = pipeline.superpixels(img)
    assert isinstance(lab, torch.Tensor) and lab.dtype == torch.int32 and tuple(lab.shape) == (H, W)
    (name, a), = recorded
    assert name == "dflow_superpixels" and len(a) == 18
    assert a[:8] == (H, W, img.data_ptr(), 16, 10, 10, 64, 0) and a[8] == lab.data_ptr() and a[10:12] == (None, None) and a[17] == "the stream"
    assert all(isinstance(p, int) and p for p in a[8:10] + a[12:17]) and len(set(a[8:10] + a[12:17])) == 7
    del recorded[:]
    lab, cen, raw, cnt = pipeline.superpixels(img, step=5, compactness=0, iters=3, min_size=7, centers=True, slic=True, counts=True)
    (name, a), = recorded
    assert a[:8] == (H, W, img.data_ptr(), 5, 0, 3, 7, 0) and a[8:12] == (lab.data_ptr(), cen.data_ptr(), raw.data_ptr(), cnt.data_ptr())
    assert pipeline.superpixel_grid(H, W, 5) == (4, 8, 32)
    assert (tuple(cen.shape), cen.dtype, tuple(raw.shape), raw.dtype, tuple(cnt.shape), cnt.dtype) == \
        ((32, 8), torch.int32, (H, W), torch.int32, (8,), torch.int32)
    del recorded[:]
    assert pipeline.superpixels(img, step=6, min_size=None) is not None and recorded[0][1][6] == 9, "min_size None is S*S//4"
    del recorded[:]
    lab, cnt = pipeline.superpixels(img, counts=True)
    assert recorded[0][1][10] is None and recorded[0][1][11] == cnt.data_ptr()
    del recorded[:]
    # the fit
    f2, f3, labels = torch.zeros((H, W, 2)), torch.zeros((H, W, 3)), torch.zeros((H, W), dtype=torch.int32)
    models, segc = pipeline.segment_fit(f2, labels, 11)
    (name, a), = recorded
    assert name == "dflow_segment_fit" and len(a) == 16
    assert a[:9] == (H, W, f2.data_ptr(), L.EVAL_DYDX, labels.data_ptr(), 11, 1.0, 3, 0) and a[9:11] == (models.data_ptr(), segc.data_ptr())
    assert a[11:14] == (None, None, None) and isinstance(a[14], int) and a[14] and a[14] % 8 == 0 and a[15] == "the stream"
    assert (tuple(models.shape), models.dtype, tuple(segc.shape), segc.dtype) == ((11, 6), torch.float32, (11, 4), torch.int32)
    del recorded[:]
    models, segc, out, cls, cnt = pipeline.segment_fit(f3, labels, 2, thresh=2.5, rounds=6, out=True, classes=True, counts=True)
    (name, a), = recorded
    assert a[:9] == (H, W, f3.data_ptr(), L.EVAL_UVV, labels.data_ptr(), 2, 2.5, 6, 0) and a[11:14] == (out.data_ptr(), cls.data_ptr(), cnt.data_ptr())
    assert (tuple(out.shape), out.dtype, tuple(cls.shape), cls.dtype, tuple(cnt.shape), cnt.dtype) == \
        ((H, W, 3), torch.float32, (H, W), torch.uint8, (8,), torch.int32)
    del recorded[:]
    models, segc, cnt = pipeline.segment_fit(f3, labels, 2, counts=True)
    assert recorded[0][1][11:13] == (None, None) and recorded[0][1][13] == cnt.data_ptr()
    assert pipeline.SUPERPIXEL_COUNTS[5] == "n_seg" and len(pipeline.SUPERPIXEL_COUNTS) == len(pipeline.SEGMENT_FIT_COUNTS) == 8


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    img, f2, labels = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.int32)
    for fn in (pipeline.superpixels, lambda im, **kw: pipeline.superpixel_flow(im, f2, **kw)):
        word = "superpixels" if fn is pipeline.superpixels else "superpixel_flow"
        for bad in (img.astype(np.float32), img[0], np.zeros((H, W, 4), np.uint8), np.zeros((0, W, 3), np.uint8)):
            with pytest.raises(ValueError, match="%s: img must be" % word):
                fn(bad)
        for kw, name in (({"step": 3}, "step"), ({"step": 65}, "step"), ({"step": 8.0}, "step"), ({"compactness": -1}, "compactness"),
                         ({"compactness": 256}, "compactness"), ({"iters": 0}, "iters"), ({"iters": 33}, "iters"), ({"iters": True}, "iters"),
                         ({"min_size": -1}, "min_size"), ({"min_size": (1 << 26) + 1}, "min_size"), ({"min_size": 2.5}, "min_size")):
            with pytest.raises(ValueError, match="%s: %s" % (word, name)):
                fn(img, **kw)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32)):
        with pytest.raises(ValueError, match="segment_fit: flow must be float32"):
            pipeline.segment_fit(bad, labels, 4)
    for bad in (labels.astype(np.int64), labels[:-1], np.zeros((H, W, 1), np.int32)):
        with pytest.raises(ValueError, match="segment_fit: labels must be int32"):
            pipeline.segment_fit(f2, bad, 4)
    for kw, name in (({"n_seg": 0}, "n_seg"), ({"n_seg": (1 << 26) + 1}, "n_seg"), ({"n_seg": 4.0}, "n_seg"), ({"thresh": 0.0}, "thresh"),
                     ({"thresh": NAN}, "thresh"), ({"thresh": INF}, "thresh"), ({"thresh": 1e-60}, "thresh"), ({"thresh": "1"}, "thresh"),
                     ({"rounds": 0}, "rounds"), ({"rounds": 7}, "rounds")):
        with pytest.raises(ValueError, match="segment_fit: %s" % name):
            pipeline.segment_fit(f2, labels, **dict({"n_seg": 4}, **kw))
    # both at once: the flow must have the image's frame, and the fit's arguments are checked before the image is uploaded
    with pytest.raises(ValueError, match="superpixel_flow: flow must be float32"):
        pipeline.superpixel_flow(img, f2[:-1])
    for kw, name in (({"thresh": 0.0}, "thresh"), ({"rounds": 7}, "rounds")):
        with pytest.raises(ValueError, match="superpixel_flow: %s" % name):
            pipeline.superpixel_flow(img, f2, **kw)
    with pytest.raises(TypeError):
        pipeline.superpixel_flow(img, f2, n_seg=3)


def test_command_line_refusals(L, capsys, tmp_path):
    sp = pkg("superpixels")
    for tail in (["--step", "3"], ["--step", "65"], ["--compactness", "-1"], ["--compactness", "256"], ["--iters", "0"], ["--iters", "33"],
                 ["--min-size", "-1"], ["--min-size", str((1 << 26) + 1)], ["--step", "x"], ["--boundaries", "b.npy"], ["--unknown"],
                 ["--flow", "f.flo"], ["--fit", "o.flo"], ["--thresh", "1"], ["--rounds", "2"], ["--classes", "c.png"], ["--models", "m.npy"],
                 ["--flow", "f.flo", "--fit", "o.png"], ["--flow", "f.flo", "--fit", "o.flo", "--thresh", "0"],
                 ["--flow", "f.flo", "--fit", "o.flo", "--thresh", "nan"], ["--flow", "f.flo", "--fit", "o.flo", "--thresh", "inf"],
                 ["--flow", "f.flo", "--fit", "o.flo", "--rounds", "0"], ["--flow", "f.flo", "--fit", "o.flo", "--rounds", "7"],
                 ["--flow", "f.flo", "--fit", "o.flo", "--classes", "c.npy"], ["--flow", "f.flo", "--fit", "o.flo", "--models", "m.png"]):
        with pytest.raises(SystemExit) as e:
            sp.main(["i.png", "o.npy"] + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    for argv in ([], ["i.png"], ["i.png", "o.flo"]):
        with pytest.raises(SystemExit) as e:
            sp.main(argv)
        assert e.value.code == 2
    a = sp.parser().parse_args(["i.png", "o.png", "--json"])
    assert (a.step, a.compactness, a.iters, a.min_size, a.boundaries, a.flow, a.fit, a.thresh, a.rounds, a.classes, a.models, a.json) == \
        (16, 10, 10, None, None, None, None, None, None, None, None, True)
    assert sp.MAX_MIN_SIZE == L.SEGMENTS_MAX
    # unreadable input: status 2 and a message, before any device is touched
    np.save(tmp_path / "g.npy", np.zeros((6, 9)))
    np.save(tmp_path / "i.npy", np.zeros((6, 9, 3), np.uint8))
    np.save(tmp_path / "f.npy", np.zeros((6, 8, 2), np.float32))
    capsys.readouterr()
    out = str(tmp_path / "o.npy")
    assert sp.main([str(tmp_path / "g.npy"), out]) == 2 and "not a (H,W,3) uint8 image" in capsys.readouterr().err
    assert sp.main([str(tmp_path / "missing.png"), out]) == 2 and "superpixels:" in capsys.readouterr().err
    assert sp.main([str(tmp_path / "i.txt"), out]) == 2 and "images are read as" in capsys.readouterr().err
    assert sp.main([str(tmp_path / "i.npy"), out, "--flow", str(tmp_path / "f.npy"), "--fit", str(tmp_path / "o.flo")]) == 2
    assert "is 8x6" in capsys.readouterr().err
    assert sp.main([str(tmp_path / "i.npy"), out, "--flow", str(tmp_path / "f.txt"), "--fit", str(tmp_path / "o.flo")]) == 2
    assert "unsupported flow file" in capsys.readouterr().err
    assert not os.path.exists(out)
    # the pictures
    labels = np.array([[0, 0, 1], [0, 2, 1], [300, 300, 70000]], np.int32)
    pic = sp.label_picture(labels, np)
    assert pic.dtype == np.uint8 and pic[2, 0].tolist() == [44, 1, 0] and pic[2, 2].tolist() == [112, 17, 1] and pic[0, 2].tolist() == [1, 0, 0]
    img = np.full((3, 3, 3), 9, np.uint8)
    edge = (sp.boundary_picture(img, labels, np) == (0, 0, 255)).all(axis=2)
    assert edge.tolist() == [[False, True, False], [True, True, True], [False, True, False]] and (img == 9).all()
