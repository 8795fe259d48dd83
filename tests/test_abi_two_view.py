"""What dflow_two_view refuses on the host, before anything is launched, each with its status and its text (the formats of abi.hip's
shared checks, in the order the header states); what pipeline.two_view refuses before any device is touched and what it hands to
the library; and what twoview.py and run_batch.py --pose refuse (CPU only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FLOW, MODEL, PART, POSE, STATE, DEPTH, CLS, ERR, CNT = (4096 * k for k in range(1, 10))      # non-NULL, aligned stand-ins
NAN, INF = float("nan"), float("inf")
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_the_binding_and_the_makefile_name_it(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    csrc = os.path.join(ROOT, PKG, "csrc")
    assert "int dflow_two_view(" in header and "dflow_two_view" in L.SYMBOLS
    assert "two_view.hip" in open(os.path.join(csrc, "Makefile")).read().split("SRCS :=")[1].split("\n")[0].split()
    assert hasattr(C.CDLL(L.LIB_PATH), "dflow_two_view")
    # a table of its own: the key sets of the others are pinned by the tests that cover them
    assert list(L._SIGNATURES_TWO_VIEW) == ["dflow_two_view"]
    others = set(L._SIGNATURES) | set(L._SIGNATURES_SHARED_GATE) | set(L._SIGNATURES_TRACKS) | set(L._SIGNATURES_EPIPOLAR) | \
        set(L._SIGNATURES_SUPERPIXELS)
    assert not set(L._SIGNATURES_TWO_VIEW) & others and set(L.SYMBOLS) == others | {"dflow_two_view"}
    # no workspace: the binding holds no size_t, and it is as long as the prototype
    restype, argtypes = L._SIGNATURES_TWO_VIEW["dflow_two_view"]
    assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == 19 and argtypes[6:10] == [C.c_double] * 4
    proto = re.search(r"int dflow_two_view\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto) and len(proto.split(",")) == len(argtypes)
    # the header's limits, its alignment line and its launch count
    block = header[header.index("/* Two-view reconstruction (DESIGN.md"):header.index("int dflow_two_view(")]
    for words in ("step outside [1,64]", "checked in this order", "4 launches and one or two memsets", "There is no d_ws", "8 cyclic Jacobi sweeps",
                  "2^-20 * sigma1", "ties to the smaller index", "NO POSE"):
        assert words in block, words
    assert "dflow_two_view              d_pose, d_state 8; d_flow, d_model, d_depth, d_err, d_counts 4; d_part, d_class 1" in header
    # what is shared with the fits has one definition, and the constants the restatement repeats are the file's
    text = open(os.path.join(csrc, "two_view.hip")).read()
    import two_view_ref as T
    assert '#include "fit_common.h"' in text and "#define TV_THREADS %d\n" % T.THREADS in text and "#define TV_PER_LANE %d " % T.PER_LANE in text and "#define TV_SWEEPS %d\n" % T.SWEEPS in text
    assert float(re.search(r"#define TV_SIGMA2_MIN (\S+)", text).group(1)) == T.SIGMA2_MIN
    import fit_common_pins
    fit_common_pins.check(csrc)
    # the gate adds no refusal text of its own to abi.hip, and lies after every slice the other tests cut out of it
    abi = open(os.path.join(csrc, "abi.hip")).read()
    assert abi.index("int dflow_two_view(") > abi.index("int dflow_remove_small_segments_host(")
    gate = abi[abi.index("int dflow_two_view("):]
    assert "launch_two_view(" in gate and "dflow_set_error(" not in gate
    assert pkg("pipeline").TWO_VIEW_COUNTS == T.COUNTS


def test_rejections_before_any_launch_status_text_and_order(L):
    lib = L.lib()

    def call(h=436, w=1024, flow=FLOW, layout=0, m=MODEL, part=PART, fx=1024.0, fy=1024.0, cx=511.5, cy=217.5, step=1, flags=0, pose=POSE,
             st=STATE, depth=DEPTH, cls=CLS, err=ERR, cnt=CNT):
        return lib.dflow_two_view(h, w, flow, layout, m, part, fx, fy, cx, cy, step, flags, pose, st, depth, cls, err, cnt, None)
    fn = "dflow_two_view: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"h": -1}, "image size 1024x-1 outside [1,8192]"),
             ({"layout": 2}, "unknown layout 2"), ({"layout": -1}, "unknown layout -1"),
             ({"fx": 0.0}, "fx=0 must be finite and > 0"), ({"fx": -1.0}, "fx=-1 must be finite and > 0"), ({"fx": NAN}, "fx=nan must be finite and > 0"),
             ({"fx": INF}, "fx=inf must be finite and > 0"), ({"fy": 0.0}, "fy=0 must be finite and > 0"), ({"fy": -INF}, "fy=-inf must be finite and > 0"),
             ({"fy": NAN}, "fy=nan must be finite and > 0"), ({"cx": NAN}, "cx=nan must be finite"), ({"cx": INF}, "cx=inf must be finite"),
             ({"cy": NAN}, "cy=nan must be finite"), ({"cy": -INF}, "cy=-inf must be finite"),
             ({"step": 0}, "step=0 outside [1,64]"), ({"step": 65}, "step=65 outside [1,64]"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"flow": None}, "d_flow is NULL"), ({"m": None}, "d_model is NULL"), ({"pose": None}, "d_pose is NULL"), ({"st": None}, "d_state is NULL"),
             ({"pose": POSE + 4}, "d_pose is not 8-byte aligned"), ({"st": STATE + 4}, "d_state is not 8-byte aligned"),
             ({"flow": FLOW + 2}, "d_flow is not 4-byte aligned"), ({"m": MODEL + 1}, "d_model is not 4-byte aligned"),
             ({"depth": DEPTH + 2}, "d_depth is not 4-byte aligned"), ({"err": ERR + 3}, "d_err is not 4-byte aligned"),
             ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_flow", "flow", FLOW), ("d_model", "m", MODEL), ("d_part", "part", PART), ("d_pose", "pose", POSE), ("d_state", "st", STATE),
              ("d_depth", "depth", DEPTH), ("d_class", "cls", CLS), ("d_err", "err", ERR), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(planes[3:], 3):            # every alias pair: an output against every plane before it
        cases += [({kw: p}, "%s is the same plane as %s" % (name, before)) for before, _, p in planes[:i]]
    assert len(cases) == 31 + sum(range(3, 9))
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    # the order: faults i .. n answer as fault i alone
    order = [{"h": 0}, {"layout": 9}, {"fx": NAN}, {"fy": 0.0}, {"cx": INF}, {"cy": NAN}, {"step": 0}, {"flags": 8}, {"flow": None}, {"m": None},
             {"pose": None}, {"st": None}, {"pose": POSE + 4}, {"st": STATE + 4}, {"flow": FLOW + 1}, {"m": MODEL + 2}, {"depth": DEPTH + 1},
             {"err": ERR + 1}, {"cnt": CNT + 1}, {"pose": FLOW}, {"st": MODEL}, {"depth": PART}, {"cls": DEPTH}, {"err": CLS}, {"cnt": ERR}]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)                       # an earlier entry of `order` overrides a later one's use of the same argument
        assert call(**kw) == EINVAL
        together = lib.dflow_last_error().decode()
        assert call(**order[i]) == EINVAL and lib.dflow_last_error().decode() == together, (i, kw, together)
    # the byte planes need no alignment, the inputs may alias each other, and optional arguments left out pass every check
    assert call(part=PART + 1, cls=CLS + 3, cnt=ERR) == EINVAL and lib.dflow_last_error().decode() == fn + "d_counts is the same plane as d_err"
    assert call(part=None, depth=None, cls=None, err=None, cnt=None, st=None) == EINVAL and b"d_state is NULL" in lib.dflow_last_error()
    # the ends of the ranges pass: the next refusal in line answers
    assert call(h=8192, w=8192, fx=5e-324, fy=1.7e308, cx=-1.7e308, cy=1.7e308, step=64, st=None) == EINVAL and b"d_state is NULL" in lib.dflow_last_error()


@pytest.fixture()
def recorded(L, monkeypatch):
    """pipeline's wrapper on host tensors with the library call recorded: [(name, args)]."""
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
    f2, f3, part = torch.zeros((H, W, 2)), torch.zeros((H, W, 3)), torch.ones((H, W), dtype=torch.uint8)
    m9, m33 = torch.zeros(9), torch.zeros((3, 3))
    pose = pipeline.two_view(f2, m9)
    assert isinstance(pose, torch.Tensor) and pose.dtype == torch.float64 and tuple(pose.shape) == (16,)
    (name, a), = recorded
    assert name == "dflow_two_view" and len(a) == 19
    # focal=None is max(H, W), center=None the frame's centre
    assert a[:12] == (H, W, f2.data_ptr(), L.EVAL_DYDX, m9.data_ptr(), None, 10.0, 10.0, 4.5, 2.5, 1, 0) and a[12] == pose.data_ptr()
    assert all(isinstance(v, float) for v in a[6:10])
    assert isinstance(a[13], int) and a[13] not in (0, a[12]) and a[14:] == (None, None, None, None, "the stream")
    del recorded[:]
    pose, depth, cls, err, cnt = pipeline.two_view(f3, m33, focal=(7.5, 8), center=(1.25, -2), part=part, step=4, depth=True, classes=True,
                                                   err=True, counts=True)
    (name, a), = recorded
    assert a[:12] == (H, W, f3.data_ptr(), L.EVAL_UVV, m33.data_ptr(), part.data_ptr(), 7.5, 8.0, 1.25, -2.0, 4, 0)
    assert a[14:18] == (depth.data_ptr(), cls.data_ptr(), err.data_ptr(), cnt.data_ptr())
    assert [(t.dtype, tuple(t.shape)) for t in (depth, cls, err, cnt)] == \
        [(torch.float32, (H, W)), (torch.uint8, (H, W)), (torch.float32, (H, W)), (torch.int32, (8,))]
    del recorded[:]
    pose, cnt = pipeline.two_view(f3, np.zeros(9, np.float32), focal=12, counts=True)
    assert recorded[0][1][6:10] == (12.0, 12.0, 4.5, 2.5) and recorded[0][1][14:17] == (None, None, None) and recorded[0][1][17] == cnt.data_ptr()
    assert pipeline.TWO_VIEW_COUNTS == ("voters", "votes", "runner_up", "candidate", "front", "behind", "flat", "reserved")


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    f2, f3, m = np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32), np.zeros(9, np.float32)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32)):
        with pytest.raises(ValueError, match="two_view: flow must be float32"):
            pipeline.two_view(bad, m)
    for bad in (m.astype(np.float64), np.zeros(8, np.float32), np.zeros((3, 4), np.float32), np.zeros((1, 9), np.float32)):
        with pytest.raises(ValueError, match="two_view: model must be float32"):
            pipeline.two_view(f2, bad)
    for bad in (np.zeros((H, W), np.float32), np.zeros((H, W + 1), np.uint8), np.zeros((H, W, 1), np.uint8)):
        with pytest.raises(ValueError, match="two_view: part"):
            pipeline.two_view(f3, m, part=bad)
    for kw, word in (({"focal": 0.0}, "focal"), ({"focal": NAN}, "focal"), ({"focal": INF}, "focal"), ({"focal": -3}, "focal"), ({"focal": "1"}, "focal"),
                     ({"focal": (1.0, 0.0)}, "focal"), ({"focal": (1.0, 2.0, 3.0)}, "focal"), ({"focal": True}, "focal"),
                     ({"center": 3.0}, "center"), ({"center": (1.0,)}, "center"), ({"center": (NAN, 0.0)}, "center"), ({"center": (0.0, INF)}, "center"),
                     ({"step": 0}, "step"), ({"step": 65}, "step"), ({"step": 2.0}, "step")):
        with pytest.raises(ValueError, match="two_view: %s" % word):
            pipeline.two_view(f2, m, **kw)
    with pytest.raises(TypeError):
        pipeline.two_view(f2, m, thresh=1.0)
    # the pose is host arithmetic on sixteen numbers
    with pytest.raises(ValueError, match="two_view_pose: pose must hold 16 numbers"):
        pipeline.two_view_pose(np.zeros(15))
    none = pipeline.two_view_pose([0.0] * 15 + [-1.0])
    assert none["candidate"] == -1 and none["axis"] is None and none["angle_deg"] == 0.0 and not none["R"].any() and not none["t"].any()
    c, s = np.cos(0.3), np.sin(0.3)
    turn = pipeline.two_view_pose([c, -s, 0, s, c, 0, 0, 0, 1, 0, 0, 1, 1, 0.5, 0.25, 2])
    assert turn["candidate"] == 2 and abs(turn["angle_deg"] - np.degrees(0.3)) < 1e-12 and np.allclose(turn["axis"], (0, 0, 1))
    assert turn["t"].tolist() == [0, 0, 1] and turn["singular"].tolist() == [1, 0.5, 0.25] and turn["R"].shape == (3, 3)
    same = pipeline.two_view_pose(list(np.eye(3).reshape(-1)) + [1, 0, 0, 1, 1, 0, 0])
    assert same["candidate"] == 0 and same["angle_deg"] == 0.0 and same["axis"] is None


def test_command_line_refusals(L, capsys, tmp_path):
    tv = pkg("twoview")
    for tail in (["--thresh", "0"], ["--thresh", "nan"], ["--hyp", "0"], ["--hyp", "21846"], ["--lo-rounds", "5"], ["--step", "0"], ["--step", "65"],
                 ["--seed", "-1"], ["--focal", "0"], ["--focal", "nan"], ["--focal", "inf"], ["--focal", "-2"], ["--focal", "x"],
                 ["--intrinsics", "1", "2", "3"], ["--intrinsics", "0", "1", "2", "3"], ["--intrinsics", "1", "1", "nan", "3"],
                 ["--intrinsics", "1", "inf", "2", "3"], ["--focal", "5", "--intrinsics", "1", "1", "2", "3"], ["--depth", "d.png"],
                 ["--classes", "c.npy"], ["--err", "e.flo"], ["--gate", "g.npy"], ["--unknown"]):
        with pytest.raises(SystemExit) as e:
            tv.main(["f.npy"] + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    with pytest.raises(SystemExit) as e:
        tv.main([])
    assert e.value.code == 2
    a = tv.parser().parse_args(["f.flo", "--json"])
    assert (a.focal, a.intrinsics, a.thresh, a.hyp, a.lo_rounds, a.step, a.seed, a.depth, a.classes, a.err, a.json) == \
        (None, None, 1.0, 512, 1, 1, 0, None, None, None, True)
    assert tv.camera(a) == ((None, None), None) and tv.MAX_HYP == L.EPIPOLAR_MAX_HYP
    assert tv.camera(tv.parser().parse_args(["f.flo", "--intrinsics", "7", "8", "1.5", "-2"])) == (((7.0, 8.0), (1.5, -2.0)), None)
    assert tv.camera(tv.parser().parse_args(["f.flo", "--focal", "9"])) == ((9.0, None), None)
    # unreadable input: status 2 and a message, before any device is touched
    np.save(tmp_path / "g.npy", np.zeros((6, 9)))
    capsys.readouterr()
    assert tv.main([str(tmp_path / "g.npy")]) == 2 and "expected an (H,W,2)" in capsys.readouterr().err
    assert tv.main([str(tmp_path / "missing.flo")]) == 2 and "twoview:" in capsys.readouterr().err
    assert tv.main([str(tmp_path / "f.txt")]) == 2 and "unsupported flow file" in capsys.readouterr().err
    # run_batch: --pose needs --epipolar and a focal length
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert a.pose is None and rb.pose_arg(a) is None
    a = rb.parser().parse_args(["--epipolar", "2", "--pose", "640"])
    assert rb.epipolar_arg(a) == 2.0 and rb.pose_arg(a) == 640.0
    for argv in (["--pose", "640"], ["--epipolar", "1", "--pose", "0"], ["--epipolar", "1", "--pose", "nan"], ["--epipolar", "1", "--pose", "inf"],
                 ["--epipolar", "1", "--pose", "x"], ["--epipolar", "1", "--pose"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--pose" in capsys.readouterr().err, argv
