"""What dflow_epipolar_fit refuses on the host, before anything is launched, each with its status and its text (the formats of
abi.hip's shared checks, in the order the header states); what pipeline.epipolar_fit refuses before any device is touched and
what it hands to the library; and what epipolar.py and run_batch.py --epipolar refuse (CPU only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FLOW, EX, MODEL, MODELS, HC, STATE, CLS, RES, CNT = (4096 * k for k in range(1, 10))     # non-NULL, aligned stand-ins
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
    assert "int dflow_epipolar_fit(" in header and "dflow_epipolar_fit" in L.SYMBOLS
    assert "epipolar.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert hasattr(C.CDLL(L.LIB_PATH), "dflow_epipolar_fit")
    assert "#define DFLOW_EPIPOLAR_MAX_HYP 21845" in header and L.EPIPOLAR_MAX_HYP == 21845 == 65535 // 3
    # a table of its own: the key sets of the others are pinned by the tests that cover them
    assert list(L._SIGNATURES_EPIPOLAR) == ["dflow_epipolar_fit"]
    assert not set(L._SIGNATURES_EPIPOLAR) & (set(L._SIGNATURES) | set(L._SIGNATURES_SHARED_GATE) | set(L._SIGNATURES_TRACKS))
    # no workspace: the binding holds no size_t, and it is as long as the prototype
    restype, argtypes = L._SIGNATURES_EPIPOLAR["dflow_epipolar_fit"]
    assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == 19
    assert issubclass(argtypes[9], C.c_uint64) and C.sizeof(argtypes[9]) == 8, "the seed is a uint64_t, and no byte count"
    proto = re.search(r"int dflow_epipolar_fit\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto) and len(proto.split(",")) == len(argtypes)
    # the header's limits, its alignment line and its launch count
    block = header[header.index("/* Epipolar-geometry fit of a flow field"):header.index("int dflow_epipolar_fit(")]
    for words in ("n_hyp outside [1,21845]", "lo_rounds outside [0,4]", "step outside\n * [1,64]", "checked in this order",
                  "3 + 4 (lo_rounds + 1) launches", "There is no d_ws"):
        assert words in block, words
    assert "dflow_epipolar_fit          d_state 8; d_flow, d_model, d_models, d_hyp_counts, d_residual, d_counts 4; d_exclude, d_class 1" in header
    # what is shared with the motion fit has one definition, and the chunk the tests derive their frames from is the file's
    csrc = os.path.join(ROOT, PKG, "csrc")
    text = open(os.path.join(csrc, "epipolar.hip")).read()
    import epipolar_ref
    import fit_common_pins
    import motion_ref
    assert '#include "fit_common.h"' in text
    fit_common_pins.check(csrc, epipolar_ref.CHUNK, motion_ref.CHUNK)
    # the gate adds no refusal text of its own to abi.hip
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("int dflow_epipolar_fit("):abi.index("int dflow_label_confidence(")]
    assert "launch_epipolar_fit(" in gate and "dflow_set_error(" not in gate


def test_rejections_before_any_launch_status_text_and_order(L):
    lib = L.lib()

    def call(h=436, w=1024, flow=FLOW, layout=0, ex=EX, thresh=1.0, n_hyp=512, lo=1, step=1, seed=0, flags=0, m=MODEL, ms=MODELS, hc=HC,
             st=STATE, cls=CLS, res=RES, cnt=CNT):
        return lib.dflow_epipolar_fit(h, w, flow, layout, ex, thresh, n_hyp, lo, step, seed, flags, m, ms, hc, st, cls, res, cnt, None)
    fn = "dflow_epipolar_fit: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"h": -1}, "image size 1024x-1 outside [1,8192]"),
             ({"layout": 2}, "unknown layout 2"), ({"layout": -1}, "unknown layout -1"),
             ({"thresh": 0.0}, "thresh=0 must be finite and > 0"), ({"thresh": -1.0}, "thresh=-1 must be finite and > 0"),
             ({"thresh": NAN}, "thresh=nan must be finite and > 0"), ({"thresh": INF}, "thresh=inf must be finite and > 0"),
             ({"n_hyp": 0}, "n_hyp=0 outside [1,21845]"), ({"n_hyp": 21846}, "n_hyp=21846 outside [1,21845]"),
             ({"lo": -1}, "lo_rounds=-1 outside [0,4]"), ({"lo": 5}, "lo_rounds=5 outside [0,4]"),
             ({"step": 0}, "step=0 outside [1,64]"), ({"step": 65}, "step=65 outside [1,64]"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"flow": None}, "d_flow is NULL"), ({"m": None}, "d_model is NULL"), ({"ms": None}, "d_models is NULL"),
             ({"hc": None}, "d_hyp_counts is NULL"), ({"st": None}, "d_state is NULL"),
             ({"st": STATE + 4}, "d_state is not 8-byte aligned"), ({"flow": FLOW + 2}, "d_flow is not 4-byte aligned"),
             ({"m": MODEL + 1}, "d_model is not 4-byte aligned"), ({"ms": MODELS + 2}, "d_models is not 4-byte aligned"),
             ({"hc": HC + 3}, "d_hyp_counts is not 4-byte aligned"), ({"res": RES + 1}, "d_residual is not 4-byte aligned"),
             ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_flow", "flow", FLOW), ("d_exclude", "ex", EX), ("d_model", "m", MODEL), ("d_models", "ms", MODELS), ("d_hyp_counts", "hc", HC),
              ("d_state", "st", STATE), ("d_class", "cls", CLS), ("d_residual", "res", RES), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(planes[2:], 2):
        cases += [({kw: p}, "%s is the same plane as %s" % (name, before)) for before, _, p in planes[:i]]
    assert len(cases) == 29 + sum(range(2, 9))
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    # the order: faults i .. n answer as fault i alone
    order = [{"h": 0}, {"layout": 9}, {"thresh": NAN}, {"n_hyp": 0}, {"lo": 9}, {"step": 0}, {"flags": 8}, {"flow": None}, {"m": None},
             {"ms": None}, {"hc": None}, {"st": None}, {"st": STATE + 4}, {"flow": FLOW + 1}, {"cnt": CNT + 1}, {"m": FLOW}, {"cnt": RES}]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)                       # an earlier entry of `order` overrides a later one's use of the same argument
        assert call(**kw) == EINVAL
        together = lib.dflow_last_error().decode()
        assert call(**order[i]) == EINVAL and lib.dflow_last_error().decode() == together, (i, kw, together)
    # the byte planes need no alignment, and optional arguments left out pass the alias and alignment checks
    assert call(ex=EX + 1, cls=CLS + 3, cnt=RES) == EINVAL and lib.dflow_last_error().decode() == fn + "d_counts is the same plane as d_residual"
    assert call(ex=None, cls=None, res=None, cnt=None, st=None) == EINVAL and b"d_state is NULL" in lib.dflow_last_error()
    # the largest n_hyp passes the range check: the next refusal in line answers
    assert call(n_hyp=21845, step=64, lo=4, thresh=1e-30, st=None) == EINVAL and b"d_state is NULL" in lib.dflow_last_error()


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
    f2, f3, ex = torch.zeros((H, W, 2)), torch.zeros((H, W, 3)), torch.zeros((H, W), dtype=torch.uint8)
    m = pipeline.epipolar_fit(f2)
    assert isinstance(m, torch.Tensor) and m.dtype == torch.float32 and tuple(m.shape) == (3, 3)
    (name, a), = recorded
    assert name == "dflow_epipolar_fit" and len(a) == 19
    assert a[:11] == (H, W, f2.data_ptr(), L.EVAL_DYDX, None, 1.0, 512, 1, 1, 0, 0) and a[11] == m.data_ptr()
    assert all(isinstance(p, int) and p for p in a[12:15]) and len(set(a[11:15])) == 4 and a[15:] == (None, None, None, "the stream")
    del recorded[:]
    m, cls, res, cnt = pipeline.epipolar_fit(f3, thresh=2.5, n_hyp=77, lo_rounds=3, step=4, seed=(5 << 32) | 9, exclude=ex, classes=True,
                                             residual=True, counts=True)
    (name, a), = recorded
    assert a[:11] == (H, W, f3.data_ptr(), L.EVAL_UVV, ex.data_ptr(), 2.5, 77, 3, 4, (5 << 32) | 9, 0)
    assert a[15:18] == (cls.data_ptr(), res.data_ptr(), cnt.data_ptr())
    assert (cls.dtype, tuple(cls.shape), res.dtype, tuple(res.shape), cnt.dtype, tuple(cnt.shape)) == \
        (torch.uint8, (H, W), torch.float32, (H, W), torch.int32, (8,))
    del recorded[:]
    m, cnt = pipeline.epipolar_fit(f3, counts=True)
    assert recorded[0][1][15:17] == (None, None) and recorded[0][1][17] == cnt.data_ptr()
    assert pipeline.EPIPOLAR_FIT_COUNTS == ("scored", "inliers", "degenerate", "best_round", "best_slot", "best_count", "models_per_1000",
                                            "reserved")


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    f2, f3 = np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32)):
        with pytest.raises(ValueError, match="epipolar_fit: flow must be float32"):
            pipeline.epipolar_fit(bad)
    for bad in (np.zeros((H, W), np.float32), np.zeros((H, W + 1), np.uint8), np.zeros((H, W, 1), np.uint8)):
        with pytest.raises(ValueError, match="epipolar_fit: exclude"):
            pipeline.epipolar_fit(f3, exclude=bad)
    for kw, word in (({"thresh": 0.0}, "thresh"), ({"thresh": NAN}, "thresh"), ({"thresh": INF}, "thresh"), ({"thresh": 1e-60}, "thresh"),
                     ({"thresh": "1"}, "thresh"), ({"n_hyp": 0}, "n_hyp"), ({"n_hyp": 21846}, "n_hyp"), ({"n_hyp": 10.0}, "n_hyp"),
                     ({"lo_rounds": 5}, "lo_rounds"), ({"lo_rounds": -1}, "lo_rounds"), ({"step": 0}, "step"), ({"step": 65}, "step"),
                     ({"seed": -1}, "seed"), ({"seed": 1 << 64}, "seed")):
        with pytest.raises(ValueError, match="epipolar_fit: %s" % word):
            pipeline.epipolar_fit(f2, **kw)
    with pytest.raises(TypeError):
        pipeline.epipolar_fit(f2, polish=1)
    # the geometry is host arithmetic on nine numbers
    for bad in ((0, 10), (10, 8193), (10.0, 10)):
        with pytest.raises(ValueError, match="epipolar_geometry: h and w"):
            pipeline.epipolar_geometry(np.zeros(9), *bad)
    geo = pipeline.epipolar_geometry(np.zeros((3, 3), np.float32), 33, 65)
    assert not geo["F"].any() and geo["foe"] is None, "no model: no epipole"
    # a sideways motion in the normalised coordinates: F^ = [t]x with t = (1,0,0); epipoles at infinity along x
    geo = pipeline.epipolar_geometry([0, 0, 0, 0, 0, -1, 0, 1, 0], 33, 65)
    assert geo["foe"] is None and geo["e1"][1] == 0 and geo["e1"][2] == 0 and geo["e1"][0] != 0 and geo["e2"][0] != 0
    # a forward motion: F^ = [t]x with t = (0,0,1): the epipole is the centre of the normalised frame, the principal point
    geo = pipeline.epipolar_geometry([0, -1, 0, 1, 0, 0, 0, 0, 0], 33, 65)
    assert geo["foe"] == (32.0, 16.0) and np.allclose(geo["e2"][:2] / geo["e2"][2], (32.0, 16.0))


def test_command_line_refusals(L, capsys, tmp_path):
    ep = pkg("epipolar")
    for tail in (["--thresh", "0"], ["--thresh", "nan"], ["--thresh", "inf"], ["--thresh", "-1"], ["--hyp", "0"], ["--hyp", "21846"],
                 ["--lo-rounds", "5"], ["--lo-rounds", "-1"], ["--step", "0"], ["--step", "65"], ["--seed", "-1"], ["--classes", "c.flo"],
                 ["--residual", "r.flo"], ["--gate", "g.png"], ["--hyp", "x"], ["--polish", "1"], ["--unknown"]):
        with pytest.raises(SystemExit) as e:
            ep.main(["f.npy"] + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    with pytest.raises(SystemExit) as e:
        ep.main([])
    assert e.value.code == 2
    a = ep.parser().parse_args(["f.flo", "--json"])
    assert (a.thresh, a.hyp, a.lo_rounds, a.step, a.seed, a.classes, a.residual, a.gate, a.json) == (1.0, 512, 1, 1, 0, None, None, None, True)
    assert ep.MAX_HYP == L.EPIPOLAR_MAX_HYP
    # unreadable input: status 2 and a message, before any device is touched
    np.save(tmp_path / "g.npy", np.zeros((6, 9)))
    capsys.readouterr()
    assert ep.main([str(tmp_path / "g.npy")]) == 2 and "expected an (H,W,2)" in capsys.readouterr().err
    assert ep.main([str(tmp_path / "missing.flo")]) == 2 and "epipolar:" in capsys.readouterr().err
    assert ep.main([str(tmp_path / "f.txt")]) == 2 and "unsupported flow file" in capsys.readouterr().err
    # the gate keeps the survivors' bits in both layouts and drops class 2 only
    cls = np.array([[0, 1, 2, 3]], np.uint8)
    f3 = np.array([[[1.5, -2.5, 0], [np.float32(0.1), -0.0, 1], [7, 8, 1], [3, 4, 1]]], np.float32)
    g = ep.gated(f3, cls, np)
    assert g.tobytes() == np.array([[[0, 0, 0], [np.float32(0.1), -0.0, 1], [0, 0, 0], [3, 4, 1]]], np.float32).tobytes()
    g2 = ep.gated(np.ascontiguousarray(f3[..., [1, 0]]), cls, np)
    assert g2.tobytes() == g.tobytes()
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert a.epipolar is None and a.epipolar_gate is False and rb.epipolar_arg(a) is None
    a = rb.parser().parse_args(["--epipolar", "2.5", "--epipolar-gate"])
    assert rb.epipolar_arg(a) == 2.5 and a.epipolar_gate is True
    for argv in (["--epipolar", "0"], ["--epipolar", "nan"], ["--epipolar", "inf"], ["--epipolar", "x"], ["--epipolar-gate"], ["--epipolar"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--epipolar" in capsys.readouterr().err, argv
