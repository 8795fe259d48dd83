"""What dflow_motion_fit refuses on the host, before anything is launched, each with its status and its text (the formats of
abi.hip's shared checks, in the order the header states); what pipeline.motion_fit and motion_layers refuse before any device is
touched and what the wrapper hands to the library; and what motionfit.py and run_batch.py --motion refuse (CPU only; no compute
calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FLOW, EX, MODEL, MODELS, HC, STATE, CLS, MF, RES, CNT = (4096 * k for k in range(1, 11))     # non-NULL, aligned stand-ins
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
    assert "int dflow_motion_fit(" in header and "dflow_motion_fit" in L.SYMBOLS
    assert "motion_fit.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert hasattr(C.CDLL(L.LIB_PATH), "dflow_motion_fit")
    assert "#define DFLOW_MOTION_AFFINE 0" in header and L.MOTION_AFFINE == 0
    assert "#define DFLOW_MOTION_HOMOGRAPHY 1" in header and L.MOTION_HOMOGRAPHY == 1
    # no workspace: the binding holds no size_t, and it is as long as the prototype
    restype, argtypes = L._SIGNATURES_SHARED_GATE["dflow_motion_fit"]
    assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == 22
    assert issubclass(argtypes[11], C.c_uint64) and C.sizeof(argtypes[11]) == 8, "the seed is a uint64_t, and no byte count"
    proto = re.search(r"int dflow_motion_fit\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto) and len(proto.split(",")) == len(argtypes)
    # one definition of the generator, of a good vector and of the chunk the tests derive their frames from
    csrc = os.path.join(ROOT, PKG, "csrc")
    defs = [name for name in sorted(os.listdir(csrc)) if name.endswith((".hip", ".h")) and "void philox4x32_10(" in open(os.path.join(csrc, name)).read()]
    assert defs == ["philox.h"]
    for name in ("neighbour.hip", "fit_common.h"):
        assert '#include "philox.h"' in open(os.path.join(csrc, name)).read()
    text = open(os.path.join(csrc, "motion_fit.hip")).read()
    import epipolar_ref
    import fit_common_pins
    import motion_ref
    assert "flow_good(" in text and '#include "fit_common.h"' in text and "mf_gauss(" in text
    # what the fits share has one definition, and the one chunk is the one both restatements derive their frames from
    fit_common_pins.check(csrc, motion_ref.CHUNK, epipolar_ref.CHUNK)
    # the count of a wave's flagged lanes and the tree of the polish sums are wave_ops.h's
    import wave_ops_pins
    wave_ops_pins.check(csrc)
    # the gate adds no refusal text of its own to abi.hip
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("int dflow_motion_fit("):abi.index("int dflow_remove_small_segments_host(")]
    assert "dflow_set_error(" not in gate


def test_rejections_before_any_launch_status_text_and_order(L):
    lib = L.lib()

    def call(h=436, w=1024, flow=FLOW, layout=0, ex=EX, model=0, thresh=1.0, n_hyp=1024, lo=1, polish=2, step=1, seed=0, flags=0,
             m=MODEL, ms=MODELS, hc=HC, st=STATE, cls=CLS, mf=MF, res=RES, cnt=CNT):
        return lib.dflow_motion_fit(h, w, flow, layout, ex, model, thresh, n_hyp, lo, polish, step, seed, flags, m, ms, hc, st, cls, mf, res,
                                    cnt, None)
    fn = "dflow_motion_fit: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"h": -1}, "image size 1024x-1 outside [1,8192]"),
             ({"layout": 2}, "unknown layout 2"), ({"layout": -1}, "unknown layout -1"),
             ({"model": 2}, "model=2 outside [0,1]"), ({"model": -1}, "model=-1 outside [0,1]"),
             ({"thresh": 0.0}, "thresh=0 must be finite and > 0"), ({"thresh": -1.0}, "thresh=-1 must be finite and > 0"),
             ({"thresh": NAN}, "thresh=nan must be finite and > 0"), ({"thresh": INF}, "thresh=inf must be finite and > 0"),
             ({"n_hyp": 0}, "n_hyp=0 outside [1,65536]"), ({"n_hyp": 65537}, "n_hyp=65537 outside [1,65536]"),
             ({"lo": -1}, "lo_rounds=-1 outside [0,4]"), ({"lo": 5}, "lo_rounds=5 outside [0,4]"),
             ({"polish": -1}, "polish=-1 outside [0,4]"), ({"polish": 5}, "polish=5 outside [0,4]"),
             ({"step": 0}, "step=0 outside [1,64]"), ({"step": 65}, "step=65 outside [1,64]"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"flow": None}, "d_flow is NULL"), ({"m": None}, "d_model is NULL"), ({"ms": None}, "d_models is NULL"),
             ({"hc": None}, "d_hyp_counts is NULL"), ({"st": None}, "d_state is NULL"),
             ({"st": STATE + 4}, "d_state is not 8-byte aligned"), ({"flow": FLOW + 2}, "d_flow is not 4-byte aligned"),
             ({"m": MODEL + 1}, "d_model is not 4-byte aligned"), ({"ms": MODELS + 2}, "d_models is not 4-byte aligned"),
             ({"hc": HC + 3}, "d_hyp_counts is not 4-byte aligned"), ({"mf": MF + 2}, "d_model_flow is not 4-byte aligned"),
             ({"res": RES + 1}, "d_residual is not 4-byte aligned"), ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_flow", "flow", FLOW), ("d_exclude", "ex", EX), ("d_model", "m", MODEL), ("d_models", "ms", MODELS), ("d_hyp_counts", "hc", HC),
              ("d_state", "st", STATE), ("d_class", "cls", CLS), ("d_model_flow", "mf", MF), ("d_residual", "res", RES), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(planes[2:], 2):
        cases += [({kw: p}, "%s is the same plane as %s" % (name, before)) for before, _, p in planes[:i]]
    assert len(cases) == 34 + sum(range(2, 10))
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    # the order: each refusal wins over every one after it
    order = [{"h": 0}, {"layout": 9}, {"model": 9}, {"thresh": NAN}, {"n_hyp": 0}, {"lo": 9}, {"polish": 9}, {"step": 0}, {"flags": 8},
             {"flow": None}, {"m": None}, {"ms": None}, {"hc": None}, {"st": None}, {"st": STATE + 4}, {"flow": FLOW + 1}, {"cnt": CNT + 1},
             {"m": FLOW}, {"cnt": RES}]
    words = ["image size", "layout", "model=", "thresh=", "n_hyp=", "lo_rounds=", "polish=", "step=", "flags", "d_flow is NULL", "d_model is NULL",
             "d_models is NULL", "d_hyp_counts is NULL", "d_state is NULL", "d_state is not 8", "d_flow is not 4", "d_counts is not 4",
             "d_model is the same plane as d_flow", "d_counts is the same plane as d_residual"]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)                       # an earlier entry of `order` overrides a later one's use of the same argument
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (i, kw, lib.dflow_last_error())
    # optional arguments left out pass the gate's alias and alignment checks: the next refusal in line is reported
    assert call(ex=None, cls=None, mf=None, res=None, cnt=None, st=None) == EINVAL and b"d_state is NULL" in lib.dflow_last_error()


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
    m = pipeline.motion_fit(f2)
    assert isinstance(m, torch.Tensor) and m.dtype == torch.float32 and tuple(m.shape) == (3, 3)
    (name, a), = recorded
    assert name == "dflow_motion_fit" and len(a) == 22
    assert a[:13] == (H, W, f2.data_ptr(), L.EVAL_DYDX, None, L.MOTION_AFFINE, 1.0, 1024, 1, 2, 1, 0, 0) and a[13] == m.data_ptr()
    assert all(isinstance(p, int) and p for p in a[14:17]) and len(set(a[13:17])) == 4 and a[17:] == (None, None, None, None, "the stream")
    del recorded[:]
    m, cls, mf, res, cnt = pipeline.motion_fit(f3, model="homography", thresh=2.5, n_hyp=77, lo_rounds=3, polish=0, step=4, seed=(5 << 32) | 9,
                                               exclude=ex, classes=True, model_flow=True, residual=True, counts=True)
    (name, a), = recorded
    assert a[:13] == (H, W, f3.data_ptr(), L.EVAL_UVV, ex.data_ptr(), L.MOTION_HOMOGRAPHY, 2.5, 77, 3, 0, 4, (5 << 32) | 9, 0)
    assert a[17:21] == (cls.data_ptr(), mf.data_ptr(), res.data_ptr(), cnt.data_ptr())
    assert (cls.dtype, tuple(cls.shape), tuple(mf.shape), tuple(res.shape), cnt.dtype, tuple(cnt.shape)) == \
        (torch.uint8, (H, W), (H, W, 3), (H, W, 3), torch.int32, (8,))
    del recorded[:]
    m, cnt = pipeline.motion_fit(f3, counts=True)
    assert recorded[0][1][17:20] == (None, None, None) and recorded[0][1][20] == cnt.data_ptr()
    assert pipeline.MOTION_FIT_COUNTS == ("scored", "inliers", "degenerate", "best_round", "best_j", "best_count", "accepted", "skipped")
    # the layers: k calls of the one entry point that share their scratch planes, every one with the classes and an exclude mask
    del recorded[:]
    models, layers = pipeline.motion_layers(f3, 3, n_hyp=50, seed=7)
    assert [n for n, _ in recorded] == ["dflow_motion_fit"] * 3 and len(models) == 3 and layers.dtype == torch.uint8 and tuple(layers.shape) == (H, W)
    for _, a in recorded:
        assert a[7] == 50 and a[11] == 7 and a[4] is not None and a[17] is not None and a[18:21] == (None, None, None)
        assert a[14:17] == recorded[0][1][14:17]
    assert len({a[13] for _, a in recorded}) == 3, "every fit has its own model"


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    f2, f3 = np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32)
    for fn, run in (("motion_fit", lambda flow, **kw: pipeline.motion_fit(flow, **kw)),
                    ("motion_layers", lambda flow, **kw: pipeline.motion_layers(flow, 2, **kw))):
        for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32)):
            with pytest.raises(ValueError, match="%s: flow must be float32" % fn):
                run(bad)
        for bad in (np.zeros((H, W), np.float32), np.zeros((H, W + 1), np.uint8), np.zeros((H, W, 1), np.uint8)):
            with pytest.raises(ValueError, match="%s: exclude" % fn):
                run(f3, exclude=bad)
        for kw, word in (({"model": "rigid"}, "model"), ({"model": 0}, "model"), ({"thresh": 0.0}, "thresh"), ({"thresh": NAN}, "thresh"),
                         ({"thresh": INF}, "thresh"), ({"thresh": 1e-60}, "thresh"), ({"thresh": "1"}, "thresh"), ({"n_hyp": 0}, "n_hyp"),
                         ({"n_hyp": 65537}, "n_hyp"), ({"n_hyp": 10.0}, "n_hyp"), ({"lo_rounds": 5}, "lo_rounds"), ({"lo_rounds": -1}, "lo_rounds"),
                         ({"polish": 5}, "polish"), ({"step": 0}, "step"), ({"step": 65}, "step"), ({"seed": -1}, "seed"), ({"seed": 1 << 64}, "seed")):
            with pytest.raises(ValueError, match="%s: %s" % (fn, word)):
                run(f2, **kw)
    for k in (0, 256, 1.0):
        with pytest.raises(ValueError, match="motion_layers: k"):
            pipeline.motion_layers(f2, k)
    with pytest.raises(ValueError, match="motion_layers: unknown arguments"):
        pipeline.motion_layers(f2, 2, classes=True)


def test_command_line_refusals(L, capsys, tmp_path):
    mf = pkg("motionfit")
    for tail in (["--model", "rigid"], ["--thresh", "0"], ["--thresh", "nan"], ["--thresh", "inf"], ["--thresh", "-1"], ["--hyp", "0"],
                 ["--hyp", "65537"], ["--lo-rounds", "5"], ["--lo-rounds", "-1"], ["--polish", "5"], ["--step", "0"], ["--step", "65"],
                 ["--seed", "-1"], ["--layers", "0"], ["--layers", "256"], ["--layers", "2", "--model-flow", "m.flo"],
                 ["--layers", "2", "--residual", "r.flo"], ["--model-flow", "m.npy"], ["--residual", "r.png"], ["--classes", "c.flo"],
                 ["--hyp", "x"], ["--unknown"]):
        with pytest.raises(SystemExit) as e:
            mf.main(["f.npy"] + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    with pytest.raises(SystemExit) as e:
        mf.main([])
    assert e.value.code == 2
    a = mf.parser().parse_args(["f.flo", "--json"])
    assert (a.model, a.thresh, a.hyp, a.lo_rounds, a.polish, a.step, a.seed, a.model_flow, a.residual, a.classes, a.layers, a.json) == \
        ("affine", 1.0, 1024, 1, 2, 1, 0, None, None, None, None, True)
    # unreadable input: status 2 and a message, before any device is touched
    np.save(tmp_path / "g.npy", np.zeros((6, 9)))
    capsys.readouterr()
    assert mf.main([str(tmp_path / "g.npy")]) == 2 and "expected an (H,W,2)" in capsys.readouterr().err
    assert mf.main([str(tmp_path / "missing.flo")]) == 2 and "motionfit:" in capsys.readouterr().err
    assert mf.main([str(tmp_path / "f.txt")]) == 2 and "unsupported flow file" in capsys.readouterr().err
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert a.motion is None and a.motion_thresh is None and rb.motion_args(a) == (None, 1.0)
    a = rb.parser().parse_args(["--motion", "homography", "--motion-thresh", "2.5"])
    assert rb.motion_args(a) == ("homography", 2.5)
    for argv in (["--motion", "rigid"], ["--motion", "0"], ["--motion", "affine", "--motion-thresh", "0"],
                 ["--motion", "affine", "--motion-thresh", "nan"], ["--motion", "affine", "--motion-thresh", "inf"],
                 ["--motion", "affine", "--motion-thresh", "x"], ["--motion-thresh", "1"], ["--motion"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--motion" in capsys.readouterr().err, argv
