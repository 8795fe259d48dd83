"""What dflow_label_confidence and dflow_flow_gate refuse on the host, before anything is launched, each with its status and its
text (the formats of abi.hip's shared checks, in the order the header states); what DiscreteFlow.confidence and pipeline.flow_gate
refuse before any device is touched and what flow_gate hands to the library; and what "python bcd.py" --confidence,
spremiZaEpic.py --margin and run_batch.py --confidence refuse (CPU only; no compute calls here)."""
import ctypes as C
import os
import re
import runpy

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

PROP, COST, NPROP, LAB, MARGIN, ALT, SPARSE, CNT = (4096 * k for k in range(1, 9))       # non-NULL, aligned stand-ins
NAN, INF = float("nan"), float("inf")
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def prototype(header, name):
    return re.search(r"int %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)


def test_the_header_the_binding_and_the_makefile_name_them(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    csrc = os.path.join(ROOT, PKG, "csrc")
    assert "label_conf.hip" in open(os.path.join(csrc, "Makefile")).read()
    handle = C.CDLL(L.LIB_PATH)
    for name, nargs in (("dflow_label_confidence", 13), ("dflow_flow_gate", 10)):
        assert "int %s(" % name in header and name in L.SYMBOLS and hasattr(handle, name)
        restype, argtypes = L._SIGNATURES_SHARED_GATE[name]
        proto = prototype(header, name)
        # no workspace: the binding holds no size_t, and it is as long as the prototype
        assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == nargs == len(proto.split(","))
        assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto)
    assert "#define DFLOW_CONF_LOCAL 0" in header and L.CONF_LOCAL == 0
    assert "#define DFLOW_CONF_DATA  1" in header and L.CONF_DATA == 1
    assert "#define DFLOW_CONF_COUNTS 6" in header and L.CONF_COUNTS == 6
    # one copy of the row helpers, in wave_ops.h, and both users include it
    defs = [n for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h")) and "int row_min16(" in open(os.path.join(csrc, n)).read()]
    assert defs == ["wave_ops.h"]
    text = open(os.path.join(csrc, "label_conf.hip")).read()
    assert '#include "wave_ops.h"' in text and '#include "wave_ops.h"' in open(os.path.join(csrc, "prior.hip")).read()
    assert "row_min16(" in text and "flow_l1_biased(" in text and "flow_load4<" in text and "asm" not in text
    # the gates add no refusal text of their own to abi.hip
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("int dflow_label_confidence("):abi.index("int dflow_remove_small_segments_host(")]
    assert "int dflow_flow_gate(" in gate and "dflow_set_error(" not in gate


def params(L, **kw):
    p = L.default_params(436, 1024, 27, 64)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_label_confidence_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(p=None, prop=PROP, cost=COST, nprop=NPROP, lab=LAB, mode=0, min_sep=1, thresh=0.0, margin=MARGIN, alt=ALT, sparse=SPARSE,
             cnt=CNT, **fields):
        pp = C.byref(params(L, **fields)) if p is None else p
        return lib.dflow_label_confidence(pp, prop, cost, nprop, lab, mode, min_sep, thresh, margin, alt, sparse, cnt, None)
    fn = "dflow_label_confidence: "
    cases = [({"p": C.POINTER(L.Params)()}, "params is NULL"),
             ({"pich": 0}, "image size 1024x0 outside [1,8192]"), ({"picw": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"label_pitch": 8}, "label_pitch=8 must be a multiple of 16 in [16,160]"),
             ({"label_pitch": 150}, "label_pitch=150 must be a multiple of 16 in [16,160]"),
             ({"label_pitch": 176}, "label_pitch=176 must be a multiple of 16 in [16,160]"),
             ({"maxnprop": 0}, "maxnprop=0 outside [1,label_pitch=160]"), ({"maxnprop": 161}, "maxnprop=161 outside [1,label_pitch=160]"),
             ({"tpsi": 0}, "tpsi=0 outside [1,8]"), ({"tpsi": 9}, "tpsi=9 outside [1,8]"),
             ({"lamda": -1.0}, "lamda=-1 must be finite and >= 0"), ({"lamda": NAN}, "lamda=nan must be finite and >= 0"),
             ({"lamda": INF}, "lamda=inf must be finite and >= 0"),
             ({"mode": 2}, "mode=2 outside [0,1]"), ({"mode": -1}, "mode=-1 outside [0,1]"),
             ({"min_sep": -1}, "min_sep=-1 outside [0,1024]"), ({"min_sep": 1025}, "min_sep=1025 outside [0,1024]"),
             ({"thresh": NAN}, "thresh=nan must be a number"),
             ({"margin": None, "alt": None, "sparse": None, "cnt": None}, "each of d_margin, d_alt, d_sparse and d_counts is NULL"),
             ({"prop": None}, "d_proposals is NULL"), ({"cost": None}, "d_lcosts is NULL"), ({"nprop": None}, "d_nprop is NULL"),
             ({"lab": None}, "d_bestlabels is NULL"),
             ({"prop": PROP + 8}, "d_proposals is not 16-byte aligned"), ({"cost": COST + 4}, "d_lcosts is not 16-byte aligned"),
             ({"sparse": SPARSE + 12}, "d_sparse is not 16-byte aligned"), ({"nprop": NPROP + 2}, "d_nprop is not 4-byte aligned"),
             ({"lab": LAB + 1}, "d_bestlabels is not 4-byte aligned"), ({"margin": MARGIN + 2}, "d_margin is not 4-byte aligned"),
             ({"alt": ALT + 3}, "d_alt is not 4-byte aligned"), ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_proposals", "prop", PROP), ("d_lcosts", "cost", COST), ("d_nprop", "nprop", NPROP), ("d_bestlabels", "lab", LAB),
              ("d_margin", "margin", MARGIN), ("d_alt", "alt", ALT), ("d_sparse", "sparse", SPARSE), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(planes[4:], 4):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, _, q in planes[:i]]
    assert len(cases) == 31 + 4 + 5 + 6 + 7
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    # tphi is not read: what dflow_bcd_stats refuses passes here as far as the first pointer
    assert call(tphi=NAN, prop=None) == EINVAL and b"d_proposals is NULL" in lib.dflow_last_error()
    # infinite thresholds pass the gate: the next refusal in line is reported
    for t in (INF, -INF):
        assert call(thresh=t, prop=None) == EINVAL and b"d_proposals is NULL" in lib.dflow_last_error()
    # the order: each refusal wins over every one after it
    order = [{"pich": 0}, {"label_pitch": 8}, {"maxnprop": 0}, {"tpsi": 0}, {"lamda": NAN}, {"mode": 9}, {"min_sep": -1}, {"thresh": NAN},
             {"margin": None, "alt": None, "sparse": None, "cnt": None}, {"prop": None}, {"cost": None}, {"nprop": None}, {"lab": None}]
    words = ["image size", "label_pitch=", "maxnprop=", "tpsi=", "lamda=", "mode=", "min_sep=", "thresh=nan must be a number", "each of d_margin",
             "d_proposals is NULL", "d_lcosts is NULL", "d_nprop is NULL", "d_bestlabels is NULL"]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (i, kw, lib.dflow_last_error())
    order = [{"lab": None}, {"prop": PROP + 4}, {"cnt": CNT + 1}, {"margin": PROP}, {"cnt": SPARSE}]
    words = ["d_bestlabels is NULL", "d_proposals is not 16", "d_counts is not 4", "d_margin is the same plane as d_proposals",
             "d_counts is the same plane as d_sparse"]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (i, kw, lib.dflow_last_error())
    # one output is enough for the gate: with only d_counts the next refusal in line is reported
    assert call(margin=None, alt=None, sparse=None, lab=None) == EINVAL and b"d_bestlabels is NULL" in lib.dflow_last_error()


def test_flow_gate_rejections_status_text_and_order(L):
    lib = L.lib()
    FLOW, SCORE, OUT, CNT2 = PROP, COST, MARGIN, CNT

    def call(h=436, w=1024, flow=FLOW, layout=0, score=SCORE, lo=0.0, hi=1.0, out=OUT, cnt=CNT2):
        return lib.dflow_flow_gate(h, w, flow, layout, score, lo, hi, out, cnt, None)
    fn = "dflow_flow_gate: "
    cases = [({"h": 0}, "image size 1024x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x436 outside [1,8192]"),
             ({"layout": 2}, "unknown layout 2"), ({"layout": -1}, "unknown layout -1"),
             ({"lo": NAN}, "lo=nan must be a number"), ({"hi": NAN}, "hi=nan must be a number"), ({"lo": 2.0}, "lo=2 must be <= hi=1"),
             ({"lo": INF, "hi": -INF}, "lo=inf must be <= hi=-inf"),
             ({"flow": None}, "d_flow is NULL"), ({"score": None}, "d_score is NULL"), ({"out": None}, "d_out is NULL"),
             ({"flow": FLOW + 4}, "d_flow is not 16-byte aligned"), ({"score": SCORE + 8}, "d_score is not 16-byte aligned"),
             ({"out": OUT + 12}, "d_out is not 16-byte aligned"), ({"cnt": CNT2 + 2}, "d_counts is not 4-byte aligned"),
             ({"out": FLOW, "layout": 1}, "d_out is the same plane as d_flow"), ({"out": SCORE}, "d_out is the same plane as d_score"),
             ({"cnt": FLOW}, "d_counts is the same plane as d_flow"), ({"cnt": SCORE}, "d_counts is the same plane as d_score"),
             ({"cnt": OUT}, "d_counts is the same plane as d_out"),
             ({"out": FLOW, "cnt": FLOW}, "d_counts is the same plane as d_flow")]
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    order = [{"h": 0}, {"layout": 9}, {"lo": NAN}, {"hi": NAN}, {"lo": 5.0}, {"flow": None}, {"score": None}, {"out": None},
             {"flow": FLOW + 4}, {"cnt": CNT2 + 1}, {"out": SCORE}]
    words = ["image size", "layout", "lo=nan must be", "hi=nan must be", "must be <= hi", "d_flow is NULL", "d_score is NULL", "d_out is NULL",
             "d_flow is not 16", "d_counts is not 4", "same plane"]
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (i, kw, lib.dflow_last_error())
    # infinities, lo == hi and d_out = d_flow under [U,V,valid] pass the gate: the next refusal in line is reported
    assert call(lo=-INF, hi=INF, score=None) == EINVAL and b"d_score is NULL" in lib.dflow_last_error()
    assert call(lo=1.0, hi=1.0, score=None) == EINVAL and b"d_score is NULL" in lib.dflow_last_error()
    assert call(out=FLOW, layout=0, cnt=CNT2 + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()


def test_flow_gate_hands_over_what_it_was_given(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda dev: "the stream")
    monkeypatch.setattr(pipeline, "_device_of", lambda *tensors: torch.device("cpu"))
    H, W = 6, 10
    f2, f3, sc = torch.zeros((H, W, 2)), torch.zeros((H, W, 3)), torch.zeros((H, W))
    out = pipeline.flow_gate(f2, sc)
    (name, a), = calls
    assert name == "dflow_flow_gate" and a == (H, W, f2.data_ptr(), L.EVAL_DYDX, sc.data_ptr(), -INF, INF, out.data_ptr(), None, "the stream")
    assert out.dtype == torch.float32 and tuple(out.shape) == (H, W, 3)
    del calls[:]
    out, cnt = pipeline.flow_gate(f3, sc, lo=0.5, hi=2, counts=True)
    assert calls[0][1] == (H, W, f3.data_ptr(), L.EVAL_UVV, sc.data_ptr(), 0.5, 2.0, out.data_ptr(), cnt.data_ptr(), "the stream")
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (2,) and out.data_ptr() != f3.data_ptr()
    assert pipeline.LABEL_CONF_COUNTS == ("labelled", "not_labelled", "no_alternative", "negative", "zero", "kept")
    assert pipeline.CONF_MODES == {"local": L.CONF_LOCAL, "data": L.CONF_DATA}


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 20, 24
    f2, sc = np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.float32)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((H, W, 4), np.float32)):
        with pytest.raises(ValueError, match="flow_gate: flow must be float32"):
            pipeline.flow_gate(bad, sc)
    for bad in (sc.astype(np.float64), np.zeros((H, W + 1), np.float32), np.zeros((H, W, 1), np.float32)):
        with pytest.raises(ValueError, match="flow_gate: score must be float32"):
            pipeline.flow_gate(f2, bad)
    for kw, word in (({"lo": NAN}, "lo"), ({"hi": NAN}, "hi"), ({"lo": "0"}, "lo"), ({"hi": None}, "hi"), ({"lo": 2.0, "hi": 1.0}, "lo=2 is above hi=1")):
        with pytest.raises(ValueError, match="flow_gate: %s" % word):
            pipeline.flow_gate(f2, sc, **kw)
    # DiscreteFlow.confidence: its gate needs no object
    for kw, word in (({"mode": "global"}, "mode"), ({"mode": 0}, "mode"), ({"min_sep": -1}, "min_sep"), ({"min_sep": 1025}, "min_sep"),
                     ({"min_sep": 1.0}, "min_sep"), ({"thresh": NAN}, "thresh"), ({"thresh": "1"}, "thresh"),
                     ({"thresh": None, "sparse": True}, "sparse=True needs a thresh")):
        args = dict(dict(mode="local", min_sep=1, thresh=0.0), **kw)
        with pytest.raises(ValueError, match="confidence: %s" % word):
            pipeline._confidence_gate("confidence", **args)
    assert pipeline._confidence_gate("confidence", "data", 3, None) == (L.CONF_DATA, 3, -INF)
    assert pipeline._confidence_gate("confidence", "local", 0, INF, sparse=True) == (L.CONF_LOCAL, 0, INF)

    class Stub:
        pass
    with pytest.raises(ValueError, match="confidence: sparse=True needs a thresh"):
        pipeline.DiscreteFlow.confidence(Stub(), sparse=True)
    with pytest.raises(ValueError, match="confidence: mode"):
        pipeline.DiscreteFlow.confidence(Stub(), mode="chain")


def test_command_line_refusals(L, capsys, tmp_path, monkeypatch):
    flowio = pkg("flowio")
    assert flowio.margin_name(3, 0, 2) == "Margin slike 103 backward=0 posle 02 BCD.npy"
    bcd = runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="bcd_cli")
    a = bcd["parser"]().parse_args(["1", "0", "2"])
    assert (a.confidence, a.conf_mode, a.conf_sep) == (False, None, None)
    a = bcd["parser"]().parse_args(["1", "0", "2", "--confidence", "--conf-mode", "data", "--conf-sep", "0"])
    assert pkg("labelconf").from_args(bcd["parser"](), a) == ("data", 0)
    for tail in (["--conf-mode", "data"], ["--conf-sep", "1"], ["--confidence", "--conf-mode", "chain"], ["--confidence", "--conf-sep", "-1"],
                 ["--confidence", "--conf-sep", "1025"], ["--confidence", "--conf-sep", "x"], ["--confidence", "1"]):
        with pytest.raises(SystemExit) as e:
            bcd["main"](["1", "0", "2"] + tail)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, tail
    rb = pkg("run_batch")
    a = rb.parser().parse_args([])
    assert (a.confidence, a.conf_mode, a.conf_sep) == (None, None, None) and pkg("labelconf").from_args(rb.parser(), a) == ("local", 1)
    for argv in (["--confidence"], ["--confidence", "nan"], ["--confidence", "x"], ["--conf-mode", "data"], ["--conf-sep", "1"],
                 ["--confidence", "1", "--conf-mode", "chain"], ["--confidence", "1", "--conf-sep", "1025"],
                 ["--confidence", "1", "--conf-sep", "1.5"]):
        with pytest.raises(SystemExit) as e:
            rb.main(argv)
        assert e.value.code == 2 and "--conf" in capsys.readouterr().err, argv
    spz = pkg("spremiZaEpic")
    six = ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"]
    for tail in (["--margin"], ["--margin", "m.npy"], ["--margin", "m.npy", "nan"], ["--margin", "m.npy", "x"]):
        assert spz.main(six + tail) == 2 and "--margin needs FILE and T" in capsys.readouterr().err, tail
    assert spz.take_margin(six + ["--margin", "m.npy", "-inf", "--gpu-epic"]) == (six + ["--gpu-epic"], ("m.npy", -INF))
    assert spz.take_margin(six) == (six, None)
    # in its place only: after --segments, before --gpu-epic
    assert spz.main(six + ["--gpu-epic", "--margin", "m.npy", "1"]) == 2
    assert spz.main(six + ["--margin", "m.npy", "1", "--segments", "3", "1"]) == 2
    capsys.readouterr()
    # a margin file that does not fit the flow: status 2 before any device is touched
    monkeypatch.chdir(tmp_path)
    np.save("f.npy", np.zeros((6, 9, 2)))
    np.save("m64.npy", np.zeros((6, 9)))
    np.save("m.npy", np.zeros((6, 8), np.float32))
    assert spz.main(six + ["--margin", "m64.npy", "1"]) == 2 and "expected float32 (6, 9)" in capsys.readouterr().err
    assert spz.main(six + ["--margin", "m.npy", "1"]) == 2 and "expected float32 (6, 9)" in capsys.readouterr().err
    assert spz.main(six + ["--margin", "missing.npy", "1"]) == 2 and "--margin missing.npy" in capsys.readouterr().err
