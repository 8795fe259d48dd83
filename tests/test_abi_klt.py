"""What dflow_klt_pyramid(_bytes), dflow_corners and dflow_klt_track (include/dflow_klt.h) refuse on the host, before anything is
launched, each with its status and its text (the formats of abi.hip's shared checks, in the order the header states); the size
function against the offset formula; what the pipeline wrappers refuse before any device is touched; and the source pins with
klt.hip present (CPU only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import klt_ref as R
from conftest import PKG, ROOT, pkg

BGR, PYR, PYR2, PIN, SIN, POUT, SOUT, ERR, BACK, CNT, N, RESP, MASK, OCC, RMAX = (4096 * k for k in range(1, 16))   # non-NULL, aligned stand-ins
NAN, INF = float("nan"), float("inf")
EINVAL = -1
NAMES = ("dflow_klt_pyramid_bytes", "dflow_klt_pyramid", "dflow_corners", "dflow_klt_track")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_the_binding_and_the_makefile_name_them(L):
    header = open(os.path.join(ROOT, "include", "dflow_klt.h")).read()
    main_header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    csrc = os.path.join(ROOT, PKG, "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "klt.hip" in make.split("SRCS :=")[1].split("\n")[0].split() and "../../include/dflow_klt.h" in make
    assert '#include "dflow.h"' in header
    handle = C.CDLL(L.LIB_PATH)
    assert tuple(L._SIGNATURES_KLT) == NAMES == L.SYMBOLS_KLT
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in zip(NAMES, (3, 6, 18, 21)):
        assert hasattr(handle, name) and name not in L.SYMBOLS and (name + "(") not in main_header
        restype, argtypes = L._SIGNATURES_KLT[name]
        proto = re.search(r"(size_t|int) %s\((.*?)\);" % name, bare, re.S)
        assert proto and len(argtypes) == nargs == len(proto.group(2).split(","))
        assert (restype is C.c_size_t) == (proto.group(1) == "size_t") == (name == "dflow_klt_pyramid_bytes")
        assert getattr(L.lib(), name).argtypes == argtypes and "d_ws" not in proto.group(2)
    for state, k in (("FLAT", 6), ("RESIDUAL", 7)):
        assert re.search(r"#define DFLOW_TRACK_%s %d\b" % (state, k), header) and getattr(L, "TRACK_" + state) == k == getattr(R, state)
    assert (R.LIVE, R.LEFT, R.INCONSISTENT) == (L.TRACK_LIVE, L.TRACK_LEFT, L.TRACK_INCONSISTENT)
    # the gates add no refusal text of their own to abi.hip
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("size_t dflow_klt_pyramid_bytes("):]
    assert all("int %s(" % n in gate for n in NAMES[1:]) and "dflow_set_error(" not in gate
    text = open(os.path.join(csrc, "klt.hip")).read()
    assert '#include "plane_ops.h"' in text and "asm" not in text and "block_count<" in text and "block_reduce<" in text
    P = pkg("pipeline")
    assert P.TRACK_STATES_KLT[6:] == ("flat", "residual") and len(P.KLT_TRACK_COUNTS) == 8 and len(P.CORNER_COUNTS) == 4


def test_the_source_pins_hold_with_klt_hip_present():
    csrc = os.path.join(ROOT, PKG, "csrc")
    import cli_pins
    import component_pins
    import fit_common_pins
    import wave_ops_pins
    wave_ops_pins.check(csrc)
    component_pins.check(csrc)
    fit_common_pins.check(csrc)
    cli_pins.check(os.path.join(ROOT, PKG))
    assert "def read_flow" not in open(os.path.join(ROOT, PKG, "klt.py")).read()


def test_pyramid_bytes_is_the_offset_formula(L):
    lib, P = L.lib(), pkg("pipeline")
    for h, w in ((1, 1), (3, 70), (33, 65), (96, 128), (436, 1024), (8192, 8192), (8191, 1)):
        for levels in range(1, 9):
            offs, total = R.level_offsets(h, w, levels)
            assert lib.dflow_klt_pyramid_bytes(h, w, levels) == total == P.klt_pyramid_len(h, w, levels)
    for (h, w, levels), msg in (((0, 5, 3), "image size 5x0 outside [1,8192]"), ((5, 8193, 3), "image size 8193x5 outside [1,8192]"),
                                ((5, 5, 0), "levels=0 outside [1,8]"), ((5, 5, 9), "levels=9 outside [1,8]"),
                                ((0, 5, 0), "image size 5x0 outside [1,8192]")):
        assert lib.dflow_klt_pyramid_bytes(h, w, levels) == 0 and lib.dflow_last_error().decode() == "dflow_klt_pyramid_bytes: " + msg


def in_order(lib, call, order, words):
    """Each refusal wins over every one after it."""
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (i, kw, lib.dflow_last_error())


def exact(lib, call, fn, cases):
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())


def test_klt_pyramid_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(h=37, w=53, levels=3, bgr=BGR, pyr=PYR):
        return lib.dflow_klt_pyramid(h, w, levels, bgr, pyr, None)
    exact(lib, call, "dflow_klt_pyramid: ",
          [({"h": 0}, "image size 53x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x37 outside [1,8192]"),
           ({"levels": 0}, "levels=0 outside [1,8]"), ({"levels": 9}, "levels=9 outside [1,8]"), ({"bgr": None}, "d_bgr is NULL"),
           ({"pyr": None}, "d_pyr is NULL"), ({"bgr": BGR + 2}, "d_bgr is not 4-byte aligned"), ({"pyr": PYR + 1}, "d_pyr is not 4-byte aligned"),
           ({"pyr": BGR}, "d_pyr is the same plane as d_bgr")])
    in_order(lib, call, [{"h": 0}, {"levels": 0}, {"bgr": None}, {"pyr": None}],
             ["image size", "levels=", "d_bgr is NULL", "d_pyr is NULL"])
    in_order(lib, call, [{"w": 0}, {"levels": 9}, {"bgr": BGR + 2}, {"pyr": BGR + 2}], ["image size", "levels=", "d_bgr is not 4", "d_pyr is not 4"])
    assert call(bgr=BGR + 4, pyr=BGR + 4) == EINVAL and b"d_pyr is the same plane as d_bgr" in lib.dflow_last_error()


def test_corners_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(h=37, w=53, pyr=PYR, rc=2, md=4, border=4, q=0.01, mr=0.0, cap=100, pos=PIN, state=SIN, n=N, resp=RESP, mask=MASK, occ=OCC,
             rmax=RMAX, cnt=CNT):
        return lib.dflow_corners(h, w, pyr, rc, md, border, q, mr, cap, pos, state, n, resp, mask, occ, rmax, cnt, None)
    fn = "dflow_corners: "
    cases = [({"h": 8193}, "image size 53x8193 outside [1,8192]"), ({"w": 0}, "image size 0x37 outside [1,8192]"),
             ({"rc": 0}, "rc=0 outside [1,7]"), ({"rc": 8}, "rc=8 outside [1,7]"), ({"md": 0}, "min_dist=0 outside [1,32]"),
             ({"md": 33}, "min_dist=33 outside [1,32]"), ({"border": -1}, "border=-1 outside [0,8192]"),
             ({"border": 8193}, "border=8193 outside [0,8192]"), ({"q": -0.5}, "quality=-0.5 must be finite and >= 0"),
             ({"q": NAN}, "quality=nan must be finite and >= 0"), ({"q": INF}, "quality=inf must be finite and >= 0"),
             ({"q": 1.5}, "quality=1.5 must be <= 1"), ({"mr": -1.0}, "min_response=-1 must be finite and >= 0"),
             ({"mr": NAN}, "min_response=nan must be finite and >= 0"), ({"cap": 0}, "cap=0 outside [1,67108864]"),
             ({"cap": (1 << 26) + 1}, "cap=67108865 outside [1,67108864]"), ({"pos": None}, "d_pos is NULL"), ({"state": None}, "d_state is NULL"),
             ({"n": None}, "d_n is NULL"), ({"occ": None}, "d_occ is NULL"), ({"pyr": None}, "d_pyr is NULL"), ({"resp": None}, "d_response is NULL"),
             ({"mask": None}, "d_mask is NULL"), ({"rmax": None}, "d_rmax is NULL"), ({"pos": PIN + 4}, "d_pos is not 8-byte aligned"),
             ({"state": SIN + 2}, "d_state is not 4-byte aligned"), ({"n": N + 1}, "d_n is not 4-byte aligned"),
             ({"resp": RESP + 2}, "d_response is not 4-byte aligned"), ({"rmax": RMAX + 2}, "d_rmax is not 4-byte aligned"),
             ({"cnt": CNT + 3}, "d_counts is not 4-byte aligned")]
    ins = [("d_pyr", PYR), ("d_pos", PIN), ("d_state", SIN), ("d_n", N)]
    outs = [("d_response", "resp", RESP), ("d_mask", "mask", MASK), ("d_occ", "occ", OCC), ("d_rmax", "rmax", RMAX), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(outs):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, q in ins + [(o[0], o[2]) for o in outs[:i]]]
    assert len(cases) == 30 + 4 + 5 + 6 + 7 + 8
    exact(lib, call, fn, cases)
    # d_occ stays: with all four planes of a set NULL there is none, and cap is not looked at
    in_order(lib, call, [{"h": 0}, {"rc": 0}, {"md": 0}, {"border": -1}, {"q": NAN}, {"mr": -1.0}, {"cap": 0}, {"pos": None}, {"state": None},
                         {"n": None}, {"pyr": None}, {"resp": None}, {"mask": None}, {"rmax": None}],
             ["image size", "rc=", "min_dist=", "border=", "quality=", "min_response=", "cap=", "d_pos is NULL", "d_state is NULL", "d_n is NULL",
              "d_pyr is NULL", "d_response is NULL", "d_mask is NULL", "d_rmax is NULL"])
    in_order(lib, call, [{"n": None}, {"occ": None}, {"pyr": None}], ["d_n is NULL", "d_occ is NULL", "d_pyr is NULL"])
    in_order(lib, call, [{"q": 2.0}, {"mr": INF}, {"cap": -1}, {"pos": PIN + 4}, {"state": SIN + 2}, {"cnt": CNT + 2}, {"resp": PYR}, {"cnt": RMAX}],
             ["quality=2 must be <= 1", "min_response=", "cap=", "d_pos is not 8", "d_state is not 4", "d_counts is not 4",
              "d_response is the same plane as d_pyr", "d_counts is the same plane as d_rmax"])
    # without a set cap is not looked at; the ends of the ranges pass: the next refusal in line is reported
    none = dict(pos=None, state=None, n=None, occ=None)
    assert call(cap=0, cnt=CNT + 2, **none) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    for kw in ({"rc": 1}, {"rc": 7}, {"md": 1}, {"md": 32}, {"border": 0}, {"border": 8192}, {"q": 0.0}, {"q": 1.0}, {"mr": 0.0}, {"cap": 1}, {"cap": 1 << 26}):
        assert call(cnt=CNT + 2, **kw) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error(), kw
    # one plane of a set alone asks for the others
    assert call(**dict(none, occ=OCC)) == EINVAL and lib.dflow_last_error().decode() == fn + "d_pos is NULL"
    assert call(**dict(none, n=N, cap=0)) == EINVAL and lib.dflow_last_error().decode() == fn + "cap=0 outside [1,67108864]"


def test_klt_track_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(h=37, w=53, levels=3, p1=PYR, p2=PYR2, cap=1000, pin=PIN, sin=SIN, r=7, iters=20, eps=0.01, me=1.0, mx=0.0, fb=0.5, flags=0,
             pout=POUT, sout=SOUT, err=ERR, back=BACK, cnt=CNT):
        return lib.dflow_klt_track(h, w, levels, p1, p2, cap, pin, sin, r, iters, eps, me, mx, fb, flags, pout, sout, err, back, cnt, None)
    fn = "dflow_klt_track: "
    cases = [({"h": 0}, "image size 53x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x37 outside [1,8192]"),
             ({"levels": 0}, "levels=0 outside [1,8]"), ({"levels": 9}, "levels=9 outside [1,8]"), ({"cap": 0}, "cap=0 outside [1,67108864]"),
             ({"cap": (1 << 26) + 1}, "cap=67108865 outside [1,67108864]"), ({"r": 0}, "r=0 outside [1,10]"), ({"r": 11}, "r=11 outside [1,10]"),
             ({"iters": 0}, "iters=0 outside [1,64]"), ({"iters": 65}, "iters=65 outside [1,64]"), ({"eps": 0.0}, "eps=0 must be finite and > 0"),
             ({"eps": -1.0}, "eps=-1 must be finite and > 0"), ({"eps": NAN}, "eps=nan must be finite and > 0"),
             ({"eps": INF}, "eps=inf must be finite and > 0"), ({"me": -1.0}, "min_eig=-1 must be finite and >= 0"),
             ({"me": NAN}, "min_eig=nan must be finite and >= 0"), ({"mx": -0.5}, "max_err=-0.5 must be finite and >= 0"),
             ({"mx": INF}, "max_err=inf must be finite and >= 0"), ({"fb": -1.0}, "fb=-1 must be finite and >= 0"),
             ({"fb": NAN}, "fb=nan must be finite and >= 0"), ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"p1": None}, "d_pyr1 is NULL"), ({"p2": None}, "d_pyr2 is NULL"), ({"pin": None}, "d_pos_in is NULL"),
             ({"sin": None}, "d_state_in is NULL"), ({"pout": None}, "d_pos_out is NULL"), ({"sout": None}, "d_state_out is NULL"),
             ({"pin": PIN + 4}, "d_pos_in is not 8-byte aligned"), ({"pout": POUT + 4}, "d_pos_out is not 8-byte aligned"),
             ({"back": BACK + 4}, "d_back is not 8-byte aligned"), ({"sin": SIN + 2}, "d_state_in is not 4-byte aligned"),
             ({"sout": SOUT + 3}, "d_state_out is not 4-byte aligned"), ({"err": ERR + 2}, "d_err is not 4-byte aligned"),
             ({"cnt": CNT + 1}, "d_counts is not 4-byte aligned")]
    ins = [("d_pyr1", PYR), ("d_pyr2", PYR2), ("d_pos_in", PIN), ("d_state_in", SIN)]
    outs = [("d_pos_out", "pout", POUT), ("d_state_out", "sout", SOUT), ("d_err", "err", ERR), ("d_back", "back", BACK), ("d_counts", "cnt", CNT)]
    allowed = {("d_pos_out", "d_pos_in"), ("d_state_out", "d_state_in")}
    for i, (name, kw, _) in enumerate(outs):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, q in ins + [(o[0], o[2]) for o in outs[:i]]
                  if (name, before) not in allowed]
    assert len(cases) == 35 + 3 + 4 + 6 + 7 + 8
    exact(lib, call, fn, cases)
    in_order(lib, call, [{"h": 0}, {"levels": 0}, {"cap": 0}, {"r": 0}, {"iters": 0}, {"eps": 0.0}, {"me": NAN}, {"mx": -1.0}, {"fb": INF},
                         {"flags": 4}, {"p1": None}, {"p2": None}, {"pin": None}, {"sin": None}, {"pout": None}, {"sout": None}],
             ["image size", "levels=", "cap=", "r=", "iters=", "eps=", "min_eig=", "max_err=", "fb=", "unknown flags", "d_pyr1 is NULL",
              "d_pyr2 is NULL", "d_pos_in is NULL", "d_state_in is NULL", "d_pos_out is NULL", "d_state_out is NULL"])
    in_order(lib, call, [{"flags": 2}, {"pin": PIN + 4}, {"pout": POUT + 4}, {"back": BACK + 4}, {"sin": SIN + 1}, {"cnt": CNT + 2}, {"sout": PYR},
                         {"cnt": BACK}],
             ["unknown flags", "d_pos_in is not 8", "d_pos_out is not 8", "d_back is not 8", "d_state_in is not 4", "d_counts is not 4",
              "d_state_out is the same plane as d_pyr1", "d_counts is the same plane as d_back"])
    # what passes the gate: the next refusal in line is reported.  One pyramid for both frames; no test, no backward pass; the
    # optional outputs left out; the set in place, with whatever follows it still checked against the inputs
    assert call(p2=PYR, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(mx=0.0, fb=0.0, me=0.0, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(err=None, back=None, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(pout=PIN, sout=SIN, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(pout=PIN, sout=SIN, err=PIN) == EINVAL and lib.dflow_last_error().decode() == fn + "d_err is the same plane as d_pos_in"
    assert call(pout=SIN, sout=SIN) == EINVAL and lib.dflow_last_error().decode() == fn + "d_pos_out is the same plane as d_state_in"
    for kw in ({"levels": 1}, {"levels": 8}, {"r": 1}, {"r": 10}, {"iters": 1}, {"iters": 64}, {"cap": 1}, {"cap": 1 << 26}):
        assert call(cnt=CNT + 2, **kw) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error(), kw


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    P = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    h, w, cap, levels = 20, 24, 50, 2
    img = np.zeros((h, w, 3), np.uint8)
    pyr = np.zeros(P.klt_pyramid_len(h, w, levels), np.uint8)
    pos, state = np.zeros((cap, 2), np.float32), np.zeros(cap, np.int32)
    for kw, word in (({"img": img[..., :2]}, "img must be uint8"), ({"img": img.astype(np.float32)}, "img must be uint8"),
                     ({"levels": 0}, "levels must be"), ({"levels": 9}, "levels must be"), ({"levels": 2.0}, "levels must be")):
        with pytest.raises(ValueError, match="klt_pyramid: %s" % word):
            P.klt_pyramid(**dict(dict(img=img), **kw))
    for kw, word in (({"h": 0}, "h must be"), ({"pyr": pyr[:h * w - 1]}, "pyr holds"), ({"pyr": pyr.astype(np.int8)}, "pyr must be uint8"),
                     ({"rc": 0}, "rc must be"), ({"rc": 8}, "rc must be"), ({"min_dist": 33}, "min_dist must be"), ({"border": -1}, "border must be"),
                     ({"quality": 1.5}, "quality must be"), ({"quality": NAN}, "quality must be"), ({"min_response": -1}, "min_response must be"),
                     ({"tracks": (pos[:, :1], state, 3)}, "pos must be float32"), ({"tracks": (pos, state[:-1], 3)}, "state must be int32"),
                     ({"tracks": (pos, state, 1.5)}, "n must be int32")):
        with pytest.raises(ValueError, match="corners: %s" % word):
            P.corners(**dict(dict(pyr=pyr, h=h, w=w), **kw))
    for kw, word in (({"w": 8193}, "w must be"), ({"levels": 0}, "levels must be"), ({"pyr1": pyr[:-1]}, "pyr1 holds"), ({"pyr2": pyr[:-1]}, "pyr2 holds"),
                     ({"pos": pos.astype(np.float64)}, "pos must be float32"), ({"state": state[:3]}, "state must be int32"), ({"r": 0}, "r must be"),
                     ({"r": 11}, "r must be"), ({"iters": 65}, "iters must be"), ({"eps": 0}, "eps must be"), ({"eps": NAN}, "eps must be"),
                     ({"min_eig": -1}, "min_eig must be"), ({"max_err": INF}, "max_err must be"), ({"fb": -0.5}, "fb must be")):
        with pytest.raises(ValueError, match="klt_track: %s" % word):
            P.klt_track(**dict(dict(pyr1=pyr, pyr2=pyr, h=h, w=w, levels=levels, pos=pos, state=state), **kw))
    with pytest.raises(ValueError, match="klt_sparse_flow: img2 must be uint8"):
        P.klt_sparse_flow(img, img[:-1])


def test_klt_track_hands_over_what_it_was_given(L, monkeypatch):
    import torch
    P = pkg("pipeline")
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda dev: "the stream")
    monkeypatch.setattr(P, "_device_of", lambda *tensors: torch.device("cpu"))
    h, w, cap, levels = 6, 10, 7, 2
    pyr1, pyr2 = (torch.zeros(P.klt_pyramid_len(h, w, levels), dtype=torch.uint8) for _ in range(2))
    pos, state = torch.zeros((cap, 2)), torch.zeros(cap, dtype=torch.int32)
    po, so = P.klt_track(pyr1, pyr2, h, w, levels, pos, state)
    (name, a), = calls
    assert name == "dflow_klt_track" and a == (h, w, levels, pyr1.data_ptr(), pyr2.data_ptr(), cap, pos.data_ptr(), state.data_ptr(), 7, 20,
                                               float(np.float32(0.01)), 1.0, 0.0, 0.5, 0, po.data_ptr(), so.data_ptr(), None, None, None,
                                               "the stream")
    assert po.data_ptr() != pos.data_ptr()
    del calls[:]
    po, so, err, cnt = P.klt_track(pyr1, pyr2, h, w, levels, pos, state, r=3, iters=5, eps=1, min_eig=0, max_err=4, fb=0, inplace=True, err=True,
                                   counts=True)
    assert calls[0][1] == (h, w, levels, pyr1.data_ptr(), pyr2.data_ptr(), cap, pos.data_ptr(), state.data_ptr(), 3, 5, 1.0, 0.0, 4.0, 0.0, 0,
                           pos.data_ptr(), state.data_ptr(), err.data_ptr(), None, cnt.data_ptr(), "the stream")
    assert po is pos and so is state and tuple(err.shape) == (cap,) and tuple(cnt.shape) == (8,) and cnt.dtype == torch.int32
    del calls[:]
    mask, resp, cnt = P.corners(pyr1, h, w, tracks=(pos, state, 3), response=True, counts=True)
    (name, a), = calls
    assert name == "dflow_corners" and a[:9] == (h, w, pyr1.data_ptr(), 2, 4, 4, float(np.float32(0.01)), 0.0, cap)
    assert a[9:11] == (pos.data_ptr(), state.data_ptr()) and a[12:14] == (resp.data_ptr(), mask.data_ptr()) and a[16:] == (cnt.data_ptr(), "the stream")
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w) == tuple(resp.shape) and tuple(cnt.shape) == (4,)
    del calls[:]
    mask = P.corners(pyr1, h, w)
    assert calls[0][1][8:12] == (0, None, None, None) and calls[0][1][14] is None and calls[0][1][16] is None


def test_trackset_refuses_corners_on_a_coarse_grid(L, monkeypatch):
    import torch
    P = pkg("pipeline")
    ts = P.TrackSet(12, 16, step=4, device="cpu")
    with pytest.raises(ValueError, match="TrackSet.seed_corners: the set must be built with step=1"):
        ts.seed_corners(torch.zeros(12 * 16, dtype=torch.uint8))
    ts = P.TrackSet(12, 16, step=1, device="cpu")
    with pytest.raises(ValueError, match="TrackSet.advance_klt: pyr1 holds 100 bytes"):
        ts.advance_klt(torch.zeros(100, dtype=torch.uint8), torch.zeros(100, dtype=torch.uint8))
    with pytest.raises(ValueError, match="TrackSet.advance_klt: counts is not an argument here"):
        ts.advance_klt(None, None, counts=True)
    with pytest.raises(ValueError, match="TrackSet.seed_corners: tracks is not an argument here"):
        ts.seed_corners(None, tracks=None)


def test_command_line_refusals(L, capsys, tmp_path, monkeypatch):
    cli = pkg("klt")
    monkeypatch.chdir(tmp_path)
    a = cli.parser().parse_args(["a.png", "b.png", "--out", "t.npz"])
    assert (a.images, a.levels, a.radius, a.iters, a.min_dist, a.quality, a.fb, a.max_err, a.reseed, a.cap, a.flow, a.epic, a.json) == (
        ["a.png", "b.png"], 3, 7, 20, 4, 0.01, 0.5, 0.0, False, None, None, None, False)
    base = ["a.png", "b.png", "--out", "t.npz"]
    for argv in (["a.png", "--out", "t.npz"], ["a.png", "b.png"], ["a.png", "b.png", "--out", "t.npy"], base + ["--levels", "0"],
                 base + ["--levels", "9"], base + ["--radius", "0"], base + ["--radius", "11"], base + ["--iters", "65"], base + ["--min-dist", "33"],
                 base + ["--quality", "1.5"], base + ["--quality", "nan"], base + ["--fb", "-1"], base + ["--max-err", "inf"], base + ["--cap", "0"],
                 base + ["--flow", "0", "2", "o.flo"], base + ["--flow", "0", "1"], base + ["--flow", "0", "1", "o.npy"], base + ["--epic", "o.npy"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, argv
    # unreadable or ill-fitting input: status 2 before any device is touched, and nothing is written
    np.save("a.npy", np.zeros((6, 9, 3), np.uint8))
    np.save("b.npy", np.zeros((6, 8, 3), np.uint8))
    np.save("bad.npy", np.zeros((6, 9), np.float32))
    assert cli.main(["missing.npy", "a.npy", "--out", "t.npz"]) == 2 and "klt:" in capsys.readouterr().err
    assert cli.main(["a.npy", "bad.npy", "--out", "t.npz"]) == 2 and "not a (H,W,3) uint8 image" in capsys.readouterr().err
    assert cli.main(["a.npy", "b.npy", "--out", "t.npz"]) == 2 and "a 8x6 image among 9x6 ones" in capsys.readouterr().err
    assert sorted(os.listdir(".")) == ["a.npy", "b.npy", "bad.npy"]
