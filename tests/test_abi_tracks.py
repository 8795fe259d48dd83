"""What dflow_track_advance, dflow_track_seed and dflow_track_flow refuse on the host, before anything is launched, each with its
status and its text (the formats of abi.hip's shared checks, in the order the header states); what pipeline.track_advance,
track_seed, track_flow and TrackSet refuse before any device is touched; and what tracks.py refuses before it writes anything (CPU
only; no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FWD, BWD, PIN, SIN, POUT, SOUT, ERR, CNT, BIRTH, N, SCAN, MASK = (4096 * k for k in range(1, 13))       # non-NULL, aligned stand-ins
NAN, INF = float("nan"), float("inf")
EINVAL = -1
NAMES = ("dflow_track_advance", "dflow_track_seed", "dflow_track_flow")


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
    assert "tracks.hip" in open(os.path.join(csrc, "Makefile")).read().split("SRCS :=")[1].split("\n")[0].split()
    handle = C.CDLL(L.LIB_PATH)
    assert tuple(L._SIGNATURES_TRACKS) == NAMES
    for name, nargs in zip(NAMES, (17, 13, 11)):
        assert "int %s(" % name in header and name in L.SYMBOLS and hasattr(handle, name)
        assert name not in L._SIGNATURES and name not in L._SIGNATURES_SHARED_GATE
        restype, argtypes = L._SIGNATURES_TRACKS[name]
        proto = prototype(header, name)
        # no workspace: the binding holds no size_t, and it is as long as the prototype
        assert restype is C.c_int and C.c_size_t not in argtypes and len(argtypes) == nargs == len(proto.split(","))
        assert "size_t" not in proto and not re.search(r"\bd_ws\b", proto)
        assert getattr(L.lib(), name).argtypes == argtypes
    for k, state in enumerate(("FREE", "LIVE", "LEFT", "NOFLOW", "NOBACK", "INCONSISTENT")):
        assert re.search(r"#define DFLOW_TRACK_%s %d\b" % (state, k), header) and getattr(L, "TRACK_" + state) == k
    text = open(os.path.join(csrc, "tracks.hip")).read()
    assert "block_count_class<" in text and "flow_good(" in text and "asm" not in text and "__launch_bounds__(TRK_THREADS)" in text
    # the seed's rank and scan are plane_ops.h's, one definition each
    import component_pins
    component_pins.check(csrc)
    # and what they do inside a wave is wave_ops.h's
    import wave_ops_pins
    wave_ops_pins.check(csrc)
    # the gates add no refusal text of their own to abi.hip
    abi = open(os.path.join(csrc, "abi.hip")).read()
    gate = abi[abi.index("int dflow_track_advance("):abi.index("int dflow_remove_small_segments_host(")]
    assert "int dflow_track_seed(" in gate and "int dflow_track_flow(" in gate and "dflow_set_error(" not in gate
    import track_ref
    P = pkg("pipeline")
    for h, w, step in ((37, 53, 1), (37, 53, 4), (37, 53, 64), (67, 131, 2), (1100, 1100, 1), (8192, 8192, 1)):
        assert P.track_scan_len(h, w, step) == track_ref.scan_len(h, w, step)
    assert "gh*gw + ceil(gh*gw / 1024) + 1" in header


def in_order(lib, call, fn_name, order, words):
    """Each refusal wins over every one after it."""
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later)
        assert call(**kw) == EINVAL and words[i] in lib.dflow_last_error().decode(), (fn_name, i, kw, lib.dflow_last_error())


def test_track_advance_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(h=37, w=53, fwd=FWD, lf=0, bwd=BWD, lb=1, cap=1000, pin=PIN, sin=SIN, rel=0.01, abs=0.5, flags=0, pout=POUT, sout=SOUT,
             err=ERR, cnt=CNT):
        return lib.dflow_track_advance(h, w, fwd, lf, bwd, lb, cap, pin, sin, rel, abs, flags, pout, sout, err, cnt, None)
    fn = "dflow_track_advance: "
    cases = [({"h": 0}, "image size 53x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x37 outside [1,8192]"),
             ({"lf": 2}, "unknown layout_fwd 2"), ({"lf": -1}, "unknown layout_fwd -1"), ({"lb": 2}, "unknown layout_bwd 2"),
             ({"cap": 0}, "cap=0 outside [1,67108864]"), ({"cap": (1 << 26) + 1}, "cap=67108865 outside [1,67108864]"),
             ({"rel": -1.0}, "rel=-1 must be finite and >= 0"), ({"rel": NAN}, "rel=nan must be finite and >= 0"),
             ({"rel": INF}, "rel=inf must be finite and >= 0"), ({"abs": -0.5}, "abs=-0.5 must be finite and >= 0"),
             ({"abs": NAN}, "abs=nan must be finite and >= 0"), ({"abs": INF}, "abs=inf must be finite and >= 0"),
             ({"flags": 1}, "unknown flags 0x1"), ({"flags": 0x80000000}, "unknown flags 0x80000000"),
             ({"fwd": None}, "d_fwd is NULL"), ({"pin": None}, "d_pos_in is NULL"), ({"sin": None}, "d_state_in is NULL"),
             ({"pout": None}, "d_pos_out is NULL"), ({"sout": None}, "d_state_out is NULL"),
             ({"pin": PIN + 4}, "d_pos_in is not 8-byte aligned"), ({"pout": POUT + 4}, "d_pos_out is not 8-byte aligned"),
             ({"fwd": FWD + 2}, "d_fwd is not 4-byte aligned"), ({"bwd": BWD + 1}, "d_bwd is not 4-byte aligned"),
             ({"sin": SIN + 2}, "d_state_in is not 4-byte aligned"), ({"sout": SOUT + 3}, "d_state_out is not 4-byte aligned"),
             ({"err": ERR + 2}, "d_err is not 4-byte aligned"), ({"cnt": CNT + 1}, "d_counts is not 4-byte aligned")]
    ins = [("d_fwd", FWD), ("d_bwd", BWD), ("d_pos_in", PIN), ("d_state_in", SIN)]
    outs = [("d_pos_out", "pout", POUT), ("d_state_out", "sout", SOUT), ("d_err", "err", ERR), ("d_counts", "cnt", CNT)]
    allowed = {("d_pos_out", "d_pos_in"), ("d_state_out", "d_state_in")}
    for i, (name, kw, _) in enumerate(outs):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, q in ins + [(o[0], o[2]) for o in outs[:i]]
                  if (name, before) not in allowed]
    assert len(cases) == 28 + 3 + 4 + 6 + 7
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    in_order(lib, call, fn, [{"h": 0}, {"lf": 9}, {"lb": 9}, {"cap": 0}, {"rel": NAN}, {"abs": -1.0}, {"flags": 4}, {"fwd": None}, {"pin": None},
                             {"sin": None}, {"pout": None}, {"sout": None}, {"pin": PIN + 4}, {"pout": POUT + 4}, {"fwd": FWD + 1},
                             {"cnt": CNT + 2}, {"sout": FWD}, {"cnt": ERR}],
             ["image size", "layout_fwd", "layout_bwd", "cap=", "rel=", "abs=", "unknown flags", "d_fwd is NULL", "d_pos_in is NULL",
              "d_state_in is NULL", "d_pos_out is NULL", "d_state_out is NULL", "d_pos_in is not 8", "d_pos_out is not 8", "d_fwd is not 4",
              "d_counts is not 4", "d_state_out is the same plane as d_fwd", "d_counts is the same plane as d_err"])
    # what passes the gate: the next refusal in line is reported.  Without d_bwd its layout is not looked at; zero tolerances; the
    # set in place, with whatever follows it still checked against the inputs
    assert call(bwd=None, lb=7, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(rel=0.0, abs=0.0, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(pout=PIN, sout=SIN, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()
    assert call(pout=PIN, sout=SIN, err=PIN) == EINVAL and lib.dflow_last_error().decode() == fn + "d_err is the same plane as d_pos_in"
    assert call(pout=PIN, sout=PIN) == EINVAL and lib.dflow_last_error().decode() == fn + "d_state_out is the same plane as d_pos_in"
    assert call(pout=SIN, sout=SIN) == EINVAL and lib.dflow_last_error().decode() == fn + "d_pos_out is the same plane as d_state_in"
    assert call(err=None, cnt=FWD) == EINVAL and lib.dflow_last_error().decode() == fn + "d_counts is the same plane as d_fwd"


def test_track_seed_rejections_status_text_and_order(L):
    lib = L.lib()

    def call(h=37, w=53, cap=1000, step=4, frame=0, mask=MASK, pos=PIN, state=SIN, birth=BIRTH, n=N, scan=SCAN, cnt=CNT):
        return lib.dflow_track_seed(h, w, cap, step, frame, mask, pos, state, birth, n, scan, cnt, None)
    fn = "dflow_track_seed: "
    cases = [({"h": 8193}, "image size 53x8193 outside [1,8192]"), ({"w": 0}, "image size 0x37 outside [1,8192]"),
             ({"cap": 0}, "cap=0 outside [1,67108864]"), ({"cap": -5}, "cap=-5 outside [1,67108864]"),
             ({"cap": (1 << 26) + 1}, "cap=67108865 outside [1,67108864]"),
             ({"step": 0}, "step=0 outside [1,256]"), ({"step": 257}, "step=257 outside [1,256]"),
             ({"pos": None}, "d_pos is NULL"), ({"state": None}, "d_state is NULL"), ({"birth": None}, "d_birth is NULL"),
             ({"n": None}, "d_n is NULL"), ({"scan": None}, "d_scan is NULL"),
             ({"pos": PIN + 4}, "d_pos is not 8-byte aligned"), ({"state": SIN + 2}, "d_state is not 4-byte aligned"),
             ({"birth": BIRTH + 1}, "d_birth is not 4-byte aligned"), ({"n": N + 2}, "d_n is not 4-byte aligned"),
             ({"scan": SCAN + 3}, "d_scan is not 4-byte aligned"), ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    planes = [("d_mask", "mask", MASK), ("d_pos", "pos", PIN), ("d_state", "state", SIN), ("d_birth", "birth", BIRTH), ("d_n", "n", N),
              ("d_scan", "scan", SCAN), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(planes[1:], 1):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, _, q in planes[:i]]
    assert len(cases) == 18 + 1 + 2 + 3 + 4 + 5 + 6
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    in_order(lib, call, fn, [{"h": 0}, {"cap": 0}, {"step": 0}, {"pos": None}, {"state": None}, {"birth": None}, {"n": None}, {"scan": None},
                             {"pos": PIN + 4}, {"cnt": CNT + 1}, {"state": MASK}, {"cnt": SCAN}],
             ["image size", "cap=", "step=", "d_pos is NULL", "d_state is NULL", "d_birth is NULL", "d_n is NULL", "d_scan is NULL",
              "d_pos is not 8", "d_counts is not 4", "d_state is the same plane as d_mask", "d_counts is the same plane as d_scan"])
    # any frame number, no mask and the ends of the ranges pass the gate: the next refusal in line is reported
    for kw in ({"frame": -(1 << 31)}, {"frame": (1 << 31) - 1}, {"mask": None}, {"step": 1}, {"step": 256}, {"cap": 1}, {"cap": 1 << 26}):
        assert call(cnt=CNT + 2, **kw) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error(), kw


def test_track_flow_rejections_status_text_and_order(L):
    lib = L.lib()
    PA, SA, PB, SB, OWN, OUT = PIN, SIN, POUT, SOUT, SCAN, ERR

    def call(h=37, w=53, cap=1000, pa=PA, sa=SA, pb=PB, sb=SB, own=OWN, out=OUT, cnt=CNT):
        return lib.dflow_track_flow(h, w, cap, pa, sa, pb, sb, own, out, cnt, None)
    fn = "dflow_track_flow: "
    cases = [({"h": 0}, "image size 53x0 outside [1,8192]"), ({"w": 8193}, "image size 8193x37 outside [1,8192]"),
             ({"cap": 0}, "cap=0 outside [1,67108864]"), ({"cap": (1 << 26) + 1}, "cap=67108865 outside [1,67108864]"),
             ({"pa": None}, "d_pos_a is NULL"), ({"sa": None}, "d_state_a is NULL"), ({"pb": None}, "d_pos_b is NULL"),
             ({"sb": None}, "d_state_b is NULL"), ({"own": None}, "d_owner is NULL"), ({"out": None}, "d_out is NULL"),
             ({"pa": PA + 4}, "d_pos_a is not 8-byte aligned"), ({"pb": PB + 4}, "d_pos_b is not 8-byte aligned"),
             ({"sa": SA + 2}, "d_state_a is not 4-byte aligned"), ({"sb": SB + 1}, "d_state_b is not 4-byte aligned"),
             ({"own": OWN + 2}, "d_owner is not 4-byte aligned"), ({"out": OUT + 3}, "d_out is not 4-byte aligned"),
             ({"cnt": CNT + 2}, "d_counts is not 4-byte aligned")]
    ins = [("d_pos_a", PA), ("d_state_a", SA), ("d_pos_b", PB), ("d_state_b", SB)]
    outs = [("d_owner", "own", OWN), ("d_out", "out", OUT), ("d_counts", "cnt", CNT)]
    for i, (name, kw, _) in enumerate(outs):
        cases += [({kw: q}, "%s is the same plane as %s" % (name, before)) for before, q in ins + [(o[0], o[2]) for o in outs[:i]]]
    assert len(cases) == 17 + 4 + 5 + 6
    for kw, msg in cases:
        assert call(**kw) == EINVAL and lib.dflow_last_error().decode() == fn + msg, (kw, lib.dflow_last_error())
    in_order(lib, call, fn, [{"w": 0}, {"cap": 0}, {"pa": None}, {"sa": None}, {"pb": None}, {"sb": None}, {"own": None}, {"out": None},
                             {"pa": PA + 4}, {"pb": PB + 4}, {"cnt": CNT + 1}, {"own": SB}, {"cnt": OUT}],
             ["image size", "cap=", "d_pos_a is NULL", "d_state_a is NULL", "d_pos_b is NULL", "d_state_b is NULL", "d_owner is NULL",
              "d_out is NULL", "d_pos_a is not 8", "d_pos_b is not 8", "d_counts is not 4", "d_owner is the same plane as d_state_b",
              "d_counts is the same plane as d_out"])
    # the two snapshots may be one
    assert call(pb=PA, sb=SA, cnt=CNT + 2) == EINVAL and b"d_counts is not 4" in lib.dflow_last_error()


def test_the_wrappers_check_their_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    P = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    h, w, cap = 20, 24, 50
    pos, state, birth = np.zeros((cap, 2), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    fwd = np.zeros((h, w, 3), np.float32)
    for kw, word in (({"h": 0}, "h must be"), ({"w": 8193}, "w must be"), ({"h": 20.0}, "h must be"),
                     ({"pos": pos.astype(np.float64)}, "pos must be float32"), ({"pos": np.zeros((cap, 3), np.float32)}, "pos must be float32"),
                     ({"pos": np.zeros((0, 2), np.float32), "state": state[:0]}, "a track set holds 1 to 2\\^26 slots"),
                     ({"state": state[:-1]}, "state must be int32"), ({"state": state.astype(np.int64)}, "state must be int32"),
                     ({"fwd": fwd[:-1]}, "fwd must be float32"), ({"fwd": np.zeros((h, w, 4), np.float32)}, "fwd must be float32"),
                     ({"bwd": fwd[:, :-1]}, "bwd must be float32"), ({"rel": NAN}, "rel must be finite"), ({"rel": -1}, "rel must be finite"),
                     ({"abs": INF}, "abs must be finite"), ({"abs": "1"}, "abs must be finite")):
        args = dict(dict(h=h, w=w, pos=pos, state=state, fwd=fwd), **kw)
        with pytest.raises(ValueError, match="track_advance: %s" % word):
            P.track_advance(**args)
    for kw, word in (({"h": -1}, "h must be"), ({"birth": birth[:-1]}, "birth must be int32"), ({"step": 0}, "step must be"),
                     ({"step": 257}, "step must be"), ({"step": 2.0}, "step must be"), ({"frame": 1 << 31}, "frame must be"),
                     ({"n": np.zeros(2, np.int32)}, "n must be int32"), ({"n": 1.5}, "n must be int32"),
                     ({"mask": np.zeros((h, w), bool)}, "mask must be uint8"), ({"mask": np.zeros((h, w + 1), np.uint8)}, "mask must be uint8"),
                     ({"scan": np.zeros(1000, np.int32)}, "scan must be"), ({"pos": pos[:, :1]}, "pos must be float32")):
        args = dict(dict(h=h, w=w, pos=pos, state=state, birth=birth, n=0), **kw)
        with pytest.raises(ValueError, match="track_seed: %s" % word):
            P.track_seed(**args)
    for kw, word in (({"w": 0}, "w must be"), ({"pos_a": pos[:, 0]}, "pos_a must be float32"), ({"state_a": state[:3]}, "state_a must be int32"),
                     ({"pos_b": pos[:-1]}, "pos_b must be float32"), ({"state_b": state.astype(np.uint8)}, "state_b must be int32")):
        args = dict(dict(h=h, w=w, pos_a=pos, state_a=state, pos_b=pos, state_b=state), **kw)
        with pytest.raises(ValueError, match="track_flow: %s" % word):
            P.track_flow(**args)
    for kw, word in (({"h": 0}, "h must be"), ({"step": 0}, "step must be"), ({"cap": 0}, "cap must be"), ({"cap": (1 << 26) + 1}, "cap must be"),
                     ({"cap": 10.0}, "cap must be"), ({"rel": -1.0}, "rel must be"), ({"abs": NAN}, "abs must be")):
        with pytest.raises(ValueError, match="TrackSet: %s" % word):
            P.TrackSet(**dict(dict(h=h, w=w), **kw))
    assert P.TRACK_STATES == ("free", "live", "left", "noflow", "noback", "inconsistent")
    assert P.TRACK_ADVANCE_COUNTS == ("live", "left", "noflow", "noback", "inconsistent", "not_live")
    assert P.TRACK_SEED_COUNTS == ("covered", "seedable", "seeded", "dropped") and P.TRACK_FLOW_COUNTS == ("set", "lost", "no_part")


def test_track_advance_hands_over_what_it_was_given(L, monkeypatch):
    import torch
    P = pkg("pipeline")
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(L, "stream", lambda dev: "the stream")
    monkeypatch.setattr(P, "_device_of", lambda *tensors: torch.device("cpu"))
    h, w, cap = 6, 10, 7
    pos, state = torch.zeros((cap, 2)), torch.zeros(cap, dtype=torch.int32)
    f2, f3 = torch.zeros((h, w, 2)), torch.zeros((h, w, 3))
    po, so = P.track_advance(h, w, pos, state, f3)
    (name, a), = calls
    assert name == "dflow_track_advance" and a == (h, w, f3.data_ptr(), L.EVAL_UVV, None, 0, cap, pos.data_ptr(), state.data_ptr(),
                                                   float(np.float32(0.01)), 0.5, 0, po.data_ptr(), so.data_ptr(), None, None, "the stream")
    assert po.data_ptr() != pos.data_ptr() and po.shape == pos.shape and so.dtype == torch.int32
    del calls[:]
    po, so, err, cnt = P.track_advance(h, w, pos, state, f3, f2, rel=0, abs=2, inplace=True, err=True, counts=True)
    assert calls[0][1] == (h, w, f3.data_ptr(), L.EVAL_UVV, f2.data_ptr(), L.EVAL_DYDX, cap, pos.data_ptr(), state.data_ptr(), 0.0, 2.0, 0,
                           pos.data_ptr(), state.data_ptr(), err.data_ptr(), cnt.data_ptr(), "the stream")
    assert po is pos and so is state and tuple(err.shape) == (cap,) and tuple(cnt.shape) == (6,) and cnt.dtype == torch.int32


def test_command_line_refusals(L, capsys, tmp_path, monkeypatch):
    cli = pkg("tracks")
    monkeypatch.chdir(tmp_path)
    a = cli.parser().parse_args(["f0.flo", "f1.flo", "--out", "t.npz"])
    assert (a.forward, a.backward, a.step, a.reseed, a.rel, a.abs, a.cap, a.flow, a.json) == (["f0.flo", "f1.flo"], None, 4, False, 0.01, 0.5,
                                                                                               None, None, False)
    for argv in (["f0.flo"], ["--out", "t.npz"], ["f0.flo", "--out", "t.npy"], ["f0.flo", "f1.flo", "--backward", "b0.flo", "--out", "t.npz"],
                 ["f0.flo", "--out", "t.npz", "--step", "0"], ["f0.flo", "--out", "t.npz", "--step", "257"],
                 ["f0.flo", "--out", "t.npz", "--rel", "nan"], ["f0.flo", "--out", "t.npz", "--rel", "-1"],
                 ["f0.flo", "--out", "t.npz", "--abs", "inf"], ["f0.flo", "--out", "t.npz", "--cap", "0"],
                 ["f0.flo", "--out", "t.npz", "--cap", str((1 << 26) + 1)], ["f0.flo", "--out", "t.npz", "--flow", "0", "1"],
                 ["f0.flo", "--out", "t.npz", "--flow", "0", "2", "o.flo"], ["f0.flo", "--out", "t.npz", "--flow", "-1", "1", "o.flo"],
                 ["f0.flo", "--out", "t.npz", "--flow", "a", "1", "o.flo"], ["f0.flo", "--out", "t.npz", "--flow", "0", "1", "o.npy"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and "error:" in capsys.readouterr().err, argv
    # unreadable or ill-fitting input: status 2 before any device is touched, and nothing is written
    np.save("f0.npy", np.zeros((6, 9, 2), np.float32))
    np.save("f1.npy", np.zeros((6, 8, 2), np.float32))
    np.save("bad.npy", np.zeros((6, 9), np.float32))
    assert cli.main(["missing.flo", "--out", "t.npz"]) == 2 and "tracks:" in capsys.readouterr().err
    assert cli.main(["f0.txt", "--out", "t.npz"]) == 2 and "unsupported flow file" in capsys.readouterr().err
    assert cli.main(["bad.npy", "--out", "t.npz"]) == 2 and "expected an (H,W,2)" in capsys.readouterr().err
    assert cli.main(["f0.npy", "f1.npy", "--out", "t.npz"]) == 2 and "a 8x6 field among 9x6 ones" in capsys.readouterr().err
    assert cli.main(["f0.npy", "--backward", "f1.npy", "--out", "t.npz"]) == 2 and "f1.npy: a 8x6 field" in capsys.readouterr().err
    assert sorted(os.listdir(".")) == ["bad.npy", "f0.npy", "f1.npy"]
