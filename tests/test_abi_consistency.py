"""What dflow_flow_consistency refuses on the host, before anything is launched, what its Python wrapper and
PyramidFlow.run_pair refuse before any device is touched, and what the command lines refuse (CPU only; no compute calls here)."""
import os
import runpy
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

FWD, BWD, OF, OB, EF, EB, CNT = (4096 * k for k in range(1, 8))     # non-NULL, aligned stand-ins for device pointers
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_the_header_declares_it(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "int dflow_flow_consistency(" in header and "dflow_flow_consistency" in L.SYMBOLS
    assert "#define DFLOW_FBC_BILINEAR 1u" in header and L.FBC_BILINEAR == 1
    makefile = open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert "consistency.hip" in makefile


def test_rejections_before_any_launch(L):
    lib = L.lib()

    def call(h=436, w=1024, fwd=FWD, lf=0, bwd=BWD, lb=1, thresh=1.0, flags=0, of=OF, ob=OB, ef=EF, eb=EB, cnt=CNT):
        return lib.dflow_flow_consistency(h, w, fwd, lf, bwd, lb, thresh, flags, of, ob, ef, eb, cnt, None)
    cases = [({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"), ({"h": -1}, b"size"),
             ({"lf": 2}, b"layout"), ({"lf": -1}, b"layout"), ({"lb": 2}, b"layout"), ({"lb": -1}, b"layout"),
             ({"flags": 2}, b"flags"), ({"flags": 3}, b"flags"), ({"flags": 0x80000000}, b"flags"),
             ({"thresh": NAN}, b"thresh"), ({"thresh": INF}, b"thresh"), ({"thresh": -INF}, b"thresh"), ({"thresh": -1e-30}, b"thresh"),
             ({"fwd": None}, b"d_fwd"), ({"bwd": None}, b"d_bwd"), ({"of": None}, b"d_out_fwd"),
             ({"ob": None}, b"d_err_bwd needs d_out_bwd"),
             ({"fwd": FWD + 2}, b"d_fwd"), ({"bwd": BWD + 1}, b"d_bwd"), ({"of": OF + 3}, b"d_out_fwd"), ({"ob": OB + 2}, b"d_out_bwd"),
             ({"ef": EF + 1}, b"d_err_fwd"), ({"eb": EB + 2}, b"d_err_bwd"), ({"cnt": CNT + 2}, b"d_counts")]
    # any output equal to an input ...
    cases += [({out: inp}, b"same plane as an input") for out in ("of", "ob", "ef", "eb", "cnt") for inp in (FWD, BWD)]
    # ... or to another output
    outs = {"of": OF, "ob": OB, "ef": EF, "eb": EB, "cnt": CNT}
    cases += [({a: outs[b]}, b"two outputs") for a in outs for b in outs if a != b]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    assert call(h=9000) == -1 and b"dflow_flow_consistency" in lib.dflow_last_error(), "the error names the function"
    # forward only: the same refusals with the backward outputs NULL
    for kw, msg in (({"of": FWD}, b"same plane as an input"), ({"ef": OF}, b"two outputs"), ({"cnt": BWD}, b"same plane as an input"),
                    ({"eb": EB}, b"d_err_bwd needs d_out_bwd")):
        assert call(**dict(dict(ob=None, eb=None), **kw)) == -1 and msg in lib.dflow_last_error(), kw


def test_the_wrapper_checks_its_arguments_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    f2, f3 = np.zeros((20, 24, 2), np.float32), np.zeros((20, 24, 3), np.float32)
    for bad in (f2.astype(np.float64), f2[0], np.zeros((20, 24, 4), np.float32), np.zeros((20, 24, 1), np.float32)):
        with pytest.raises(ValueError, match="flow_consistency: fwd must be float32"):
            pipeline.flow_consistency(bad, f2, 1.0)
        with pytest.raises(ValueError, match="flow_consistency: bwd must be float32"):
            pipeline.flow_consistency(f3, bad, 1.0)
    for bad in (f2[:19], f3[:, :23]):
        with pytest.raises(ValueError, match="flow_consistency: bwd must be float32"):
            pipeline.flow_consistency(f2, bad, 1.0)
    for thresh in (NAN, INF, -1.0):
        with pytest.raises(ValueError, match="flow_consistency: thresh"):
            pipeline.flow_consistency(f2, f3, thresh)


def test_gate_refusals(L, monkeypatch):
    pipeline = pkg("pipeline")
    pf = object.__new__(pipeline.PyramidFlow)                 # no device: the refusals come before the first call
    pf.levels = []
    with pytest.raises(ValueError, match="gate needs pair=True"):
        pf.coarse_prior(None, 2, gate=1.0)
    for gate in (NAN, INF, -0.5):
        with pytest.raises(ValueError, match="run_pair: gate"):
            pf.run_pair(None, None, 2, gate=gate)


def test_command_line_refusals(L, monkeypatch, capsys):
    spz = pkg("spremiZaEpic")
    six = ["a.png", "b.png", "f.npy", "b.npy", "10", "canny"]
    # the token is taken directly after the six positional ones and nowhere else; everything else parses as before
    assert spz.take_natural(six + ["--natural-check"]) == (six, True)
    assert spz.take_natural(six + ["--natural-check", "--gpu-epic", "--refine"]) == (six + ["--gpu-epic", "--refine"], True)
    assert spz.take_natural(six) == (six, False) and spz.take_natural(six + ["--gpu-epic"]) == (six + ["--gpu-epic"], False)
    assert spz.parse(spz.take_natural(six + ["--natural-check", "--gpu-epic", "--prefilter"])[0]) == (six, True, True, False)
    for tail in (["--gpu-epic", "--natural-check"], ["--natural-check", "--natural-check"], ["--natural-check", "--refine"],
                 ["--gpu-epic", "--prefilter", "--natural-check"]):
        assert spz.main(six + tail) == 2, tail
    assert spz.main(six[:5] + ["--natural-check"]) == 2
    capsys.readouterr()
    rb = pkg("run_batch")
    assert rb.parser().parse_args([]).check == "reference" and rb.parser().parse_args(["--check", "natural"]).check == "natural"
    with pytest.raises(SystemExit):
        rb.parser().parse_args(["--check", "transposed"])
    with pytest.raises(SystemExit):
        rb.parser().parse_args(["--gate", "2"])               # deliberately not built
    cli = os.path.join(ROOT, PKG, "daisy i flann.py")
    base = ["daisy i flann.py", "3", "0", "1", "--synthetic", "40x48", "--cell", "5x6"]
    for extra in (["--gate", "2"], ["--pyramid", "1", "--gate", "2"], ["--pyramid", "2", "--gate", "-1"], ["--pyramid", "2", "--gate", "nan"],
                  ["--pyramid", "2", "--gate", "inf"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(SystemExit) as e:
            runpy.run_path(cli, run_name="__main__")
        assert e.value.code == 2 and "--gate T needs --pyramid" in capsys.readouterr().err, extra
