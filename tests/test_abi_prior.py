"""What dflow_prior_proposals, dflow_flow_advance and its workspace function refuse on the host, before anything is launched,
and what their Python wrappers refuse before any device is touched (CPU only; no compute calls here)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import pkg

P = 4096                      # a non-NULL, aligned stand-in for every device pointer
Q = 8192                      # a second one, for the prior (it must differ from the state pointers)


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_flags_match_the_header(L):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dflow.h")).read()
    assert "#define DFLOW_PRIOR_SEED_LABELS 1u" in header and L.PRIOR_SEED_LABELS == 1
    assert "#define DFLOW_ADVANCE_NEGATE 1u" in header and L.ADVANCE_NEGATE == 1


def test_prior_proposals_rejections_before_any_launch(L):
    lib = L.lib()

    def call(fields=None, d1=P, d2=P, prior=Q, layout=1, stride=2, flags=1, prop=P, lc=P, npr=P, best=P, counts=None):
        p = L.default_params(436, 1024, 27, 64)
        for k, v in (fields or {}).items():
            setattr(p, k, v)
        return lib.dflow_prior_proposals(C.byref(p), d1, d2, prior, layout, stride, flags, prop, lc, npr, best, counts, None)
    # whatever dflow_check_params refuses
    for fields, msg in (({"knn": 4}, b"knn"), ({"window": 3}, b"window"), ({"maxnprop": 200}, b"maxnprop"),
                        ({"label_pitch": 150}, b"label_pitch"), ({"pich": 4}, b"image size"), ({"tpsi": 0}, b"tpsi"),
                        ({"flags": 64}, b"flags"), ({"tphi": float("nan")}, b"tphi")):
        assert call(fields) == -1 and msg in lib.dflow_last_error(), (fields, lib.dflow_last_error())
    assert lib.dflow_prior_proposals(None, P, P, Q, 1, 2, 1, P, P, P, P, None, None) == -1 and b"params" in lib.dflow_last_error()
    for kw, msg in (({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"),
                    ({"stride": -1}, b"stride"), ({"stride": 8193}, b"stride"),
                    ({"flags": 2}, b"flags"), ({"flags": 3}, b"flags"), ({"flags": 0x80000000}, b"flags"),
                    ({"d1": None}, b"d_descr1"), ({"d2": None}, b"d_descr2"), ({"prior": None}, b"d_prior"),
                    ({"prop": None}, b"d_proposals"), ({"lc": None}, b"d_lcosts"), ({"npr": None}, b"d_nprop"),
                    ({"best": None}, b"d_bestlabels"),
                    ({"d1": P + 8}, b"d_descr1"), ({"d2": P + 4}, b"d_descr2"), ({"prior": Q + 2}, b"d_prior"),
                    ({"prop": P + 4}, b"d_proposals"), ({"prop": P + 8}, b"d_proposals"), ({"lc": P + 2}, b"d_lcosts"),
                    ({"npr": P + 1}, b"d_nprop"), ({"best": P + 2}, b"d_bestlabels"), ({"counts": P + 2}, b"d_counts"),
                    ({"prior": P}, b"d_prior"), ({"prior": P + 16, "lc": P + 16}, b"d_prior"),
                    ({"prior": P + 32, "d2": P + 32}, b"d_prior"), ({"prior": P + 64, "counts": P + 64}, b"d_prior")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    # the error names the function
    assert call(stride=9000) == -1 and b"dflow_prior_proposals" in lib.dflow_last_error()


def test_flow_advance_workspace_bounds(L):
    fn = L.lib().dflow_flow_advance_workspace_bytes
    wsb = fn(436, 1024)
    assert wsb >= 436 * 1024 * 4 and fn(436, 1024) == wsb, "one uint32 per pixel, a fixed function of the size"
    assert 4 <= fn(1, 1) <= wsb <= fn(8192, 8192) < 8192 * 8192 * 4 + 4096
    for h, w in ((0, 8), (8, 0), (8193, 8), (8, 8193), (-1, 8), (8, -1)):
        assert fn(h, w) == 0 and b"size" in L.lib().dflow_last_error(), (h, w)


def test_flow_advance_rejections_before_any_launch(L):
    lib = L.lib()
    wsb = lib.dflow_flow_advance_workspace_bytes(436, 1024)

    def call(h=436, w=1024, flow=Q, layout=0, flags=0, out=P, counts=None, ws=P, ws_bytes=wsb):
        return lib.dflow_flow_advance(h, w, flow, layout, flags, out, counts, ws, ws_bytes, None)
    for kw, msg in (({"h": 0}, b"size"), ({"w": 0}, b"size"), ({"h": 8193}, b"size"), ({"w": 8193}, b"size"),
                    ({"layout": 2}, b"layout"), ({"layout": -1}, b"layout"), ({"flags": 2}, b"flags"), ({"flags": 0x80000001}, b"flags"),
                    ({"flow": None}, b"d_flow"), ({"out": None}, b"d_out"),
                    ({"flow": Q + 2}, b"d_flow"), ({"out": P + 1}, b"d_out"), ({"counts": P + 2}, b"d_counts"), ({"ws": P + 2}, b"d_ws"),
                    ({"out": Q}, b"same plane")):
        assert call(**kw) == -1 and msg in lib.dflow_last_error(), (kw, lib.dflow_last_error())
    for kw in ({"ws": None}, {"ws_bytes": wsb - 1}, {"ws_bytes": 0}, {"layout": 1, "flags": 1, "counts": P, "ws_bytes": 8}):
        assert call(**kw) == -2 and b"workspace" in lib.dflow_last_error(), kw
    # an argument error is reported before a workspace that is too small
    assert call(h=0, ws=None) == -1 and call(flags=4, ws_bytes=0) == -1 and call(out=Q, ws_bytes=0) == -1


def test_python_wrappers_check_their_arrays_before_any_cuda_use(L, monkeypatch):
    import torch
    pipeline = pkg("pipeline")

    def touched(*args, **kw):
        raise AssertionError("torch.cuda was used before the arguments were checked")
    for name in ("current_device", "current_stream", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touched)
    H, W = 40, 48
    good = np.zeros((H, W, 2), np.float32)
    bads = (good.astype(np.float64), good[0], np.concatenate([good, good], axis=-1))
    for bad in bads:
        with pytest.raises(ValueError, match="flow_advance: flow must be float32"):
            pipeline.flow_advance(bad)
    # a pass without its device state: the input gate comes before anything else is read
    df = object.__new__(pipeline.DiscreteFlow)
    df.p = L.default_params(H, W, 5, 6)
    for bad in bads + (np.zeros((H, W + 1, 2), np.float32), np.zeros((H + 1, W, 3), np.float32)):
        with pytest.raises(ValueError, match="prior_proposals: prior must be float32"):
            df.prior_proposals(bad)
    for stride in (-1, 8193):
        with pytest.raises(ValueError, match="prior_proposals: stride"):
            df.prior_proposals(good, stride=stride)
