"""The match pre-filter without a GPU: what the numpy restatement (epic_prefilter_ref.py) does with the designed inputs of
epic_prefilter_cases.py, the float32 yardstick of test_gpu_epic_prefilter.py, the command lines, and every rejection of the
C-ABI (validated before any HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import epic_prefilter_cases as PC
import epic_prefilter_ref as P
import epic_ref as ER
from conftest import ROOT, pkg


def test_planted_outliers_are_exactly_what_is_dropped():
    sp, e, bad, field = PC.planted()
    r = P.prefilter(sp, e, saliency_th=0)
    assert 40 < bad.sum() < 200 and np.array_equal(r["reason"] == P.CONSISTENCY, bad)
    inl = [d for s, d in r["dist"].items() if not bad.ravel()[s]]
    out = [d for s, d in r["dist"].items() if bad.ravel()[s]]
    assert max(inl) < 3.0 and min(out) > 10.0            # far from pref_th = 5 on either side
    want = sp.copy()
    want[bad] = 0
    assert r["out"].tobytes() == want.tobytes() and (r["reason"] == P.KEPT).sum() == ER.seed_mask(sp).sum() - bad.sum()
    # end to end: the dense EPE against the known field falls (the figures test_gpu_epic_prefilter.py records)
    epe = lambda s: float(np.sqrt(((ER.interpolate(s, e)["flow"] - field) ** 2).sum(-1)).mean())
    before, after = epe(sp), epe(r["out"])
    print("EPE %.4f -> %.4f" % (before, after))
    assert abs(before - 0.3785) < 1e-3 and after < 1e-4


def test_two_motions_geodesic_keeps_what_euclidean_drops():
    sp, e, band = PC.two_motions()
    H, W = e.shape
    r = P.prefilter(sp, e, saliency_th=0)
    assert not (r["reason"] == P.CONSISTENCY).any() and (r["reason"] == P.KEPT).sum() == H * (W - 1)
    # the same decision with the pref_nn Euclidean-nearest seeds, a flat pixel weighted like a flat geodesic step (2 units)
    flat = sp.reshape(-1, 3)
    seeds = np.flatnonzero(ER.seed_mask(sp).ravel())
    sy, sx = np.divmod(seeds, W)
    for x in (band - 1, band + 1):
        for y in range(0, H, 5):
            s = y * W + x
            d = np.hypot(sy - y, sx - x)
            near = [i for i in np.lexsort((seeds, d)) if seeds[i] != s][:25]
            w = np.exp(-0.8 * 2.0 * d[near] / 2000.0)
            eu, ev = (w * flat[seeds[near], 0]).sum() / w.sum(), (w * flat[seeds[near], 1]).sum() / w.sum()
            assert P.dropped(sp, s, eu, ev, 5.0) and r["reason"][y, x] == P.KEPT


def test_flat_region_loses_its_seeds_to_stage_a():
    img = PC.half_flat_image()
    H, W = img.shape[:2]
    sp, e = PC.random_field(H, W, 0.5, seed=6)
    r = P.prefilter(sp, e, img, saliency_th=0.045, pref_nn=0)
    seeds = ER.seed_mask(sp)
    left, right = np.s_[:, :W // 2 - 8], np.s_[:, W // 2 + 8:]
    assert seeds[left].sum() > 100 and (r["reason"][left][seeds[left]] == P.SALIENCY).all()
    assert seeds[right].sum() > 100 and (r["reason"][right][seeds[right]] == P.KEPT).all()
    assert not r["saliency"][left].any() and r["saliency"][right].min() > 1.0
    assert not r["out"][left].any() and r["out"][right].tobytes() == sp[right].tobytes()


def test_decisions_do_not_depend_on_an_order_and_skipped_stages():
    sp, e, bad, _ = PC.planted(H=24, W=30)
    r = P.prefilter(sp, e, saliency_th=0)
    # judged against the whole set at once: removing the dropped seeds and filtering again may drop more, never the same
    again = P.prefilter(r["out"], e, saliency_th=0)
    assert (again["reason"] == P.CONSISTENCY).sum() < (r["reason"] == P.CONSISTENCY).sum()
    off = P.prefilter(sp, e, saliency_th=0, pref_nn=0)
    assert off["out"].tobytes() == sp.tobytes() and not off["dist"] and off["saliency"] is None
    lone = np.zeros((5, 6, 3), np.float32)
    lone[2, 3] = (40.0, -40.0, 1.0)
    r = P.prefilter(lone, np.zeros((5, 6), np.float32), saliency_th=0)
    assert r["reason"][2, 3] == P.KEPT and r["estimate"][2, 3].tolist() == [40.0, -40.0]


def test_float32_yardstick_of_the_saliency():
    """Recomputes SAL_YARD of test_gpu_epic_prefilter.py: the largest float32-vs-float64 difference of the reference's saliency
    over every image the GPU tests use.  When the images or the reference change, this says so before any GPU run."""
    worst = 0.0
    for name, img in PC.saliency_images():
        d = float(np.abs(P.saliency(img, np.float32).astype(np.float64) - P.saliency(img)).max())
        worst = max(worst, d)
    src = open(os.path.join(ROOT, "tests", "test_gpu_epic_prefilter.py")).read()
    yard, factor = re.search(r"SAL_YARD, SAL_FACTOR = (\S+), (\d+)", src).groups()
    print("yardstick %.5e" % worst)
    assert factor == "4" and abs(worst - float(yard)) <= 1e-3 * float(yard), (worst, yard)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert yard.lower() in design.lower()


def test_command_lines():
    ef = pkg("epicflow")
    five = ["a", "b", "c", "d", "e"]
    assert ef.parse_prefilter(five) is None and ef.parse_prefilter(five + ["--refine", "-nw"]) is None
    argv = five + ["--prefilter", "-nn", "7"]
    assert ef.parse_args(argv) == (five, 7, 0.8, "LA") and ef.parse_prefilter(argv) == {}
    argv = five + ["--pref-nn", "12", "--refine", "--pref-th", "2.5", "--saliency-th", "0", "--pref-nn", "13"]
    assert ef.parse_args(argv) == (five, 100, 0.8, "LA") and ef.parse_refine(argv) == (True, None)
    assert ef.parse_prefilter(argv) == dict(pref_nn=13, pref_th=2.5, saliency_th=0.0)
    for extra in (["--pref-nn"], ["--pref-nn", "x"], ["--pref-nn", "256"], ["--pref-nn", "-1"], ["--pref-nn", "2.5"],
                  ["--pref-th", "-1"], ["--pref-th", "nan"], ["--saliency-th", "inf"], ["--saliency-th"], ["--prefiltered"],
                  ["-prefnn"], ["-prefnn", "25"]):
        with pytest.raises(ef.UsageError):
            ef.parse_args(five + extra)
    with pytest.raises(ef.UsageError, match="--prefilter") as ei:
        ef.parse_args(five + ["-prefnn", "25"])
    assert "not built" not in str(ei.value)
    assert ef.main(five + ["-prefnn", "25"]) == 2
    spz = pkg("spremiZaEpic")
    six = ["a.png", "b.png", "f.npy", "b.npy", "3", "canny"]
    for extra in (["--prefilter"], ["--prefilter", "--gpu-epic"], ["--gpu-epic", "--refine", "--prefilter"],
                  ["--gpu-epic", "--prefilter", "--prefilter"], ["--gpu-epic", "--prefilter", "--refine", "x"],
                  ["--gpu-epic", "--prefilter", "--other"], ["--refine"], ["--gpu-epic", "--other"]):
        assert spz.main(six + extra) == 2
    pipeline = pkg("pipeline")
    sp, e = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError, match="img1"):
        pipeline.epic_prefilter(sp, e, None, saliency_th=0.045)
    with pytest.raises(ValueError, match="sparse"):
        pipeline.epic_prefilter(sp[..., :2], e)


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_symbols_and_workspace(L):
    handle = C.CDLL(L.LIB_PATH)
    for name in ("dflow_epic_prefilter_workspace_bytes", "dflow_epic_prefilter", "dflow_epic_prefilter_last_stats"):
        assert hasattr(handle, name) and name in L.SYMBOLS
    lib = L.lib()
    a, b = lib.dflow_epic_prefilter_workspace_bytes(100, 100), lib.dflow_epic_prefilter_workspace_bytes(200, 200)
    assert lib.dflow_epic_prefilter_workspace_bytes(1, 1) > 0 and 3.5 * a < b < 4.5 * a          # linear in h*w
    assert lib.dflow_epic_workspace_bytes(100, 100) < a < lib.dflow_epic_workspace_bytes(100, 100) + 2 * 100 * 100
    for h, w in ((0, 5), (5, 0), (-1, 5), (8193, 5), (5, 8193)):
        assert lib.dflow_epic_prefilter_workspace_bytes(h, w) == 0 and b"image size" in lib.dflow_last_error()
    assert lib.dflow_epic_prefilter_workspace_bytes(8192, 8192) > 0
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "recalled, not checked against the binary" in header and "synchronises its stream" in header


def test_prefilter_rejects_bad_calls_before_any_launch(L):
    lib = L.lib()
    ws = lib.dflow_epic_prefilter_workspace_bytes(20, 30)
    nan, inf = float("nan"), float("inf")

    def call(h=20, w=30, bgr=1, sparse=1 << 20, edges=1 << 20, sal=0.045, nn=25, th=5.0, k=0.8, out=1 << 20, d_ws=1, wsb=None):
        rc = lib.dflow_epic_prefilter(h, w, bgr, sparse, edges, sal, nn, th, k, out, None, None, None, d_ws,
                                      ws if wsb is None else wsb, None)
        return rc, lib.dflow_last_error()

    refused = [(dict(h=0), b"image size"), (dict(w=8193), b"image size"), (dict(h=8193), b"image size"), (dict(w=0), b"image size")]
    refused += [(dict(nn=v), b"pref_nn") for v in (-1, 256, 1000)]
    refused += [(dict(sal=v), b"saliency_th") for v in (-1e-9, nan, inf, -inf)]
    refused += [(dict(th=v), b"pref_th") for v in (-1e-9, nan, inf, -inf)]
    refused += [(dict(k=v), b"k=") for v in (0.0, -1.0, nan, inf)]
    refused += [(dict(sparse=None), b"d_sparse_in"), (dict(edges=None), b"d_edges"), (dict(out=None), b"d_sparse_out"),
                (dict(bgr=None), b"d_bgr"), (dict(bgr=None, sal=1e-300), b"d_bgr")]
    for kw, msg in refused:
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    for kw in (dict(wsb=ws - 1), dict(d_ws=None), dict(wsb=0)):
        rc, err = call(**kw)
        assert rc == -2 and b"workspace" in err, (kw, rc, err)
    # the other side of every bound: the workspace check is the last one, so a boundary value with a workspace one byte
    # short comes back DFLOW_ENOSPC, not DFLOW_EINVAL; the image may be NULL exactly when saliency_th is 0
    for kw in (dict(h=1), dict(h=8192), dict(w=1), dict(w=8192), dict(nn=0), dict(nn=255), dict(sal=0.0), dict(sal=0.0, bgr=None),
               dict(sal=-0.0, bgr=None), dict(th=0.0), dict(sal=1e300), dict(th=1e300), dict(k=5e-324), dict(k=1e300)):
        need = lib.dflow_epic_prefilter_workspace_bytes(kw.get("h", 20), kw.get("w", 30))
        rc, err = call(wsb=need - 1, **kw)
        assert need > 0 and rc == -2 and b"workspace" in err, (kw, rc, err)
    # no call has run on this thread: the statistics say so instead of reporting stale numbers
    assert lib.dflow_epic_prefilter_last_stats(None, None) == -1 and b"no pre-filter" in lib.dflow_last_error()
