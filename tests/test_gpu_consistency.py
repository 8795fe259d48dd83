"""dflow_flow_consistency on the device against its numpy definition (tests/consistency_ref.py), bit for bit: outputs, error
planes and counts; and the layers above it: pipeline.flow_consistency, PyramidFlow.run_pair with and without the gate against
the same run composed on the CPU, spremiZaEpic.py --natural-check, run_batch.py --check natural and the calls they issue.
Everything here needs a real MI355X: run with `pytest -m gpu`."""
import json
import os
import runpy
import sys

import numpy as np
import pytest

import consistency_ref as R
from call_log import BACK, BATCH_FLOWS, FRONT, record_calls
from conftest import PKG, ROOT, pkg

pytestmark = pytest.mark.gpu

# 45x35: the last wave and the last block are partial; 64x257: a row spans blocks
SMALL = [(1, 1), (2, 3), (7, 9), (45, 35)]
LAYOUTS = [("uvv", "uvv"), ("uvv", "dydx"), ("dydx", "uvv"), ("dydx", "dydx")]
CASES = [(s, lf, lb, mode, kind) for s in SMALL for lf, lb in LAYOUTS for mode in ("nearest", "bilinear") for kind in ("integer", "fractional")]
CASES += [((64, 257), lf, lb, mode, "fractional") for lf, lb in (("uvv", "dydx"), ("dydx", "uvv")) for mode in ("nearest", "bilinear")]
CASES += [((64, 257), "uvv", "uvv", "nearest", "integer")]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def crafted(h, w):
    """Vectors (y, x, V, U) that put a target on -1, 0, h-1 and h (and w likewise) exactly and a quarter pixel to either side,
    the ties of the nearest rounding, the ends of the int16 range and components that are not finite or overflow."""
    out = []
    for k, t in enumerate((-1.0, 0.0, h - 1.0, float(h))):
        for j, d in enumerate((-0.25, 0.0, 0.25)):
            y, x = (3 * k + j) % h, (5 * k + 2 * j + 1) % w
            out.append((y, x, t + d - y, 0.0))
    for k, t in enumerate((-1.0, 0.0, w - 1.0, float(w))):
        for j, d in enumerate((-0.25, 0.0, 0.25)):
            y, x = (4 * k + j + 1) % h, (7 * k + 3 * j) % w
            out.append((y, x, 0.5 if j == 1 else 0.0, t + d - x))
    specials = [(0.5, -0.5), (1.5, -1.5), (-0.5, 2.5), (-0.0, -0.0), (32767.4, 0.0), (0.0, 32767.5), (-32768.0, 0.0), (np.nan, 0.0),
                (0.0, np.inf), (-np.inf, 1.0), (3e38, 3e38), (-3e38, 1.0), (1e-30, -1e-30)]
    for k, (v, u) in enumerate(specials):
        out.append(((k * 11 + 2) % h, (k * 13 + 5) % w, v, u))
    return out


def fields(h, w, kind, seed):
    """[U,V,valid] fields: a forward one and a backward one that mostly undoes it, 30 % invalid pixels in either, and where
    the frame has room the crafted vectors in both."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    f = np.zeros((2, h, w, 3), np.float32)
    f[0, ..., :2] = rng.normal(0, 3.0, (h, w, 2))
    f[1, ..., :2] = -f[0, ..., :2] + rng.normal(0, 1.0, (h, w, 2))
    if kind == "integer":
        f[..., :2] = np.rint(f[..., :2])
    f[..., 2] = rng.random((2, h, w)) >= 0.3
    if h * w > 60 and kind == "fractional":
        for d in (0, 1):
            for y, x, v, u in crafted(h, w):
                y, x = (y, x) if d == 0 else (h - 1 - y, w - 1 - x)
                f[d, y, x] = (u, v, 1.0)
        f[1, h // 2, w // 2 - 1] = (3e38, -3e38, 1.0)                  # two large neighbours in a row: their difference overflows
        f[1, h // 2, w // 2] = (-3e38, 3e38, 1.0)
        f[0, h // 2, w // 2 - 1] = (0.5, 0.0, 1.0)
    return f[0], f[1]


def as_layout(f, layout):
    return f if layout == "uvv" else np.ascontiguousarray(f[..., 1::-1])


def same_bits(got, want, what):
    """Equal bit for bit, but for the payload and sign of a NaN, which IEEE 754 leaves open: a NaN must meet a NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


@pytest.mark.parametrize("size,lf,lb,mode,kind", CASES, ids=["%dx%d-%s-%s-%s-%s" % (c[0] + c[1:]) for c in CASES])
def test_matches_the_reference(torch_, size, lf, lb, mode, kind):
    h, w = size
    P = pkg("pipeline")
    fwd, bwd = fields(h, w, kind, 3)
    fwd, bwd = as_layout(fwd, lf), as_layout(bwd, lb)
    bil = mode == "bilinear"
    thresh = 4.0
    want = R.flow_consistency(fwd, bwd, thresh, R.BILINEAR if bil else 0, both=True)
    assert sum(want[4][:5]) == h * w and sum(want[4][5:]) == h * w
    if h * w > 1000 and lf == "uvv" and lb == "uvv":
        assert all(c > 0 for c in want[4]), want[4]
    got = P.flow_consistency(fwd, bwd, thresh, bilinear=bil, both=True, err=True, counts=True)
    assert len(got) == 5 and got[4].cpu().reshape(-1).tolist() == want[4]
    for g, wnt, what in zip(got[:4], want[:4], ("out_fwd", "out_bwd", "err_fwd", "err_bwd")):
        same_bits(g.cpu().numpy(), wnt, what)
    # forward only, from device tensors: the forward half of the same result
    one = P.flow_consistency(torch_.from_numpy(fwd).cuda(), torch_.from_numpy(bwd).cuda(), thresh, bilinear=bil, err=True, counts=True)
    assert len(one) == 3 and one[2].cpu().tolist() == want[4][:5]
    assert one[0].cpu().numpy().tobytes() == got[0].cpu().numpy().tobytes() and one[1].cpu().numpy().tobytes() == got[2].cpu().numpy().tobytes()
    # and the backward half is the single call with the roles swapped
    two = P.flow_consistency(bwd, fwd, thresh, bilinear=bil, err=True, counts=True)
    assert two[0].cpu().numpy().tobytes() == got[1].cpu().numpy().tobytes() and two[1].cpu().numpy().tobytes() == got[3].cpu().numpy().tobytes()
    assert two[2].cpu().tolist() == want[4][5:]
    # without the optional planes
    plain = P.flow_consistency(fwd, bwd, thresh, bilinear=bil)
    assert isinstance(plain, torch_.Tensor) and plain.cpu().numpy().tobytes() == got[0].cpu().numpy().tobytes()
    if kind == "integer":                                              # on integer fields bilinear equals nearest bit for bit
        other = P.flow_consistency(fwd, bwd, thresh, bilinear=not bil, both=True, err=True, counts=True)
        for a, b in zip(other, got):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_q13_discriminator(torch_, oracle):
    """Forward (0,+3) everywhere on 6x9, backward (0,-3): the check in image coordinates keeps the 6x6 pixels whose target is
    inside and calls the last 3 COLUMNS outside; the reference's check kills the last 3 ROWS.  dflow_fb_consistency takes no
    frame below 8 px, so at 6x9 the reference's side is the oracle's; at 8x11 both run on the device."""
    P = pkg("pipeline")
    for h, w in ((6, 9), (8, 11)):
        fwd, bwd = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
        fwd[..., 1], bwd[..., 1] = 3, -3
        for bil in (False, True):
            out, cnt = P.flow_consistency(fwd, bwd, 10, bilinear=bil, counts=True)
            out = out.cpu().numpy()
            assert out[:, :w - 3, 2].all() and not out[:, w - 3:].any() and (out[:, :w - 3, 0] == 3).all() and (out[:, :w - 3, 1] == 0).all()
            assert cnt.cpu().tolist() == [h * (w - 3), 0, 0, 3 * h, 0]
        if h < 8:
            s = oracle.fb_consistency(fwd.astype(np.float64), bwd.astype(np.float64), 10)
        else:
            s = P.fb_consistency(torch_.from_numpy(fwd).cuda(), torch_.from_numpy(bwd).cuda(), 10).cpu().numpy()
        assert s[:h - 3, :, 2].all() and not s[h - 3:, :, 2].any()
    # err == thresh is consistent
    f, b = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5, 3), np.float32)
    f[..., 2] = b[..., 2] = 1
    f[0, 0, :2], b[0, 3, :2] = (3, 0), (0, 4)
    out, err = P.flow_consistency(f, b, 5, err=True)
    assert out[0, 0].cpu().tolist() == [3, 0, 1] and err[0, 0].item() == 5
    assert P.flow_consistency(f, b, float(np.nextafter(np.float32(5), np.float32(0))))[0, 0].cpu().tolist() == [0, 0, 0]


def test_return_shapes(torch_):
    P = pkg("pipeline")
    h, w = 7, 9
    fwd, bwd = fields(h, w, "integer", 1)
    T = torch_.Tensor
    out = P.flow_consistency(fwd, bwd[..., 1::-1].copy(), 2)
    assert isinstance(out, T) and tuple(out.shape) == (h, w, 3) and out.dtype == torch_.float32 and out.is_cuda
    shapes = lambda r: [tuple(t.shape) for t in r]
    assert shapes(P.flow_consistency(fwd, bwd, 2, both=True)) == [(h, w, 3)] * 2
    assert shapes(P.flow_consistency(fwd, bwd, 2, err=True)) == [(h, w, 3), (h, w)]
    assert shapes(P.flow_consistency(fwd, bwd, 2, counts=True)) == [(h, w, 3), (5,)]
    assert shapes(P.flow_consistency(fwd, bwd, 2, both=True, counts=True)) == [(h, w, 3)] * 2 + [(2, 5)]
    r = P.flow_consistency(fwd, bwd, 2, bilinear=True, both=True, err=True, counts=True)
    assert shapes(r) == [(h, w, 3)] * 2 + [(h, w)] * 2 + [(2, 5)] and r[4].dtype == torch_.int32
    assert r[4].sum(dim=1).cpu().tolist() == [h * w, h * w]
    # it runs on torch's current stream
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        again = P.flow_consistency(fwd, bwd, 2)
    st.synchronize()
    assert again.cpu().numpy().tobytes() == P.flow_consistency(fwd, bwd, 2).cpu().numpy().tobytes()


# ---- PyramidFlow.run_pair
H, W, CH, CW, SEED = 40, 48, 5, 6, 7


PYRAMID_RUN = ["dflow_pyr_down"] + FRONT + BACK + ["dflow_flow_upsample"] + FRONT + ["dflow_prior_proposals"] + BACK


def test_run_pair_without_a_gate_is_two_runs(torch_, synth, monkeypatch):
    P = pkg("pipeline")
    img1, img2, _ = synth.make_pair(H, W, seed=SEED, amp_x=8.0, amp_y=4.0)
    names = record_calls(monkeypatch)
    want_f = P.PyramidFlow(H, W, 2, CH, CW, seed=SEED).run(img1, img2, 2).cpu().numpy().copy()
    assert names == PYRAMID_RUN, "PyramidFlow.run launches what it launched before"
    want_b = P.PyramidFlow(H, W, 2, CH, CW, seed=SEED).run(img2, img1, 2).cpu().numpy().copy()
    del names[:]
    pf = P.PyramidFlow(H, W, 2, CH, CW, seed=SEED)
    fwd, bwd = pf.run_pair(img1, img2, 2)
    assert names == (["dflow_pyr_down"] + 2 * (FRONT + BACK) + 2 * ["dflow_flow_upsample"] + 2 * (FRONT + ["dflow_prior_proposals"] + BACK))
    assert fwd.data_ptr() != bwd.data_ptr() and pf.levels[0].flow.data_ptr() not in (fwd.data_ptr(), bwd.data_ptr())
    assert np.array_equal(fwd.cpu().numpy(), want_f) and np.array_equal(bwd.cpu().numpy(), want_b)
    assert not np.array_equal(want_f, -want_b)
    # one level: the two plain passes
    del names[:]
    f1, b1 = P.PyramidFlow(H, W, 1, CH, CW, seed=SEED).run_pair(img1, img2, 2, gate=None)
    assert names == 2 * (FRONT + BACK)
    df = P.DiscreteFlow(H, W, CH, CW, seed=SEED)
    assert np.array_equal(f1.cpu().numpy(), df.run(img1, img2, 2).cpu().numpy()) and np.array_equal(b1.cpu().numpy(), df.run(img2, img1, 2).cpu().numpy())


def test_run_pair_on_three_levels_is_two_runs(torch_, synth, monkeypatch):
    """The pair of priors carried across two coarse levels: flows and, per level and direction, the counts of the single runs."""
    P = pkg("pipeline")
    img1, img2, _ = synth.make_pair(H, W, seed=SEED, amp_x=8.0, amp_y=4.0)
    singles = []
    for a, b in ((img1, img2), (img2, img1)):
        one = P.PyramidFlow(H, W, 3, CH, CW, seed=SEED)
        flow = one.run(a, b, 2, counts=True).cpu().numpy().copy()
        singles.append((flow, [(lv, ups.cpu().tolist(), prior.cpu().tolist()) for lv, ups, prior in one.counts]))
    names = record_calls(monkeypatch)
    pf = P.PyramidFlow(H, W, 3, CH, CW, seed=SEED)
    flows = pf.run_pair(img1, img2, 2, counts=True)
    with_prior = 2 * ["dflow_flow_upsample"] + 2 * (FRONT + ["dflow_prior_proposals"] + BACK)
    assert names == 2 * ["dflow_pyr_down"] + 2 * (FRONT + BACK) + 2 * with_prior
    assert [entry[0] for entry in pf.counts] == [1, 0] and pf.gate_counts == []
    for d, (flow, counts) in enumerate(singles):
        assert np.array_equal(flows[d].cpu().numpy(), flow), "flow of direction %d" % d
        assert [(lv, ups[d].cpu().tolist(), prior[d].cpu().tolist()) for lv, ups, prior in pf.counts] == counts, "counts of direction %d" % d
        assert all(prior[0] > 0 for _, _, prior in counts), "every prior appended labels"
        print("direction %d: %d of %d vectors are not zero" % (d, int(np.any(flow != 0, axis=-1).sum()), H * W))


@pytest.fixture(scope="module")
def gated_pair(oracle, synth):
    """The pair of the gate test and its run composed on the CPU, once.  Amplitude 8 x 4: at (4, 2), the other pyramid tests'
    pair, the coarse level of this geometry has nothing to gate.  The coarse flows are integer fields, on which bilinear equals
    nearest bit for bit, so the one composition is the reference of both lookups."""
    img1, img2, _ = synth.make_pair(H, W, seed=SEED, amp_x=8.0, amp_y=4.0)
    levels = pkg("pipeline").pyramid_levels(H, W, 2, CH, CW)
    want = R.compose_pair(oracle, levels, img1, img2, 2, seed=SEED, gate=2)
    n = (H // 2) * (W // 2)
    for d in (0, 1):
        gated = n - want[1][d]["gate_counts"][0]
        assert 0.01 * n < gated < 0.99 * n, "the gate removes some of the coarse vectors and not all"
    return img1, img2, want


@pytest.mark.parametrize("bilinear", [False, True])
def test_run_pair_with_a_gate_equals_the_cpu_composition(torch_, gated_pair, monkeypatch, bilinear):
    P = pkg("pipeline")
    img1, img2, want = gated_pair
    pf = P.PyramidFlow(H, W, 2, CH, CW, seed=SEED)
    labels = {}
    real = pf.run_level

    def run_level(level, *args, **kw):
        r = real(level, *args, **kw)
        labels.setdefault(level, []).append((pf.levels[level].bestlabels.cpu().numpy().copy(), r[0].cpu().numpy().copy()))
        return r
    monkeypatch.setattr(pf, "run_level", run_level)
    names = record_calls(monkeypatch)
    fwd, bwd = pf.run_pair(img1, img2, 2, gate=2, gate_bilinear=bilinear, counts=True)
    assert names == (["dflow_pyr_down"] + 2 * (FRONT + BACK) + ["dflow_flow_consistency"] + 2 * ["dflow_flow_upsample"]
                     + 2 * (FRONT + ["dflow_prior_proposals"] + BACK))
    for level in (1, 0):                                               # the coarsest first: the first difference is the cause
        for d in (0, 1):
            assert np.array_equal(labels[level][d][0], want[level][d]["bestlabels"]), "labels of level %d, direction %d" % (level, d)
            assert np.array_equal(labels[level][d][1].astype(np.float64), want[level][d]["flow"]), "flow of level %d, direction %d" % (level, d)
    assert np.array_equal(fwd.cpu().numpy().astype(np.float64), want[0][0]["flow"]) and np.array_equal(bwd.cpu().numpy().astype(np.float64), want[0][1]["flow"])
    (lv, cnt), = pf.gate_counts
    assert lv == 1 and cnt.cpu().tolist() == [want[1][0]["gate_counts"], want[1][1]["gate_counts"]]
    (lv0, ups, prior_cnt), = pf.counts
    assert lv0 == 0 and [c.cpu().tolist() for c in prior_cnt] == [want[0][d]["prior_counts"] for d in (0, 1)]
    assert all(c.cpu().tolist()[2] > 0 for c in ups), "gated-out vectors leave fine pixels without a prior"
    # coarse_prior's two-direction variant is what run_pair used
    pf2 = P.PyramidFlow(H, W, 2, CH, CW, seed=SEED)
    pr = pf2.coarse_prior(pf2.image_pyramid(img1, img2), 2, gate=2, gate_bilinear=bilinear, pair=True)
    assert len(pr) == 2 and all(tuple(p.shape) == (H, W, 3) for p in pr)
    with pytest.raises(ValueError, match="gate needs pair=True"):
        pf2.coarse_prior(pf2.image_pyramid(img1, img2), 2, gate=2)


# ---- the command lines
def test_spremi_za_epic_natural_check(torch_, synth, tmp_path, monkeypatch, capsys):
    P, spz = pkg("pipeline"), pkg("spremiZaEpic")
    h, w = 60, 90
    rng = np.random.default_rng(12)
    fwd = rng.integers(-4, 5, (h, w, 2)).astype(np.float64)
    bwd = np.where(rng.random((h, w, 1)) < 0.7, -fwd, rng.integers(-4, 5, (h, w, 2))).astype(np.float64)
    img1 = synth.make_pair(h, w, seed=13)[0]
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img1[..., ::-1].copy()).save("a.png")
    Image.fromarray(img1[..., ::-1].copy()).save("b.png")
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    six = ["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny"]
    names = record_calls(monkeypatch)
    assert spz.main(six) == 0
    assert names == ["dflow_fb_consistency", "dflow_canny_edges"], "without the token: the launches it always issued"
    reference = np.load("sparse_field.npy")
    del names[:]
    assert spz.main(six + ["--natural-check"]) == 0
    assert names == ["dflow_flow_consistency", "dflow_canny_edges"]
    want = P.flow_consistency(fwd.astype(np.float32), bwd.astype(np.float32), 3).cpu().numpy()
    got = np.load("sparse_field.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want) and 0 < want[..., 2].sum() < h * w
    assert not np.array_equal(got, reference)
    pkg("evaluate").parovi(want, "want.txt")
    assert open("parovi.txt").read() == open("want.txt").read()
    del names[:]
    assert spz.main(six + ["--natural-check", "--gpu-epic"]) == 0
    assert names[0] == "dflow_flow_consistency" and "dflow_epic_interpolate" in names and "dflow_fb_consistency" not in names
    epic = pkg("flowio").read_flo("epic.flo")
    ivice = pkg("edge").canny_ivice_tensor("a.png")
    assert np.array_equal(epic[..., ::-1], P.epic_interpolate(want, ivice).cpu().numpy())
    assert spz.main(six + ["--gpu-epic", "--natural-check"]) == 2
    capsys.readouterr()


def test_run_batch_check_natural(torch_, synth, tmp_path, monkeypatch, capsys):
    P, flowio, rb = pkg("pipeline"), pkg("flowio"), pkg("run_batch")
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a"), "--eval"])
    assert names[:len(BATCH_FLOWS) + 1] == BATCH_FLOWS + ["dflow_fb_consistency"] and "dflow_flow_consistency" not in names
    del names[:]
    rb.main(base + ["--out", str(tmp_path / "r"), "--check", "reference"])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency"], "without the option: the launches it always issued"
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--check", "natural", "--eval", "--epic"])
    assert names[:len(BATCH_FLOWS) + 1] == BATCH_FLOWS + ["dflow_flow_consistency"] and "dflow_fb_consistency" not in names
    flows = [np.load(tmp_path / "b" / flowio.flow_name(0, d, 2)).astype(np.float32) for d in (0, 1)]
    for d in (0, 1):
        assert np.array_equal(flows[d], np.load(tmp_path / "a" / flowio.flow_name(0, d, 2)))
    want = P.flow_consistency(flows[0], flows[1], 2)
    got = np.load(tmp_path / "b" / "sparse_field_00.npy")
    assert np.array_equal(got, want.cpu().numpy()) and 0 < got[..., 2].sum() < 40 * 48
    assert not np.array_equal(got, np.load(tmp_path / "a" / "sparse_field_00.npy"))
    pkg("evaluate").parovi(got, str(tmp_path / "want.txt"))
    assert open(tmp_path / "b" / "parovi_00.txt").read() == open(tmp_path / "want.txt").read()
    assert "pair 0: %.1f%% of the forward flow survives" % (100.0 * got[..., 2].mean()) in capsys.readouterr().out
    ea, eb = json.load(open(tmp_path / "a" / "eval.json")), json.load(open(tmp_path / "b" / "eval.json"))
    assert "check" not in ea and eb["check"] == "natural"
    assert eb["pairs"][0]["sparse"]["n_test_valid"] == int(got[..., 2].sum()) and eb["pairs"][0]["fwd"] == ea["pairs"][0]["fwd"]
    img1 = synth.make_pair(40, 48, seed=synth.pair_seed(0, 0))[0]
    epic = flowio.read_flo(str(tmp_path / "b" / "epic_00.flo"))
    assert np.array_equal(epic[..., ::-1], P.epic_interpolate(want, P.canny_edges(img1)[1]).cpu().numpy())


def test_the_first_cli_with_a_gate(torch_, synth, tmp_path, monkeypatch):
    """`daisy i flann.py --pyramid 2 --gate 2`: the files of --pyramid 2, from the gated prior of this direction."""
    P = pkg("pipeline")
    monkeypatch.chdir(tmp_path)
    cli = os.path.join(ROOT, PKG, "daisy i flann.py")
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "3", "1", "1", "--synthetic", "%dx%d" % (H, W), "--cell", "%dx%d" % (CH, CW),
                                      "--pyramid", "2", "--coarse-bcd-times", "2", "--gate", "0.5", "--no-packedksets"])
    names = record_calls(monkeypatch)
    runpy.run_path(cli, run_name="__main__")
    assert names.count("dflow_flow_consistency") == 1 and names.count("dflow_flow_upsample") == 2
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(3, 0))
    pf = P.PyramidFlow(H, W, 2, CH, CW)
    prior = pf.coarse_prior(pf.image_pyramid(img2, img1), 2, gate=0.5, pair=True)[0]      # backward=1: the images swapped
    plain = pf.coarse_prior(pf.image_pyramid(img2, img1), 2)
    assert not np.array_equal(prior.cpu().numpy(), plain.cpu().numpy())
    df = pf.levels[0]
    df.load_pair(img2, img1)
    df.generisi()
    df.nasumicni()
    df.prior_proposals(prior, stride=2)
    st = df.host_state()
    assert np.array_equal(np.load("Daisy output slike 103 backward=1 labels_prior.npy"), st["bestlabels"])
    assert np.array_equal(np.load("Daisy output slike 103 backward=1 proposals_nakon_gausa.npy"), st["proposals"])
