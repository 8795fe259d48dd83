"""dflow_epic_prefilter (csrc/epic_prefilter.hip) against the numpy restatement epic_prefilter_ref.py: the reason plane byte
for byte except at seeds within a margin of a threshold, the estimates within 1e-3 px, the saliency within TOL_S, the output
field exactly the input with the dropped seeds zeroed; and the drop-ins built on it.  Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import canny_ref as CR
import epic_prefilter_cases as PC
import epic_prefilter_ref as P
import epic_ref as ER
from conftest import GOLDEN_NAMES, pkg

pytestmark = pytest.mark.gpu

# The largest |float32 - float64| of the reference's saliency over epic_prefilter_cases.saliency_images(), measured on the
# CPU (test_epic_prefilter_ref.py recomputes it), times 4: the GPU's tile order of float32 sums need not be numpy's.
SAL_YARD, SAL_FACTOR = 1.0072e-05, 4
TOL_S = SAL_FACTOR * SAL_YARD
TOL_B = 1e-6          # px, on |estimate - flow| - pref_th: both sides sum at most 256 double terms in the same order
TOL_EST = 1e-3        # px, as for the interpolated flow
CAP = 1e-3            # at most this share of a case's seeds may be excluded


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def gpu(sparse, edges, img=None, **kw):
    out, reason, sal, est = pkg("pipeline").epic_prefilter(sparse, edges, img, aux=True, **kw)
    return out.cpu().numpy(), reason.cpu().numpy(), sal.cpu().numpy(), est.cpu().numpy()


def compare(sparse, edges, img, got, ref, saliency_th, pref_th):
    """got = (out, reason, saliency, estimate) of the GPU against ref = P.prefilter(...)."""
    out, reason, sal, est = got
    seeds = ER.seed_mask(sparse)
    excl = np.zeros(seeds.shape, bool)
    if ref["saliency"] is not None:
        err = np.abs(sal.astype(np.float64) - ref["saliency"]).max()
        print("saliency: max |gpu - ref| = %.3e (TOL_S %.3e)" % (err, TOL_S))
        assert err <= TOL_S
        excl |= seeds & (np.abs(ref["saliency"] - saliency_th) <= TOL_S)
        # a flip in stage A changes the neighbourhoods of stage B: the inputs are chosen so that none is possible
        assert not (excl.any() and ref["dist"]), "stage A has seeds within TOL_S of its threshold in a case that runs stage B"
    else:
        assert not sal.any()
    for sd, d in ref["dist"].items():
        if abs(d - pref_th) <= TOL_B:
            excl.ravel()[sd] = True
    print("seeds %d, excluded %d, reasons ref %s gpu %s" % (seeds.sum(), excl.sum(), np.bincount(ref["reason"].ravel(), minlength=4).tolist(),
                                                           np.bincount(reason.ravel(), minlength=4).tolist()))
    assert excl.sum() <= CAP * seeds.sum()
    bad = np.argwhere((reason != ref["reason"]) & ~excl)
    assert bad.size == 0, "reason differs at %s" % bad[:5].tolist()
    at = np.zeros(seeds.shape, bool)
    at.ravel()[list(ref["dist"])] = True
    fin = np.isfinite(ref["estimate"]).all(axis=-1)
    err = np.abs(est - ref["estimate"])[fin]
    print("estimate: max |gpu - ref| = %.3e" % (err.max() if err.size else 0.0))
    assert err.size == 0 or err.max() < TOL_EST
    assert not est[~at].any()
    want = np.asarray(sparse, np.float32).copy()
    want[reason >= P.SALIENCY] = 0
    assert out.tobytes() == want.tobytes()
    counts, ms = pkg("pipeline").epic_prefilter_last_stats()
    assert counts == dict(seeds=int(seeds.sum()), dropped_saliency=int((reason == P.SALIENCY).sum()),
                          dropped_consistency=int((reason == P.CONSISTENCY).sum()))
    assert set(ms) == {"saliency", "graph", "consistency", "compact"}


def check(sparse, edges, img=None, saliency_th=0.0, pref_nn=25, pref_th=5.0, k=0.8):
    kw = dict(saliency_th=saliency_th, pref_nn=pref_nn, pref_th=pref_th, k=k)
    ref = P.prefilter(sparse, edges, img, **kw)
    compare(sparse, edges, img, gpu(sparse, edges, img, **kw), ref, saliency_th, pref_th)
    return ref


def median_saliency(img):
    """A threshold that splits the pixels of a textured frame evenly (at EpicFlow's 0.045 these frames lose no seed): half
    way between the two middle values of the reference's saliency, so that no pixel sits on it."""
    s = np.sort(P.saliency(img).ravel())
    return float(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_stage_b(torch_, name):
    sp, e, _ = PC.golden_case(name)
    check(sp, e)
    check(sp, e, pref_nn=100, pref_th=1.0, k=2.5)          # two register slots' worth of list; a threshold that bites


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_stage_a(torch_, name):
    sp, e, img = PC.golden_case(name)
    check(sp, e, img, saliency_th=median_saliency(img), pref_nn=0)
    check(sp, e, img, saliency_th=0.045, pref_nn=0)


def test_golden_both_stages(torch_):
    sp, e, img = PC.golden_case("c45x35_c9x7")
    ref = check(sp, e, img, saliency_th=median_saliency(img), pref_nn=25, pref_th=1.5)
    assert (ref["reason"] == P.SALIENCY).any() and (ref["reason"] == P.CONSISTENCY).any() and (ref["reason"] == P.KEPT).any()


@pytest.mark.parametrize("frame", PC.SYNTH_FRAMES[:2])
def test_random_fields(torch_, frame):
    H, W, seed = frame
    img = PC.synth_image(H, W, seed)
    for frac, style in ((0.3, "random"), (0.94, "sparse")):
        sp, e = PC.random_field(H, W, frac, seed, style)
        ref = check(sp, e, pref_th=4.0)
        assert (ref["reason"] == P.CONSISTENCY).any() and (ref["reason"] == P.KEPT).any()
        check(sp, e, img, saliency_th=median_saliency(img), pref_nn=0)


@pytest.mark.parametrize("size", [(1, 1), (1, 70), (70, 1)])
def test_small_sizes(torch_, size):
    sp, e = PC.random_field(*size, 0.3, seed=size[0] * 100 + size[1])
    sp[0, 0] = (1.5, -0.5, 1.0)
    img = dict(PC.saliency_images())["noise%dx%d" % size]
    check(sp, e, pref_nn=8, pref_th=3.0)
    check(sp, e, img, saliency_th=0.045, pref_nn=0)       # a 1-px-wide frame has no second gradient direction: s = 0


@pytest.mark.parametrize("case", ["none", "one", "two", "all"])
def test_seed_sets(torch_, case):
    H, W = 40, 60
    sp, e = PC.random_field(H, W, 1.0 if case == "all" else 0.0, seed=3, edge_style="sparse")
    if case in ("one", "two"):
        sp[7, 11] = (2.0, -1.0, 1.0)
    if case == "two":
        sp[30, 50] = (-3.0, 0.5, 1.0)
    ref = check(sp, e, pref_th=3.0)
    if case == "one":
        assert ref["reason"][7, 11] == P.KEPT and ref["dist"] == {7 * W + 11: 0.0}      # no other seed: kept
    if case == "two":
        assert (ref["reason"] == P.CONSISTENCY).sum() == 2                              # each is the other's only witness


def test_pref_nn_beyond_the_seeds_and_zero(torch_):
    sp, e = PC.random_field(30, 40, 0.02, seed=9)
    n = int(ER.seed_mask(sp).sum())
    assert 2 < n < 60
    check(sp, e, pref_nn=255, pref_th=3.0)
    check(sp, e, pref_nn=64, pref_th=3.0)                  # 65 entries: the four-slot kernel
    check(sp, e, pref_nn=63, pref_th=3.0)                  # 64 entries: the one-slot kernel, full
    ref = check(sp, e, pref_nn=0)
    assert not ref["dist"] and (ref["reason"][ER.seed_mask(sp)] == P.KEPT).all()


def test_nan_flow_is_no_seed(torch_):
    sp, e = PC.random_field(20, 30, 0.5, seed=4)
    sp[5, 5] = (np.nan, 1.0, 1.0)
    sp[6, 6] = (1.0, np.inf, 1.0)
    ref = check(sp, e)
    assert ref["reason"][5, 5] == P.NONE and ref["reason"][6, 6] == P.NONE


def test_null_image_needs_zero_threshold(torch_):
    sp, e = PC.random_field(20, 30, 0.5, seed=4)
    with pytest.raises(ValueError, match="img1"):
        pkg("pipeline").epic_prefilter(sp, e, None, saliency_th=0.045)
    a = pkg("pipeline").epic_prefilter(sp, e).cpu().numpy()                   # no image: stage B alone
    assert a.tobytes() == P.prefilter(sp, e, saliency_th=0)["out"].tobytes()


def test_planted_outliers_and_end_to_end(torch_):
    """The reference drops exactly the planted seeds (test_epic_prefilter_ref.py), and so must the GPU.  Mean dense EPE of
    the reference's LA interpolation against the known field: 0.3785 px from the unfiltered seeds, 0.0000 px from the
    filtered ones (the inliers are exactly affine)."""
    sp, e, bad, field = PC.planted()
    ref = check(sp, e)
    out, reason, _, _ = gpu(sp, e)
    assert np.array_equal(reason == P.CONSISTENCY, bad)
    pipeline = pkg("pipeline")
    epe = lambda f: float(np.sqrt(((f.cpu().numpy() - field) ** 2).sum(-1)).mean())
    before, after = epe(pipeline.epic_interpolate(sp, e)), epe(pipeline.epic_interpolate(pipeline.epic_prefilter(sp, e), e))
    print("EPE %.4f -> %.4f" % (before, after))
    assert after < before


def test_two_motions_and_flat_image(torch_):
    sp, e, band = PC.two_motions()
    ref = check(sp, e)
    assert not (ref["reason"] == P.CONSISTENCY).any()
    img = PC.half_flat_image()
    H, W = img.shape[:2]
    sp, e = PC.random_field(H, W, 0.5, seed=6)
    ref = check(sp, e, img, saliency_th=0.045, pref_nn=0)
    seeds = ER.seed_mask(sp)
    assert (ref["reason"][:, :W // 2 - 8][seeds[:, :W // 2 - 8]] == P.SALIENCY).all()
    assert (ref["reason"][:, W // 2 + 8:][seeds[:, W // 2 + 8:]] == P.KEPT).all()


def test_in_place_gives_the_same_bytes(torch_):
    torch = torch_
    L, pipeline = pkg("_lib"), pkg("pipeline")
    sp, e, img = PC.golden_case("a40x48_c5x6")
    th = median_saliency(img)
    want = pipeline.epic_prefilter(sp, e, img, saliency_th=th, pref_th=1.5).cpu().numpy()
    assert (want != sp).any()
    H, W = sp.shape[:2]
    dev = torch.device("cuda", 0)
    buf, ed, im = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sp, e, img))
    ws, ws_bytes = L.workspace("dflow_epic_prefilter_workspace_bytes", H, W, dev)
    L.call("dflow_epic_prefilter", H, W, im.data_ptr(), buf.data_ptr(), ed.data_ptr(), th, 25, 1.5, 0.8, buf.data_ptr(),
           None, None, None, ws.data_ptr(), ws_bytes, L.stream(dev))
    assert buf.cpu().numpy().tobytes() == want.tobytes()


def test_sampled_seeds_at_bench_size(torch_):
    """436x1024: stage A over the whole frame; stage B on a sample of seeds, with the reference's lists walked over the seed
    graph of the GPU's own diagram once verify_fixed_point has proved that diagram exact."""
    H, W, seed = PC.SYNTH_FRAMES[2]
    img = PC.synth_image(H, W, seed)
    sp, _ = PC.random_field(H, W, 0.7, seed)
    e = CR.ivice(CR.canny(img))
    pipeline = pkg("pipeline")
    th = median_saliency(img)
    check(sp, e, img, saliency_th=th, pref_nn=0)
    out, reason, _, est = gpu(sp, e, pref_th=4.0)
    _, S, D, _, _ = pipeline.epic_interpolate(sp, e, aux=True, lists=False)
    S, D = S.cpu().numpy(), D.cpu().numpy().view(np.uint32)
    assert ER.verify_fixed_point(sp, e, S, D) is None
    graph = ER.seed_graph(S, D.astype(np.int64), e)
    seeds = np.flatnonzero(ER.seed_mask(sp).ravel())
    kinds = set()
    for s in np.random.default_rng(4).choice(seeds, 256, replace=False).tolist():
        eu, ev, d = P.judge(sp, graph, s, 25, 0.8)
        assert abs(est.reshape(-1, 2)[s, 0] - eu) < TOL_EST and abs(est.reshape(-1, 2)[s, 1] - ev) < TOL_EST
        assert abs(d - 4.0) > TOL_B
        assert reason.ravel()[s] == (P.CONSISTENCY if P.dropped(sp, s, eu, ev, 4.0) else P.KEPT)
        kinds.add(int(reason.ravel()[s]))
    assert kinds == {P.KEPT, P.CONSISTENCY}
    want = sp.copy()
    want[reason >= P.SALIENCY] = 0
    assert out.tobytes() == want.tobytes()


def _png(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)


def test_epicflow_cli_prefilter(torch_, golden, tmp_path):
    z = golden("c45x35_c9x7")
    H, W = z["img1"].shape[:2]
    _png(os.path.join(tmp_path, "a.png"), z["img1"])
    _png(os.path.join(tmp_path, "b.png"), z["img2"])
    with open(os.path.join(tmp_path, "m.txt"), "wb") as f:
        f.write(z["parovi_t3_txt"].tobytes())
    edges = CR.ivice(CR.canny(z["img1"]))
    edges.tofile(os.path.join(tmp_path, "e.bin"))
    ef, flowio, pipeline = pkg("epicflow"), pkg("flowio"), pkg("pipeline")
    sp = ef.read_matches(os.path.join(tmp_path, "m.txt"), H, W)
    img = flowio.read_bgr(os.path.join(tmp_path, "a.png"))
    th = median_saliency(img)
    pos = [os.path.join(tmp_path, n) for n in ("a.png", "b.png", "e.bin", "m.txt", "o.flo")]
    for extra, kw in ((["--prefilter"], {}), (["--pref-th", "1.5", "--saliency-th", repr(th), "--pref-nn", "12", "-k", "2.5"],
                                              dict(pref_th=1.5, saliency_th=th, pref_nn=12, k=2.5))):
        assert ef.main(pos + extra) == 0
        filtered = pipeline.epic_prefilter(sp, edges, img, **kw)
        want = pipeline.epic_interpolate(filtered, edges, k=kw.get("k", 0.8)).cpu().numpy()
        assert flowio.read_flo(pos[4]).tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    assert (filtered.cpu().numpy() != sp).any()            # the second run did remove matches
    assert ef.main(pos + ["-prefnn", "25"]) == 2


def _fwd_bwd(H, W, tmp_path, monkeypatch, synth):
    rng = np.random.default_rng(12)
    fwd = rng.integers(-4, 5, (H, W, 2)).astype(np.float64)
    bwd = np.where(rng.random((H, W, 1)) < 0.7, -fwd, rng.integers(-4, 5, (H, W, 2))).astype(np.float64)
    img1 = synth.make_pair(H, W, seed=13)[0]
    monkeypatch.chdir(tmp_path)
    _png("a.png", img1)
    _png("b.png", img1)
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    return img1


def test_spremi_za_epic_prefilter(torch_, synth, tmp_path, monkeypatch, capsys):
    H, W = 60, 90
    img1 = _fwd_bwd(H, W, tmp_path, monkeypatch, synth)
    spz, pipeline = pkg("spremiZaEpic"), pkg("pipeline")
    six = ["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny"]
    assert spz.main(six + ["--gpu-epic"]) == 0
    plain = (open("sparse_field.npy", "rb").read(), open("parovi.txt", "rb").read(), open("epic.flo", "rb").read())
    assert spz.main(six + ["--gpu-epic", "--prefilter"]) == 0
    assert "pre-filter" in capsys.readouterr().out
    assert (open("sparse_field.npy", "rb").read(), open("parovi.txt", "rb").read()) == plain[:2]       # written unfiltered
    sparse = np.load("sparse_field.npy")
    edges = np.fromfile("ivice.bin", np.float32).reshape(H, W)
    filtered = pipeline.epic_prefilter(sparse, edges, img1)
    assert (filtered.cpu().numpy() != sparse).any()
    want = pipeline.epic_interpolate(filtered, edges).cpu().numpy()
    assert pkg("flowio").read_flo("epic.flo").tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    assert open("epic.flo", "rb").read() != plain[2]
    assert spz.main(six + ["--gpu-epic", "--prefilter", "--refine"]) == 0
    want = pipeline.variational_refine(img1, img1, want).cpu().numpy()
    assert pkg("flowio").read_flo("epic.flo").tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    assert spz.main(six + ["--gpu-epic", "--refine", "--prefilter"]) == 2


def test_run_batch_prefilter(torch_, synth, tmp_path):
    H, W = 48, 64
    rb, pipeline = pkg("run_batch"), pkg("pipeline")
    rb.main(["--pairs", "1", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--out", str(tmp_path), "--epic", "--prefilter"])
    sparse = np.load(os.path.join(tmp_path, "sparse_field_00.npy"))
    img1 = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))[0]
    edges = CR.ivice(CR.canny(img1))
    want = pipeline.epic_interpolate(pipeline.epic_prefilter(sparse, edges, img1), edges).cpu().numpy()
    got = pkg("flowio").read_flo(os.path.join(tmp_path, "epic_00.flo"))
    assert got.tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
