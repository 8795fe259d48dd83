"""dflow_flow_color and dflow_warp_eval (csrc/flow_picture.hip) against the numpy restatements of flowpic_ref.py, and what is
built on them: pipeline.flow_color / warp_eval / photo_stats, flowpicture.py and run_batch --pictures --photo.  Run with
`pytest -m gpu`.

Warp: float32 with one rounding per operation on both sides: counts, max_err, the error plane (on its bits), the warped image
and the error picture are asserted exactly; sum_err within 1e-9 relative of the reference's sequential double sum (any order
of n <= 1,052,675 non-negative doubles stays within n * 2^-53 = 1.2e-10) and bit-equal between two calls.
Colour: double with one rounding per operation; everything but atan2 is determined to the bit.  A byte v passes when
v == floor(c) for the reference's unrounded c = 255 * col; where 0 < |c - rint(c)| <= 1e-6 it also passes as rint(c) or
rint(c) - 1.  tests/test_flowpic_ref.py asserts that at most 1 % of the pixels of any field used here have a channel in that
band; the planted pixels must match exactly.
Shapes: a lane takes four pixels and a block 1024: 1x1, 1x7 and 5x1 are less than one group or end in a part of one, 33x65
(2145 px) and 37x61 (2257 px) are three blocks and no multiple of 4; 436x1024 is the many-block reduction; 1025x1027
(flowpic_ref.BIG_SHAPE) is more groups than the capped grid's 1024 blocks take in one step, and ends in three single pixels."""
import json
import os

import numpy as np
import pytest

import flowpic_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = ("n", "n_outside", "n_unknown", "n_above")


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def fields(flow):
    """The field in both layouts."""
    return (("UVV", flow), ("DYDX", R.dydx(flow)))


# ------------------------------------------------------------------------------------------------ the colour picture
def check_color(img, ref, planted, label):
    c, v = ref["c"], img.astype(np.float64)
    r = np.rint(c)
    exact = v == np.floor(c)
    band = (np.abs(c - r) > 0) & (np.abs(c - r) <= 1e-6)
    ok = exact | (band & ((v == r) | (v == r - 1)))
    H, W = c.shape[:2]
    print("%s: %d bytes, %d not floor(c) (all inside the band: %s)" % (label, c.size, int((~exact).sum()), bool(ok.all())))
    for y, x in np.argwhere(~ok.all(axis=-1))[:8]:
        print("%s differs at (%d,%d): got %r, c = %r" % (label, y, x, img[y, x].tolist(), c[y, x].tolist()))
    assert ok.all()
    at = np.unravel_index(planted, (H, W))
    assert np.array_equal(img[at], ref["bgr"][at]), "the planted pixels match exactly"
    assert not img[~ref["known"]].any()


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_color_matches_the_reference(torch_, H, W):
    pipeline = pkg("pipeline")
    for scale in R.SCALES:
        flow, planted = R.color_case(H, W, scale)
        for name, field in fields(flow):
            for max_flow in (None, 10.0):
                ref = R.flow_color(field, max_flow or 0.0)
                img, radius = pipeline.flow_color(field, max_flow, return_radius=True)
                img, radius = img.cpu().numpy(), radius.cpu().numpy()
                assert img.dtype == np.uint8 and img.shape == (H, W, 3) and radius.dtype == np.float32 and radius.shape == (1,)
                assert radius.view(np.uint32)[0] == np.array([ref["maxrad"]], F).view(np.uint32)[0], (radius, ref["maxrad"])
                check_color(img, ref, planted, "%dx%d scale %g %s max_flow %s" % (H, W, scale, name, max_flow))
                # the radius output is optional and changes nothing
                assert np.array_equal(pipeline.flow_color(field, max_flow).cpu().numpy(), img)
    if H * W > 100:
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 100


def test_color_beyond_the_capped_grid(torch_):
    """color_max_kernel and color_kernel on their second grid-stride step: the automatic radius, both layouts."""
    pipeline = pkg("pipeline")
    (H, W), scale = R.BIG_SHAPE, R.BIG_SCALE
    flow, planted = R.color_case(H, W, scale)
    for name, field in fields(flow):
        ref = R.flow_color(field)
        img, radius = pipeline.flow_color(field, None, return_radius=True)
        img, radius = img.cpu().numpy(), radius.cpu().numpy()
        assert img.dtype == np.uint8 and img.shape == (H, W, 3) and radius.dtype == np.float32 and radius.shape == (1,)
        assert radius.view(np.uint32)[0] == np.array([ref["maxrad"]], F).view(np.uint32)[0], (radius, ref["maxrad"])
        check_color(img, ref, planted, "%dx%d scale %g %s automatic radius" % (H, W, scale, name))
        assert np.array_equal(pipeline.flow_color(field, None).cpu().numpy(), img)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 100


def test_color_automatic_radius_of_a_field_at_rest(torch_):
    pipeline = pkg("pipeline")
    flow = np.zeros((5, 7, 3), F)
    flow[..., 2] = 1
    flow[0, 0] = (np.nan, 0, 1)
    flow[1, 1] = (3, 4, 0)
    img, radius = pipeline.flow_color(flow, return_radius=True)
    img = img.cpu().numpy()
    assert radius.item() == 1.0 and (img[0, 0] == 0).all() and (img[1, 1] == 0).all() and (img.reshape(-1, 3)[2:8] == 255).all()
    none = flow.copy()
    none[..., 2] = 0
    img, radius = pipeline.flow_color(none, return_radius=True)
    assert radius.item() == 1.0 and not img.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ the warp
def same_plane(got, want, label):
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere((g != w).reshape(g.shape[0], g.shape[1], -1).any(axis=-1))
    for y, x in bad[:8]:
        print("%s differs at (%d,%d): got %r want %r" % (label, y, x, got[y, x], want[y, x]))
    return len(bad) == 0


def check_stats(st, ref, label):
    print("%s: n %d, outside %d, unknown %d, above %d, max %r, sum %r (reference %r)"
          % (label, st["n"], st["n_outside"], st["n_unknown"], st["n_above"], st["max_err"], st["sum_err"], ref["sum_err"]))
    for k in COUNTS:
        assert st[k] == ref[k], (label, k, st[k], ref[k])
    assert st["max_err"] == ref["max_err"]
    assert abs(st["sum_err"] - ref["sum_err"]) <= 1e-9 * ref["sum_err"]


def run_warp(img1, img2, field, **kw):
    stats, wp, err, pic = pkg("pipeline").warp_eval(img1, img2, field, warped=True, err=True, image=True, **kw)
    return stats, wp.cpu().numpy(), err.cpu().numpy(), pic.cpu().numpy()


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_warp_matches_the_reference(torch_, H, W):
    pipeline = pkg("pipeline")
    for scale in R.SCALES:
        img1, img2, flow, _ = R.warp_case(H, W, scale)
        for name, field in fields(flow):
            thresh, emax = (10.0, 30.0) if name == "UVV" else (60.0, 90.0)
            label = "%dx%d scale %g %s" % (H, W, scale, name)
            ref = R.warp(img1, img2, field, thresh, emax)
            stats, wp, err, pic = run_warp(img1, img2, field, err_thresh=thresh, err_max=emax)
            st = pipeline.photo_stats(stats)
            check_stats(st, ref, label)
            assert err.dtype == np.float32 and err.shape == (H, W) and wp.shape == pic.shape == (H, W, 3)
            assert same_plane(err, ref["err"], label + " err")
            assert same_plane(wp, ref["warped"], label + " warped")
            assert same_plane(pic, ref["bgr"], label + " error picture")
            # the statistics do not depend on the optional outputs, and two calls give the same bytes
            again = pipeline.warp_eval(img1, img2, field, thresh, emax)
            assert again.cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
            if st["n"]:
                assert st["mean_err"] == st["sum_err"] / st["n"] and st["above_pct"] == st["n_above"] * 100 / st["n"]
            else:
                assert np.isnan(st["mean_err"]) and np.isnan(st["above_pct"]) and st["max_err"] == 0.0 and st["sum_err"] == 0.0


def test_warp_beyond_the_capped_grid(torch_):
    """warp_main_kernel on its second grid-stride step: every optional output, both layouts."""
    pipeline = pkg("pipeline")
    (H, W), scale = R.BIG_SHAPE, R.BIG_SCALE
    img1, img2, flow, _ = R.warp_case(H, W, scale)
    for name, field in fields(flow):
        thresh, emax = (10.0, 30.0) if name == "UVV" else (60.0, 90.0)
        label = "%dx%d scale %g %s" % (H, W, scale, name)
        ref = R.warp(img1, img2, field, thresh, emax)
        stats, wp, err, pic = run_warp(img1, img2, field, err_thresh=thresh, err_max=emax)
        st = pipeline.photo_stats(stats)
        check_stats(st, ref, label)
        assert err.dtype == np.float32 and err.shape == (H, W) and wp.shape == pic.shape == (H, W, 3)
        assert same_plane(err, ref["err"], label + " err")
        assert same_plane(wp, ref["warped"], label + " warped")
        assert same_plane(pic, ref["bgr"], label + " error picture")
        again = pipeline.warp_eval(img1, img2, field, thresh, emax)
        assert again.cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
        assert st["n"] and st["mean_err"] == st["sum_err"] / st["n"] and st["above_pct"] == st["n_above"] * 100 / st["n"]


def test_warp_accumulates_over_two_pairs(torch_):
    torch = torch_
    pipeline = pkg("pipeline")
    a = R.warp_case(33, 65, 4.0)[:3]
    b = R.warp_case(37, 61, 20.0)[:3]
    ra, rb = R.warp(*a), R.warp(*b)
    total = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    assert pipeline.warp_eval(*a, stats=total) is total
    pipeline.warp_eval(*b, stats=total)
    st = pipeline.photo_stats(total)
    ref = {k: ra[k] + rb[k] for k in COUNTS + ("sum_err",)}
    ref["max_err"] = max(ra["max_err"], rb["max_err"])
    check_stats(st, ref, "33x65 + 37x61 accumulated")
    sa, sb = (pipeline.photo_stats(pipeline.warp_eval(*c)) for c in (a, b))
    assert st["sum_err"] == (0.0 + sa["sum_err"]) + sb["sum_err"]
    with pytest.raises(ValueError):
        pipeline.warp_eval(*a, stats=torch.zeros(8, dtype=torch.int64, device="cuda:0"))


# ------------------------------------------------------------------------------------------------ a frame-sized field
def test_two_calls_give_identical_bytes_at_436x1024(torch_, synth):
    torch = torch_
    pipeline = pkg("pipeline")
    H, W = 436, 1024
    img1, img2, gt = synth.make_pair(H, W, seed=1)
    flow = (np.asarray(gt, F) + np.random.default_rng(2).normal(0, 1.5, (H, W, 2))).astype(F)
    dev = torch.device("cuda", 0)
    t1, t2, tf = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (img1, img2, flow))
    runs = []
    for _ in range(2):
        out = pipeline.warp_eval(t1, t2, tf, warped=True, err=True, image=True) + pipeline.flow_color(tf, return_radius=True)
        runs.append([t.cpu().numpy().tobytes() for t in out])
    assert runs[0] == runs[1]
    st = pipeline.photo_stats(torch.frombuffer(bytearray(runs[0][0]), dtype=torch.int64))
    assert st["n"] + st["n_outside"] + st["n_unknown"] == H * W and st["n"] > 0.9 * H * W and st["n_unknown"] == 0
    # the warp by (nearly) the true flow explains the second image far better than no flow at all
    still = pipeline.photo_stats(pipeline.warp_eval(t1, t2, torch.zeros_like(tf)))
    print("436x1024: mean photometric error %.3f with the flow, %.3f with zero flow" % (st["mean_err"], still["mean_err"]))
    assert st["mean_err"] < 0.5 * still["mean_err"]


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L, pipeline = pkg("_lib"), pkg("pipeline")
    H, W = 37, 61
    img1, img2, flow, _ = R.warp_case(H, W, 4.0)
    dev = torch.device("cuda", 0)
    t1, t2, tf = (torch.from_numpy(a).to(dev) for a in (img1, img2, flow))
    want_stats = pipeline.warp_eval(t1, t2, tf).cpu().numpy().tobytes()
    want_img, want_rad = (t.cpu().numpy() for t in pipeline.flow_color(tf, return_radius=True))
    wsb_w, wsb_c = L.lib().dflow_warp_eval_workspace_bytes(H, W), L.lib().dflow_flow_color_workspace_bytes(H, W)
    ws_w, ws_c = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (wsb_w, wsb_c))
    stats = torch.full((6,), -7, dtype=torch.int64, device=dev)
    img = torch.full((H, W, 3), 7, dtype=torch.uint8, device=dev)
    rad = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_warp_eval", H, W, t1.data_ptr(), t2.data_ptr(), tf.data_ptr(), L.EVAL_UVV, 10.0, 30.0, 0, stats.data_ptr(),
               None, None, None, ws_w.data_ptr(), wsb_w, L.stream(dev))
        L.call("dflow_flow_color", H, W, tf.data_ptr(), L.EVAL_UVV, 0.0, img.data_ptr(), rad.data_ptr(), ws_c.data_ptr(), wsb_c,
               L.stream(dev))
    torch.cuda.synchronize()
    assert (stats == -7).all().item() and rad.item() == -7.0, "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert stats.cpu().numpy().tobytes() == want_stats
        assert np.array_equal(img.cpu().numpy(), want_img) and np.array_equal(rad.cpu().numpy(), want_rad)
        img.fill_(7)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ command lines
def test_flowpicture_command(torch_, tmp_path, monkeypatch, capsys):
    fp, flowio, pipeline = pkg("flowpicture"), pkg("flowio"), pkg("pipeline")
    H, W = 33, 65
    img1, img2, flow, _ = R.warp_case(H, W, 4.0)
    field = R.dydx(flow).astype(np.float64)
    field[~np.isfinite(field)] = 0.0
    monkeypatch.chdir(tmp_path)
    np.save("f.npy", field)                                   # [dy,dx], as the hot path saves it
    flowio.write_flo("f.flo", field)
    np.save("a.npy", img1)
    flowio.write_picture("b.ppm", img2)
    read = pkg("evaluate").ucitajFlow("f.npy")
    assert fp.main(["f.npy", "c.png"]) == 0 and fp.main(["f.flo", "c8.ppm", "--max-flow", "8"]) == 0
    assert capsys.readouterr().out == ""
    assert np.array_equal(flowio.read_png8("c.png"), pipeline.flow_color(read).cpu().numpy())
    assert np.array_equal(flowio.read_image("c8.ppm"), pipeline.flow_color(read, 8.0).cpu().numpy())
    assert fp.main(["f.npy", "--warp", "a.npy", "b.ppm", "--warped", "w.png", "--error-picture", "e.png"]) == 0
    stats, wp, pic = pipeline.warp_eval(img1, img2, read, warped=True, image=True)
    st = pipeline.photo_stats(stats)
    out = capsys.readouterr().out
    assert out == ("mean photometric error %.4f, %.2f%% above 10, over %d px; %d targets outside the frame, %d unknown\n"
                   % (st["mean_err"], st["above_pct"], st["n"], st["n_outside"], st["n_unknown"]))
    assert np.array_equal(flowio.read_png8("w.png"), wp.cpu().numpy()) and np.array_equal(flowio.read_png8("e.png"), pic.cpu().numpy())
    assert wp.any().item() and pic.any().item() and st["n"] > H * W // 2
    np.save("small.npy", img1[:-1])
    assert fp.main(["f.npy", "--warp", "small.npy", "b.ppm"]) == 2 and "the flow is 65x33" in capsys.readouterr().err


def test_run_batch_pictures_and_photo(torch_, synth, tmp_path):
    H, W = 45, 70
    rb, flowio, pipeline = pkg("run_batch"), pkg("flowio"), pkg("pipeline")
    plain, full = os.path.join(tmp_path, "plain"), os.path.join(tmp_path, "full")
    common = ["--pairs", "1", "--size", "%dx%d" % (H, W)]
    rb.main(common + ["--out", plain])
    rb.main(common + ["--out", full, "--pictures", "--photo"])
    # without the options: the files of today; with them: the same files with the same bytes, and two more
    assert sorted(os.listdir(plain)) == sorted([flowio.flow_name(0, 0, 4), flowio.flow_name(0, 1, 4), flowio.flow_name(0, 0, 4)[:-4] + ".flo",
                                                "sparse_field_00.npy", "parovi_00.txt"])
    assert sorted(os.listdir(full)) == sorted(os.listdir(plain) + ["flowcolor_00.png", "photo.json"])
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(full, name), "rb").read(), name
    fwd = np.load(os.path.join(full, flowio.flow_name(0, 0, 4))).astype(F)
    assert np.array_equal(flowio.read_png8(os.path.join(full, "flowcolor_00.png")), pipeline.flow_color(fwd).cpu().numpy())
    doc = json.load(open(os.path.join(full, "photo.json")))
    assert [r["pair"] for r in doc["pairs"]] == [0] and set(doc["totals"]) == {"fwd"} and doc["size"] == [H, W]
    row = doc["pairs"][0]["fwd"]
    assert doc["totals"]["fwd"] == row, "one pair: the device-accumulated total is the pair's row"
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
    ref = R.warp(img1, img2, fwd)
    assert all(row[k] == ref[k] for k in COUNTS) and row["max_err"] == ref["max_err"]
    assert abs(row["sum_err"] - ref["sum_err"]) <= 1e-9 * ref["sum_err"] and row["mean_err"] == row["sum_err"] / row["n"]
