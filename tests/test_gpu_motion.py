"""dflow_motion_fit on the device against its restatement (tests/motion_ref.py), bit for bit: the hypotheses of the last round,
their counts, the best key, the model, the counts, the classes, the model's flow and the residual; and the layers above it:
pipeline.motion_fit, motion_layers, motionfit.py, run_batch.py --motion and the calls they issue.  A lane owns a hypothesis, a
wave 64 and a block 256 of them, and a block stages R.CHUNK scored pixels: 1x1, 1x7, 2x2 and 3x3 are smaller than a sample,
collinear or just enough, BIG has more scored pixels than two chunks and a ragged last one.  Every call is made twice, into
outputs filled with garbage, and gives the same bytes.  Everything here needs a real MI355X: run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import motion_ref as R
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu
F = np.float32
BIG = (64, 3 * R.CHUNK // 64 + 2)
SMALL = ((1, 1), (1, 7), (2, 2), (3, 3), (17, 19), (33, 65))
HIGH_SEED = 0x9E3779B97F4A7C15                      # a non-zero high word: the second half of the Philox key
OUTPUTS = ("cls", "model_flow", "residual", "counts")
KIND_OF = {R.AFFINE: "affine", R.HOMOGRAPHY: "homography"}


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def device(torch_, flow, exclude=None, model=R.AFFINE, thresh=1.0, n_hyp=64, lo_rounds=1, polish=2, step=1, seed=0, outputs=OUTPUTS):
    """dflow_motion_fit through the C-ABI, twice, every output filled with garbage first -> the dict motion_ref.fit returns."""
    L = pkg("_lib")
    h, w = flow.shape[:2]
    up = lambda a: None if a is None else torch_.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    dflow, dex = up(flow), up(exclude)
    ptr = lambda x: None if x is None else x.data_ptr()
    runs = []
    for garbage in (0x5A, 0xC3):
        new = lambda shape, dtype, want=True: torch_.full(shape, garbage, dtype=torch_.uint8, device="cuda").view(dtype) if want else None
        t = dict(model=new((36,), torch_.float32), models=new((n_hyp * 36,), torch_.float32), hyp_counts=new((n_hyp * 4,), torch_.int32),
                 state=new((256,), torch_.int64), cls=new((h * w,), torch_.uint8, "cls" in outputs),
                 model_flow=new((h * w * 12,), torch_.float32, "model_flow" in outputs),
                 residual=new((h * w * 12,), torch_.float32, "residual" in outputs), counts=new((32,), torch_.int32, "counts" in outputs))
        L.call("dflow_motion_fit", h, w, dflow.data_ptr(), L.EVAL_UVV if flow.shape[2] == 3 else L.EVAL_DYDX, ptr(dex), model, float(thresh),
               n_hyp, lo_rounds, polish, step, seed, 0, t["model"].data_ptr(), t["models"].data_ptr(), t["hyp_counts"].data_ptr(),
               t["state"].data_ptr(), ptr(t["cls"]), ptr(t["model_flow"]), ptr(t["residual"]), ptr(t["counts"]), L.stream(dflow.device))
        torch_.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
        got["key"] = int(got.pop("state").view(np.uint64)[0])
        runs.append(got)
    for k, v in runs[0].items():
        assert (v == runs[1][k]) if k == "key" else (v.tobytes() == runs[1][k].tobytes()), "the second call's %s differs" % k
    return runs[0]


def same(got, want, what):
    assert got["key"] == want["key"], "%s: best key %#x, expected %#x" % (what, got["key"], want["key"])
    assert got["hyp_counts"].tolist() == want["hyp_counts"].tolist(), what
    for k in ("models", "model", "model_flow", "residual"):
        if k in got:
            g, v = got[k].view(np.uint32).reshape(-1), np.ascontiguousarray(want[k]).view(np.uint32).reshape(-1)
            bad = np.flatnonzero(g != v)
            assert bad.size == 0, "%s: %s differs at %d words, the first at %s: %s / %s" % (
                what, k, bad.size, bad[:4], got[k].reshape(-1)[bad[:4]], np.asarray(want[k]).reshape(-1)[bad[:4]])
    if "cls" in got:
        assert np.array_equal(got["cls"], want["cls"].reshape(-1)), "%s: classes differ at %d pixels" % (
            what, (got["cls"] != want["cls"].reshape(-1)).sum())
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"], what


def check(torch_, flow, exclude=None, what="", outputs=OUTPUTS, **kw):
    want = R.fit(flow, exclude=exclude, **kw)
    same(device(torch_, flow, exclude, outputs=outputs, **kw), want, "%s %s" % (what, kw))
    return want


@pytest.mark.parametrize("model", (R.AFFINE, R.HOMOGRAPHY))
@pytest.mark.parametrize("shape", SMALL + (BIG,), ids=lambda s: "%dx%d" % s)
def test_every_frame_both_models_and_layouts(torch_, shape, model):
    h, w = shape
    f, planted, ex = R.field(h, w, h * 100 + w, KIND_OF[model], outliers=0.3 if h * w > 9 else 0.0, dirty=h * w > 9)
    for layout in (R.UVV, R.DYDX):
        want = check(torch_, R.as_layout(f, layout), ex if layout == R.UVV else None, "layout %d" % layout, model=model, n_hyp=65,
                     lo_rounds=2, polish=2, seed=h + w)
        if h == 1:
            assert want["key"] == 0 and want["counts"][3:6] == [-1, -1, 0] and want["counts"][2] == 3 * 65, "no model from a line"
            assert np.array_equal(want["model"], R.IDENTITY)
    if shape == BIG:
        assert want["counts"][0] > 2 * R.CHUNK and (h * w) % R.CHUNK, "more scored pixels than two chunks, the last chunk ragged"


@pytest.mark.parametrize("n_hyp", (1, 63, 64, 65, 257, 1000))
def test_a_lane_a_wave_and_a_block_of_hypotheses(torch_, n_hyp):
    f, planted, ex = R.field(17, 19, n_hyp, "affine")
    check(torch_, f, ex, model=R.AFFINE, n_hyp=n_hyp, lo_rounds=0 if n_hyp == 1000 else 2, polish=1, seed=n_hyp)
    g, _, _ = R.field(17, 19, n_hyp, "homography")
    check(torch_, g, None, model=R.HOMOGRAPHY, n_hyp=n_hyp, lo_rounds=0 if n_hyp == 1000 else 1, polish=0, seed=n_hyp + 1)


@pytest.mark.parametrize("step", (1, 2, 3))
def test_steps_rounds_and_polish(torch_, step):
    h, w = 33, 65
    f, planted, ex = R.field(h, w, 40 + step, "affine")
    g, _, gex = R.field(h, w, 50 + step, "homography")
    for lo_rounds in (0, 2):
        for polish in (0, 2):
            want = check(torch_, f, ex, model=R.AFFINE, n_hyp=96, lo_rounds=lo_rounds, polish=polish, step=step, seed=step)
            assert want["counts"][0] == int((R.Field(f, ex, step).part & R.Field(f, ex, step).on_grid).sum())
            assert want["counts"][6] <= polish
        check(torch_, g, gex, model=R.HOMOGRAPHY, n_hyp=96, lo_rounds=lo_rounds, polish=2, step=step, seed=step)


def test_exclude_a_seed_with_a_high_word_and_every_output_left_out_in_turn(torch_):
    h, w = 33, 65
    f, planted, ex = R.field(h, w, 60, "affine")
    for exclude in (None, ex):
        for seed in (7, HIGH_SEED):
            check(torch_, f, exclude, model=R.AFFINE, n_hyp=65, seed=seed)
    a = R.fit(f, n_hyp=65, seed=HIGH_SEED)
    assert not np.array_equal(a["models"], R.fit(f, n_hyp=65, seed=HIGH_SEED & 0xFFFFFFFF)["models"]), "the high word is part of the key"
    for left_out in OUTPUTS + (OUTPUTS,):
        outs = tuple(o for o in OUTPUTS if o != left_out and o not in left_out)
        check(torch_, f, ex, "without %s" % (left_out,), outputs=outs, model=R.AFFINE, n_hyp=64, seed=3)
        check(torch_, f, ex, "without %s" % (left_out,), outputs=outs, model=R.HOMOGRAPHY, n_hyp=64, seed=3)


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_kind_of_field(torch_, kind):
    for h, w in ((17, 19), (33, 65)):
        f, planted, ex = R.field(h, w, 70, kind)
        for model in (R.AFFINE, R.HOMOGRAPHY):
            want = check(torch_, f, ex, kind, model=model, n_hyp=64, lo_rounds=1, polish=2, seed=11)
            if kind in ("allbad", "collinear"):
                assert want["key"] == 0 and want["counts"][2] == 2 * 64 and (want["cls"] != 1).all()
            if kind == "allbad":
                assert (want["cls"] == 0).all() and want["counts"][0] == 0
    # a threshold that is no power of two, a large one, and thresholds far below the rounding of the targets
    f, planted, ex = R.field(33, 65, 71, "homography")
    for thresh in (0.3, 3.0, 1e-6):
        check(torch_, f, ex, "thresh", model=R.HOMOGRAPHY, thresh=thresh, n_hyp=64, seed=12)
        check(torch_, f, ex, "thresh", model=R.AFFINE, thresh=thresh, n_hyp=64, seed=12)


def test_bench_size_counts_on_a_sample_of_hypotheses(torch_):
    h, w, n_hyp = 436, 1024, 1024
    f, planted, ex = R.field(h, w, 80, "affine")
    js = [int(j) for j in np.random.RandomState(81).choice(n_hyp, 64, replace=False)]
    for model in (R.AFFINE, R.HOMOGRAPHY):
        got = device(torch_, f, ex, model=model, n_hyp=n_hyp, lo_rounds=0, polish=0, seed=82, outputs=("counts",))
        assert got["hyp_counts"][js].tolist() == R.hyp_counts_of(f, js, model=model, seed=82, exclude=ex)
        assert got["key"] >> 32 == got["hyp_counts"].max() == got["counts"][5] and got["counts"][3] == 0
        assert got["counts"][4] == int(np.argmax(got["hyp_counts"])), "at equal counts the smaller index"


# ---- the layers above the entry point
def test_the_wrapper_gives_what_the_call_gives(torch_):
    P = pkg("pipeline")
    h, w = 33, 65
    f, planted, ex = R.field(h, w, 90, "affine")
    want = R.fit(f, R.AFFINE, thresh=1.5, n_hyp=80, lo_rounds=2, polish=1, step=2, seed=HIGH_SEED, exclude=ex)
    m, cls, mf, res, cnt = P.motion_fit(f, thresh=1.5, n_hyp=80, lo_rounds=2, polish=1, step=2, seed=HIGH_SEED, exclude=ex, classes=True,
                                        model_flow=True, residual=True, counts=True)
    assert m.cpu().numpy().tobytes() == want["model"].tobytes() and cnt.cpu().tolist() == want["counts"]
    assert np.array_equal(cls.cpu().numpy(), want["cls"])
    assert mf.cpu().numpy().tobytes() == want["model_flow"].tobytes() and res.cpu().numpy().tobytes() == want["residual"].tobytes()
    # device tensors in, a side stream, the defaults but for n_hyp; a homography; one output alone
    g, _, _ = R.field(h, w, 91, "homography")
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        m, res = P.motion_fit(torch_.from_numpy(R.as_layout(g, R.DYDX)).cuda(), model="homography", n_hyp=64, residual=True)
    st.synchronize()
    want = R.fit(R.as_layout(g, R.DYDX), R.HOMOGRAPHY, n_hyp=64)
    assert tuple(m.shape) == (3, 3) and m.cpu().numpy().tobytes() == want["model"].tobytes()
    assert res.cpu().numpy().tobytes() == want["residual"].tobytes()
    planted_model = P.motion_fit(R.planted_flow(R.PLANTED["affine"], h, w), n_hyp=16)
    assert R.corner_shift(planted_model.cpu().numpy().reshape(-1), R.PLANTED["affine"], h, w) < 1e-3


def test_motion_layers_separate_two_motions_with_nothing_read_back(torch_, monkeypatch):
    P = pkg("pipeline")
    h, w = 33, 65
    f, which = R.two_motions(h, w)
    names = record_calls(monkeypatch)
    models, layers = P.motion_layers(f, 2, n_hyp=64, seed=1)
    assert names == ["dflow_motion_fit"] * 2
    want_models, want_layers = R.layers(f, 2, n_hyp=64, seed=1)
    assert np.array_equal(layers.cpu().numpy(), want_layers) and np.array_equal(want_layers, which)
    for got, want in zip(models, want_models):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    # an exclude mask of the caller's, and a field with holes
    g, _, ex = R.field(h, w, 92, "affine")
    models, layers = P.motion_layers(g, 2, exclude=ex, n_hyp=48, polish=1, seed=3)
    want_models, want_layers = R.layers(g, 2, exclude=ex, n_hyp=48, polish=1, seed=3)
    assert np.array_equal(layers.cpu().numpy(), want_layers) and (want_layers[ex != 0] == 0).all()
    assert [m.cpu().numpy().tobytes() for m in models] == [m.tobytes() for m in want_models]


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    h, w, n_hyp = 33, 65, 64
    f, _, ex = R.field(h, w, 93, "affine")
    want = R.fit(f, R.AFFINE, n_hyp=n_hyp, seed=5, exclude=ex)
    dev = torch.device("cuda", 0)
    tf, te = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in (f, ex))
    model, models = torch.full((9,), 7.0, device=dev), torch.empty(n_hyp * 9, device=dev)
    hc, state = torch.empty(n_hyp, dtype=torch.int32, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    cls, cnt = torch.full((h * w,), 9, dtype=torch.uint8, device=dev), torch.full((8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_motion_fit", h, w, tf.data_ptr(), L.EVAL_UVV, te.data_ptr(), L.MOTION_AFFINE, 1.0, n_hyp, 1, 2, 1, 5, 0, model.data_ptr(),
               models.data_ptr(), hc.data_ptr(), state.data_ptr(), cls.data_ptr(), None, None, cnt.data_ptr(), L.stream(dev))
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (model == 7).all().item(), "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert model.cpu().numpy().tobytes() == want["model"].tobytes() and cnt.cpu().tolist() == want["counts"]
        assert np.array_equal(cls.cpu().numpy(), want["cls"].reshape(-1)) and hc.cpu().tolist() == want["hyp_counts"].tolist()


def test_motionfit_cli(torch_, tmp_path, monkeypatch, capsys):
    flowio, mf = pkg("flowio"), pkg("motionfit")
    h, w = 33, 65
    f, _, _ = R.field(h, w, 94, "affine")
    dydx = R.as_layout(R.field(h, w, 95, "homography", dirty=False)[0], R.DYDX)
    monkeypatch.chdir(tmp_path)
    np.save("sparse.npy", f)
    flowio.write_flo("dense.flo", dydx)
    names = record_calls(monkeypatch)
    assert mf.main(["sparse.npy", "--hyp", "64", "--seed", "3", "--thresh", "1.5", "--model-flow", "m.flo", "--residual", "r.flo",
                    "--classes", "c.png"]) == 0
    assert names == ["dflow_motion_fit"]
    want = R.fit(f, R.AFFINE, thresh=1.5, n_hyp=64, seed=3)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "affine model: " + " ".join("%.9g" % v for v in want["model"])
    assert out[1].startswith("inliers: %d of %d scored vectors" % (want["counts"][1], want["counts"][0]))
    # the model's flow is a file --prior takes: [u,v] of every pixel
    assert flowio.read_flo("m.flo").tobytes() == np.ascontiguousarray(want["model_flow"][..., :2]).tobytes()
    assert flowio.read_flo("r.flo").tobytes() == np.ascontiguousarray(want["residual"][..., :2]).tobytes()
    assert np.array_equal(flowio.read_png8("c.png")[..., 0], want["cls"] * 85)
    # a .flo in, a homography, a coarser grid, JSON out
    del names[:]
    assert mf.main(["dense.flo", "--model", "homography", "--hyp", "64", "--step", "2", "--lo-rounds", "2", "--json"]) == 0
    assert names == ["dflow_motion_fit"]
    want = R.fit(dydx, R.HOMOGRAPHY, n_hyp=64, step=2, lo_rounds=2)
    got = json.loads(capsys.readouterr().out)
    assert np.array(got["matrix"], F).tobytes() == want["model"].tobytes() and got["model"] == "homography"
    assert [got[k] for k in R.COUNTS] == want["counts"] and got["inlier_fraction"] == want["counts"][1] / want["counts"][0]
    # layers
    del names[:]
    two, which = R.two_motions(h, w)
    np.save("two.npy", two)
    assert mf.main(["two.npy", "--layers", "2", "--hyp", "64", "--seed", "1", "--classes", "l.png", "--json"]) == 0
    assert names == ["dflow_motion_fit"] * 2
    got = json.loads(capsys.readouterr().out)
    want_models, want_layers = R.layers(two, 2, n_hyp=64, seed=1)
    assert [np.array(l["matrix"], F).tobytes() for l in got["layers"]] == [m.tobytes() for m in want_models]
    assert [l["share"] for l in got["layers"]] == [float((which == i).sum()) / (h * w) for i in (1, 2)]
    assert np.array_equal(flowio.read_png8("l.png")[..., 0], want_layers * 127)


def test_run_batch_motion(torch_, synth, tmp_path, monkeypatch, capsys):
    flowio, rb = pkg("flowio"), pkg("run_batch")
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency"], "without the option: the launches it always issued"
    assert not (tmp_path / "a" / "motion.json").exists() and not (tmp_path / "a" / "residual_00.flo").exists()
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--motion", "homography", "--motion-thresh", "2"])
    assert names == BATCH_FLOWS + ["dflow_motion_fit", "dflow_fb_consistency"]
    fwd = np.load(tmp_path / "b" / flowio.flow_name(0, 0, 2)).astype(F)
    assert np.array_equal(fwd, np.load(tmp_path / "a" / flowio.flow_name(0, 0, 2)).astype(F))
    want = R.fit(fwd, R.HOMOGRAPHY, thresh=2.0, n_hyp=1024, lo_rounds=1, polish=2)
    mj = json.load(open(tmp_path / "b" / "motion.json"))
    assert mj["model"] == "homography" and mj["thresh"] == 2.0 and len(mj["pairs"]) == 1
    row = mj["pairs"][0]
    assert np.array(row["matrix"], F).tobytes() == want["model"].tobytes()
    assert (row["pair"], row["scored"], row["inliers"]) == (0, want["counts"][0], want["counts"][1])
    assert flowio.read_flo(str(tmp_path / "b" / "residual_00.flo")).tobytes() == np.ascontiguousarray(want["residual"][..., :2]).tobytes()
    assert "pair 0: homography motion: %d of %d vectors within 2 px" % (want["counts"][1], want["counts"][0]) in capsys.readouterr().out
    assert np.load(tmp_path / "b" / "sparse_field_00.npy").tobytes() == np.load(tmp_path / "a" / "sparse_field_00.npy").tobytes()
