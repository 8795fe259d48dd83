"""dflow_epipolar_fit on the device against its restatement (tests/epipolar_ref.py), bit for bit: the slots of the last round,
their counts, the best key, the model, the counts, the classes and the residual; and the layers above it: pipeline.epipolar_fit,
epipolar.py, run_batch.py --epipolar and the calls they issue.  A lane owns a sample in the solve and a slot in the score, a
wave 64 and a block 256 of them, three slots per sample, and a block stages R.CHUNK scored pixels: 1x1, 1x9 and 2x3 cannot give
a sample, 2x4 is a sample's worth of pixels and one, BIG has more scored pixels than two chunks and a ragged last one.  Every
call is made twice, into outputs filled with different garbage, and gives the same bytes.  Everything here needs a real MI355X:
run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import epipolar_ref as R
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu
F = np.float32
BIG = (64, 3 * R.CHUNK // 64 + 2)
SMALL = ((1, 1), (1, 9), (2, 3), (2, 4), (3, 3), (17, 19), (33, 65))
HIGH_SEED = 0x9E3779B97F4A7C15                      # a non-zero high word: the second half of the Philox key
OUTPUTS = ("cls", "residual", "counts")


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def device(torch_, flow, exclude=None, thresh=1.0, n_hyp=64, lo_rounds=1, step=1, seed=0, outputs=OUTPUTS):
    """dflow_epipolar_fit through the C-ABI, twice, every output filled with garbage first -> the dict epipolar_ref.fit returns."""
    L = pkg("_lib")
    h, w = flow.shape[:2]
    up = lambda a: None if a is None else torch_.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    dflow, dex = up(flow), up(exclude)
    ptr = lambda x: None if x is None else x.data_ptr()
    runs = []
    for garbage in (0x5A, 0xC3):
        new = lambda shape, dtype, want=True: torch_.full(shape, garbage, dtype=torch_.uint8, device="cuda").view(dtype) if want else None
        t = dict(model=new((36,), torch_.float32), models=new((3 * n_hyp * 36,), torch_.float32), hyp_counts=new((3 * n_hyp * 4,), torch_.int32),
                 state=new((256,), torch_.int64), cls=new((h * w,), torch_.uint8, "cls" in outputs),
                 residual=new((h * w * 4,), torch_.float32, "residual" in outputs), counts=new((32,), torch_.int32, "counts" in outputs))
        L.call("dflow_epipolar_fit", h, w, dflow.data_ptr(), L.EVAL_UVV if flow.shape[2] == 3 else L.EVAL_DYDX, ptr(dex), float(thresh), n_hyp,
               lo_rounds, step, seed, 0, t["model"].data_ptr(), t["models"].data_ptr(), t["hyp_counts"].data_ptr(), t["state"].data_ptr(),
               ptr(t["cls"]), ptr(t["residual"]), ptr(t["counts"]), L.stream(dflow.device))
        torch_.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
        got["key"] = int(got.pop("state").view(np.uint64)[0])
        runs.append(got)
    for k, v in runs[0].items():
        assert (v == runs[1][k]) if k == "key" else (v.tobytes() == runs[1][k].tobytes()), "the second call's %s differs" % k
    return runs[0]


def same(got, want, what):
    assert got["key"] == want["key"], "%s: best key %#x, expected %#x" % (what, got["key"], want["key"])
    for k in ("models", "model", "residual"):
        if k in got:
            g, v = got[k].view(np.uint32).reshape(-1), np.ascontiguousarray(want[k]).view(np.uint32).reshape(-1)
            bad = np.flatnonzero(g != v)
            assert bad.size == 0, "%s: %s differs at %d words, the first at %s: %s / %s" % (
                what, k, bad.size, bad[:4], got[k].reshape(-1)[bad[:4]], np.asarray(want[k]).reshape(-1)[bad[:4]])
    assert got["hyp_counts"].tolist() == want["hyp_counts"].tolist(), what
    if "cls" in got:
        assert np.array_equal(got["cls"], want["cls"].reshape(-1)), "%s: classes differ at %d pixels" % (
            what, (got["cls"] != want["cls"].reshape(-1)).sum())
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"], what


def check(torch_, flow, exclude=None, what="", outputs=OUTPUTS, **kw):
    want = R.fit(flow, exclude=exclude, **kw)
    same(device(torch_, flow, exclude, outputs=outputs, **kw), want, "%s %s" % (what, kw))
    return want


@pytest.mark.parametrize("shape", SMALL + (BIG,), ids=lambda s: "%dx%d" % s)
def test_every_frame_both_layouts(torch_, shape):
    h, w = shape
    f, ex = R.field(h, w, h * 100 + w, dirt=h * w > 9)
    for layout in (R.UVV, R.DYDX):
        want = check(torch_, R.M.as_layout(f, layout), ex if layout == R.UVV else None, "layout %d" % layout, thresh=0.5, n_hyp=44,
                     lo_rounds=2, seed=h + w)
        if h * w < 7 or h == 1:
            assert want["key"] == 0 and want["counts"][2:6] == [3 * 3 * 44, -1, -1, 0] and not want["model"].any(), "no sample, no model"
        if shape in ((17, 19), (33, 65), BIG):
            assert want["key"] >> 32 > 0.4 * want["counts"][0], "the scene is found through the dirt"
    if shape == BIG:
        assert want["counts"][0] > 2 * R.CHUNK and (h * w) % R.CHUNK, "more scored pixels than two chunks, the last chunk ragged"


@pytest.mark.parametrize("n_hyp", (1, 21, 22, 85, 86, 1000))
def test_a_lane_a_wave_and_a_block_of_slots(torch_, n_hyp):
    """3 * 21 = 63 and 3 * 22 = 66 slots cross a wave, 255 and 258 a block."""
    f, ex = R.field(17, 19, n_hyp)
    want = check(torch_, f, ex, thresh=0.5, n_hyp=n_hyp, lo_rounds=0 if n_hyp == 1000 else 2, seed=n_hyp)
    assert want["hyp_counts"].size == 3 * n_hyp


@pytest.mark.parametrize("step", (1, 2, 3))
def test_steps_and_rounds(torch_, step):
    h, w = 33, 65
    f, ex = R.field(h, w, 40 + step)
    for lo_rounds in (0, 2):
        want = check(torch_, f, ex, thresh=0.5, n_hyp=60, lo_rounds=lo_rounds, step=step, seed=step)
        assert want["counts"][0] == int((R.Field(f, ex, step).part & R.Field(f, ex, step).on_grid).sum())
        assert 0 <= want["counts"][3] <= lo_rounds


def test_exclude_a_seed_with_a_high_word_and_every_output_left_out_in_turn(torch_):
    h, w = 33, 65
    f, ex = R.field(h, w, 60)
    for exclude in (None, ex):
        for seed in (7, HIGH_SEED):
            check(torch_, f, exclude, thresh=0.5, n_hyp=44, seed=seed)
    a = R.fit(f, n_hyp=20, seed=HIGH_SEED, lo_rounds=0)
    assert not np.array_equal(a["models"], R.fit(f, n_hyp=20, seed=HIGH_SEED & 0xFFFFFFFF, lo_rounds=0)["models"]), "the high word is part of the key"
    for left_out in OUTPUTS + (OUTPUTS,):
        outs = tuple(o for o in OUTPUTS if o != left_out and o not in left_out)
        check(torch_, f, ex, "without %s" % (left_out,), outputs=outs, thresh=0.5, n_hyp=44, seed=3)


def test_fields_without_a_model_bad_vectors_and_thresholds(torch_):
    still = np.zeros((17, 19, 3), F)
    still[..., 2] = 1
    want = check(torch_, still, None, "a still camera", n_hyp=44)
    assert want["key"] == 0 and (want["cls"] == 2).all() and np.isinf(want["residual"]).all()
    bad = np.random.RandomState(1).uniform(-3, 3, (17, 19, 3)).astype(F)
    bad[..., 2] = 0
    bad[::2, :, 2], bad[::2, :, 0] = 1, np.nan
    bad[1, :, 1] = np.inf
    want = check(torch_, bad, None, "no good vector", n_hyp=44)
    assert want["counts"][0] == 0 and (want["cls"] == 0).all() and (want["residual"] == -1).all()
    f, ex = R.field(33, 65, 70)
    six = f.copy()
    six[..., 2] = 0
    six.reshape(-1, 3)[[0, 50, 190, 700, 1200, 2000], 2] = 1
    six[..., :2] = np.nan_to_num(six[..., :2], nan=0.0, posinf=0.0, neginf=0.0)
    assert check(torch_, six, None, "six participants", n_hyp=44)["key"] == 0
    # huge vectors: across the epipolar lines they overflow the denominator and agree with nothing; along them (this scene's
    # lines are close to horizontal) a model whose first row is all float32 denormals takes them in, on the device as in the
    # restatement
    huge = R.field(17, 19, 71, dirt=False)[0]
    huge[::3, ::2, 0] = F(3e38)
    huge[1::3, ::2, 1] = F(-1e30)
    want = check(torch_, huge, None, "huge vectors", thresh=0.5, n_hyp=44)
    assert (want["cls"][1::3, ::2] == 2).all() and np.isinf(want["residual"][1::3, ::2]).all() and want["key"] >> 32 > 100
    assert (np.abs(want["model"][:3]) < 2.0 ** -126).all() and want["model"][:3].any(), "denormal coefficients take part"
    # a threshold that is no power of two, a large one, and one far below the rounding of the targets
    for thresh in (0.3, 3.0, 1e-6, 1e-30):
        check(torch_, f, ex, "thresh", thresh=thresh, n_hyp=44, seed=12)


def test_bench_size_counts_on_a_sample_of_slots(torch_):
    h, w, n_hyp = 436, 1024, 1024
    f, ex = R.field(h, w, 80)
    js = [int(j) for j in np.random.RandomState(81).choice(n_hyp, 12, replace=False)]
    got = device(torch_, f, ex, thresh=1.0, n_hyp=n_hyp, lo_rounds=0, seed=82, outputs=("counts",))
    slots = [3 * j + m for j in js for m in range(3)]
    assert got["hyp_counts"][slots].tolist() == R.slot_counts_of(f, js, thresh=1.0, seed=82, exclude=ex)
    assert got["key"] >> 32 == got["hyp_counts"].max() == got["counts"][5] and got["counts"][3] == 0
    assert got["counts"][4] == int(np.argmax(got["hyp_counts"])), "at equal counts the smaller slot"
    assert got["counts"][6] == (1000 * int((got["models"].reshape(-1, 9) != 0).any(axis=1).sum())) // n_hyp


# ---- the layers above the entry point
def test_the_wrapper_gives_what_the_call_gives(torch_):
    P = pkg("pipeline")
    h, w = 33, 65
    f, ex = R.field(h, w, 90)
    want = R.fit(f, thresh=0.75, n_hyp=50, lo_rounds=2, step=2, seed=HIGH_SEED, exclude=ex)
    m, cls, res, cnt = P.epipolar_fit(f, thresh=0.75, n_hyp=50, lo_rounds=2, step=2, seed=HIGH_SEED, exclude=ex, classes=True, residual=True,
                                      counts=True)
    assert tuple(m.shape) == (3, 3) and m.cpu().numpy().tobytes() == want["model"].tobytes() and cnt.cpu().tolist() == want["counts"]
    assert np.array_equal(cls.cpu().numpy(), want["cls"]) and res.cpu().numpy().tobytes() == want["residual"].tobytes()
    # device tensors in, a side stream, one output alone
    g = R.M.as_layout(R.field(h, w, 91, dirt=False)[0], R.DYDX)
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        m, res = P.epipolar_fit(torch_.from_numpy(g).cuda(), n_hyp=50, residual=True)
    st.synchronize()
    want = R.fit(g, n_hyp=50)
    assert m.cpu().numpy().tobytes() == want["model"].tobytes() and res.cpu().numpy().tobytes() == want["residual"].tobytes()
    # the planted focus of expansion, through the device
    fwd, _ = R.scene("forward", seed=0, noise=0.0, moving=False)
    foe = P.epipolar_geometry(P.epipolar_fit(fwd, thresh=0.5, n_hyp=200).cpu().numpy(), h, w)["foe"]
    assert np.hypot(foe[0] - 32.0, foe[1] - 16.0) <= 2.0


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    h, w, n_hyp = 33, 65, 44
    f, ex = R.field(h, w, 93)
    want = R.fit(f, thresh=0.5, n_hyp=n_hyp, seed=5, exclude=ex)
    dev = torch.device("cuda", 0)
    tf, te = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in (f, ex))
    model, models = torch.full((9,), 7.0, device=dev), torch.empty(3 * n_hyp * 9, device=dev)
    hc, state = torch.empty(3 * n_hyp, dtype=torch.int32, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    cls, cnt = torch.full((h * w,), 9, dtype=torch.uint8, device=dev), torch.full((8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_epipolar_fit", h, w, tf.data_ptr(), L.EVAL_UVV, te.data_ptr(), 0.5, n_hyp, 1, 1, 5, 0, model.data_ptr(), models.data_ptr(),
               hc.data_ptr(), state.data_ptr(), cls.data_ptr(), None, cnt.data_ptr(), L.stream(dev))
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (model == 7).all().item(), "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert model.cpu().numpy().tobytes() == want["model"].tobytes() and cnt.cpu().tolist() == want["counts"]
        assert np.array_equal(cls.cpu().numpy(), want["cls"].reshape(-1)) and hc.cpu().tolist() == want["hyp_counts"].tolist()


def test_the_cli_and_run_batch_and_the_calls_they_issue(torch_, tmp_path, monkeypatch, capsys):
    flowio, ep, rb, P = pkg("flowio"), pkg("epipolar"), pkg("run_batch"), pkg("pipeline")
    h, w = 33, 65
    f, _ = R.field(h, w, 94)
    dydx = R.M.as_layout(R.field(h, w, 95, dirt=False)[0], R.DYDX)
    monkeypatch.chdir(tmp_path)
    np.save("sparse.npy", f)
    flowio.write_flo("dense.flo", dydx)
    names = record_calls(monkeypatch)
    assert ep.main(["sparse.npy", "--hyp", "50", "--seed", "3", "--thresh", "0.5", "--classes", "c.png", "--residual", "r.npy",
                    "--gate", "g.npy"]) == 0
    assert names == ["dflow_epipolar_fit"]
    want = R.fit(f, thresh=0.5, n_hyp=50, seed=3)
    geo = P.epipolar_geometry(want["model"], h, w)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "F: " + " ".join("%.9g" % v for v in geo["F"].reshape(-1))
    assert out[2].startswith("inliers: %d of %d scored vectors" % (want["counts"][1], want["counts"][0]))
    assert np.array_equal(flowio.read_png8("c.png")[..., 0], want["cls"] * 85)
    assert np.load("r.npy").tobytes() == want["residual"].tobytes()
    # the gate: outliers become [0,0,0], every other vector keeps its bits (pixels without a vector were [.,.,0] and are [0,0,0])
    g = np.load("g.npy")
    keep = (want["cls"] == 1) | (want["cls"] == 3)
    assert g[keep].tobytes() == f[keep].tobytes() and not g[~keep].any() and (want["cls"] == 2).any() and keep.any()
    # a .flo in, a coarser grid, JSON out, a .flo gate
    del names[:]
    assert ep.main(["dense.flo", "--hyp", "50", "--step", "2", "--lo-rounds", "2", "--gate", "g.flo", "--json"]) == 0
    assert names == ["dflow_epipolar_fit"]
    want = R.fit(dydx, n_hyp=50, step=2, lo_rounds=2)
    got = json.loads(capsys.readouterr().out)
    assert np.array(got["model"], F).tobytes() == want["model"].tobytes()
    assert [got[k] for k in R.COUNTS[:7]] == want["counts"][:7] and got["inlier_fraction"] == want["counts"][1] / want["counts"][0]
    assert np.array_equal(np.array(got["F"]), P.epipolar_geometry(want["model"], h, w)["F"])
    gf = flowio.read_flo("g.flo")
    inl = want["cls"] == 1
    assert gf[inl].tobytes() == np.ascontiguousarray(dydx[..., ::-1])[inl].tobytes() and not gf[~inl].any()
    # run_batch: without the option nothing new is called; with it one call per pair, after the check
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2"]
    del names[:]
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency"], "without the option: the launches it always issued"
    assert not (tmp_path / "a" / "epipolar.json").exists()
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--epipolar", "2", "--epipolar-gate"])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency", "dflow_epipolar_fit"]
    sparse = np.load(tmp_path / "a" / "sparse_field_00.npy")
    want = R.fit(sparse, thresh=2.0, n_hyp=512, lo_rounds=1)
    ej = json.load(open(tmp_path / "b" / "epipolar.json"))
    assert ej["thresh"] == 2.0 and ej["gate"] is True and len(ej["pairs"]) == 1
    row = ej["pairs"][0]
    assert np.array(row["model"], F).tobytes() == want["model"].tobytes()
    assert (row["pair"], row["scored"], row["inliers"], row["best_slot"]) == (0, want["counts"][0], want["counts"][1], want["counts"][4])
    assert "pair 0: epipolar geometry: %d of %d checked vectors within 2 px" % (want["counts"][1], want["counts"][0]) in capsys.readouterr().out
    gated = np.load(tmp_path / "b" / "sparse_field_00.npy")
    keep = want["cls"] != 2
    assert gated[keep].tobytes() == sparse[keep].tobytes() and not gated[~keep].any()
    for name in (flowio.flow_name(0, 0, 2), flowio.flow_name(0, 1, 2)):
        assert np.load(tmp_path / "b" / name).tobytes() == np.load(tmp_path / "a" / name).tobytes()
