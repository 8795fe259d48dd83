"""dflow_two_view on the device against its restatement (tests/two_view_ref.py), byte for byte: d_pose, the four votes, depth,
class, err and counts; and the layers above it: pipeline.two_view, twoview.py, run_batch.py --pose and the calls they issue.  A
lane owns T.PER_LANE grid pixels and a block T.THREADS * T.PER_LANE contiguous ones: 1x1, 1x9 and 9x1 are a lane and a line,
33x65 is a block and 97 pixels (a wave and a ragged one), BIG more than two blocks and a ragged last one.  Every call is made
twice, into outputs filled with different garbage, and gives the same bytes; every plane is exact-size between guards at its lowest alignment (ws_guard.GuardedWs).
Everything here needs a real MI355X: run with `pytest -m gpu`."""
import itertools
import json

import numpy as np
import pytest

import epipolar_ref as R
import two_view_ref as T
import ws_guard as G
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu
F = np.float32
BIG = (64, 71)
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 4), (17, 19), (33, 65), (48, 160), BIG)
OUTPUTS = ("depth", "cls", "err", "counts")
MIXED = R.SCENES["mixed"][2:]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


class Placed:
    """Device planes of one call, each exactly its bytes between guards, `align` bytes past a 256-byte boundary."""

    def __init__(self, torch, poison):
        self.torch, self.dev, self.planes, self.poison = torch, torch.device("cuda", 0), {}, poison

    def put(self, name, align, data=None, dtype=None, shape=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype, shape = data.dtype, data.shape
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        g = G.GuardedWs(self.torch, nbytes, self.poison, self.dev, offset=align)
        assert g.ptr % align == 0 and g.ptr % (2 * align) != 0
        if data is not None:
            g.region.copy_(self.torch.from_numpy(np.frombuffer(data.tobytes(), np.uint8).copy()).to(self.dev))
        self.planes[name] = (g, np.dtype(dtype), tuple(shape), data)
        return g.ptr

    def get(self, name):
        g, dtype, shape, _ = self.planes[name]
        return np.frombuffer(g.snapshot(), dtype).reshape(shape)

    def check(self, what):
        self.torch.cuda.synchronize()
        for name, (g, _, _, data) in self.planes.items():
            g.assert_guards("%s, plane %s" % (what, name))
            if data is not None:
                assert g.snapshot() == data.tobytes(), "%s: input %s was changed" % (what, name)


def intrinsics(h, w, K):
    return (float(max(h, w)),) * 2 + ((w - 1) * 0.5, (h - 1) * 0.5) if K is None else tuple(float(v) for v in K)


def device(torch, flow, model, K=None, part=None, step=1, outputs=OUTPUTS):
    """dflow_two_view through the C-ABI, twice, every output filled with garbage first -> the dict two_view_ref.two_view returns."""
    L = pkg("_lib")
    h, w = flow.shape[:2]
    runs = []
    for poison in (0x5A, 0xFF):
        P = Placed(torch, poison)
        opt = lambda name, align, dtype, shape: P.put(name, align, None, dtype, shape) if name in outputs else None
        args = [P.put("flow", 4, flow), L.EVAL_UVV if flow.shape[2] == 3 else L.EVAL_DYDX, P.put("model", 4, np.asarray(model, F).reshape(9)),
                None if part is None else P.put("part", 1, np.asarray(part, np.uint8)), *intrinsics(h, w, K), step, 0,
                P.put("pose", 8, None, np.float64, (16,)), P.put("state", 8, None, np.int64, (32,)), opt("depth", 4, F, (h, w)),
                opt("cls", 1, np.uint8, (h, w)), opt("err", 4, F, (h, w)), opt("counts", 4, np.int32, (8,))]
        L.call("dflow_two_view", h, w, *args, L.stream(P.dev))
        P.check("dflow_two_view %dx%d step %d" % (w, h, step))
        got = {k: P.get(k) for k in ("pose",) + tuple(outputs)}
        got["votes"] = P.get("state")[:4]
        runs.append(got)
    for k, v in runs[0].items():
        assert v.tobytes() == runs[1][k].tobytes(), "the second call's %s differs" % k
    return runs[0]


def same(got, want, what):
    assert got["votes"].tolist() == want["votes"], "%s: votes %s, expected %s" % (what, got["votes"].tolist(), want["votes"])
    assert got["pose"].tobytes() == np.asarray(want["pose"], np.float64).tobytes(), "%s: pose\n%s\nexpected\n%s" % (what, got["pose"], want["pose"])
    for k in ("depth", "err"):
        if k in got:
            g, v = got[k].view(np.uint32).reshape(-1), np.ascontiguousarray(want[k]).view(np.uint32).reshape(-1)
            bad = np.flatnonzero(g != v)
            assert bad.size == 0, "%s: %s differs at %d pixels, the first at %s: %s / %s" % (
                what, k, bad.size, bad[:4], got[k].reshape(-1)[bad[:4]], want[k].reshape(-1)[bad[:4]])
    if "cls" in got:
        assert np.array_equal(got["cls"], want["cls"]), "%s: classes differ at %d pixels" % (what, (got["cls"] != want["cls"]).sum())
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"], "%s: counts %s, expected %s" % (what, got["counts"].tolist(), want["counts"])


def check(torch, flow, model, K=None, part=None, step=1, outputs=OUTPUTS, what=""):
    fx, fy, cx, cy = intrinsics(*flow.shape[:2], K)
    want = T.two_view(flow, model, fx, fy, cx, cy, part=part, step=step)
    same(device(torch, flow, model, K, part, step, outputs), want, "%s step %d" % (what, step))
    return want


def parts_of(f, seed):
    """The voters' planes of a field: none, the fit's classes (or, where a frame is too small for a fit, bytes 0..3), all 1, all 0."""
    h, w = f.shape[:2]
    cls = R.fit(f, thresh=0.5, n_hyp=30, lo_rounds=0, seed=seed)["cls"] if (h, w) in ((17, 19), (33, 65)) else \
        np.random.RandomState(seed).randint(0, 4, (h, w)).astype(np.uint8)
    return [None, cls, np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_frame_layout_voters_plane_and_step(torch_, shape):
    h, w = shape
    f, _ = R.field(h, w, h * 100 + w, dirt=h * w > 9)
    model = T.exact_model(h, w, *MIXED)
    parts, steps = parts_of(f, h + w), (1, 3, 64)
    if shape == (33, 65):
        combos = list(itertools.product((R.UVV, R.DYDX), range(4), steps))
        bad = f[..., :2][f[..., 2] > 0.5]
        assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any() and (bad == F(1e30)).any() and \
            (bad == F(-3e38)).any() and (f[..., 2] == 0).any(), "holes, NaN, +-Inf, 1e30 and -3e38 px are in the field"
    else:
        combos = [(R.UVV, 0, 1), (R.DYDX, 1, 3), (R.UVV, 2, 64), (R.DYDX, 3, 1), (R.UVV, 1, 1)]
    for layout, pi, step in combos:
        want = check(torch_, R.M.as_layout(f, layout), model, None, parts[pi], step, what="%dx%d layout %d part %d" % (h, w, layout, pi))
        if pi == 3:
            assert want["counts"][:4] == [0, 0, 0, -1] and want["pose"][15] == -1 and not want["pose"][:15].any(), "nobody votes: no pose"
        if pi == 0 and step == 1 and layout == R.UVV and h * w > 9:
            assert want["counts"][3] >= 0 and want["counts"][1] > 0.6 * want["counts"][0], "the pose is found through the dirt"
    block = T.THREADS * T.PER_LANE
    if shape == BIG:
        assert h * w > 2 * block and (h * w) % block and (h * w) % T.THREADS, "more than two blocks of grid pixels and a ragged last one"
    if shape == (33, 65):
        assert block < h * w < 2 * block and (h * w - block) % 64


def test_every_optional_output_left_out_in_turn(torch_):
    h, w = 33, 65
    f, _ = R.field(h, w, 60)
    model = T.exact_model(h, w, *MIXED)
    for left_out in OUTPUTS + (OUTPUTS,):
        outs = tuple(o for o in OUTPUTS if o != left_out and o not in left_out)
        check(torch_, f, model, outputs=outs, what="without %s" % (left_out,))


def sign_cases():
    for name in ("sideways", "forward", "mixed"):
        h, w, t, rot = R.SCENES[name]
        for ts, fs in itertools.product((1.0, -1.0), (1.0, -1.0)):
            yield name, h, w, tuple(ts * v for v in t), rot, fs


def test_each_candidate_wins_on_the_device(torch_):
    won = {}
    for name, h, w, t, rot, fs in sign_cases():
        flow = T.camera_flow(h, w, 0, t, rot)[0].astype(F)
        want = check(torch_, flow, T.exact_model(h, w, t, rot, sign=fs), what="%s t %s F %+g" % (name, t, fs))
        cand = want["counts"][3]
        assert cand >= 0 and want["votes"][cand] == want["counts"][1] and sum(want["votes"]) == want["counts"][1], "every vote goes to the winner"
        won.setdefault(name, []).append(cand)
    assert all(sorted(v) == [0, 1, 2, 3] for v in won.values()), won


def test_inputs_without_a_pose(torch_):
    h, w = 33, 65
    scene = R.scene("mixed")[0][:h, :w].copy()
    still = np.zeros((h, w, 3), F)
    still[..., 2] = 1
    rank1 = np.outer([1, 0.5, -0.25], [0.5, 1, 0.125]).astype(F).reshape(-1)
    for what, flow, model in (("a zero F^", scene, np.zeros(9, F)), ("the identity as F^, a still camera", still, np.eye(3, dtype=F).reshape(-1)),
                              ("an F^ of rank 1", scene, rank1), ("a NaN in F^", scene, np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 0], F))):
        want = check(torch_, flow, model, what=what)
        assert want["counts"] == [h * w, 0, 0, -1, 0, 0, h * w, 0] and want["pose"][15] == -1 and not want["pose"][:15].any(), what
        assert (want["cls"] == 3).all() and not want["depth"].any() and np.isposinf(want["err"]).all(), what
    # a still camera's flow through the fit itself: no model, so no pose
    P = pkg("pipeline")
    m = P.epipolar_fit(still, n_hyp=44)
    pose, cls, cnt = P.two_view(still, m, classes=True, counts=True)
    assert not m.cpu().numpy().any() and pose.cpu().tolist() == [0.0] * 15 + [-1.0]
    assert (cls == 3).all().item() and cnt.cpu().tolist() == [h * w, 0, 0, -1, 0, 0, h * w, 0]


def test_other_intrinsics_and_focal_lengths_at_the_edge(torch_):
    h, w, (t, rot) = 33, 65, MIXED
    K = (70.0, 55.5, 40.25, 9.75)
    flow = T.camera_flow(h, w, 4, t, rot, *K)[0].astype(F)
    want = check(torch_, flow, T.exact_model(h, w, t, rot, *K), K, what="fx != fy, an off-centre principal point")
    assert want["counts"][3] >= 0 and want["counts"][4] == h * w and T.rotation_error_deg(want["pose"][:9], rot) < 1e-4
    # the same field under the default camera: another answer, the same on both sides
    f, _ = R.field(h, w, 61)
    check(torch_, f, T.exact_model(h, w, t, rot), (1e-300, 1e300, -1e9, 1e9), what="focal lengths at the ends of float64")
    check(torch_, f, T.exact_model(h, w, t, rot), (1e300, 1e300, 0.0, 0.0), what="an essential matrix that overflows")


def test_the_fit_and_the_reconstruction_in_one_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    h, w, n_hyp = 33, 65, 44
    f, ex = R.field(h, w, 93)
    fit = R.fit(f, thresh=0.5, n_hyp=n_hyp, seed=5, exclude=ex)
    want = T.two_view(f, fit["model"], part=fit["cls"], step=2)
    assert want["counts"][3] >= 0
    dev = torch.device("cuda", 0)
    tf, te = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in (f, ex))
    model, models = torch.full((9,), 7.0, device=dev), torch.empty(3 * n_hyp * 9, device=dev)
    hc, state = torch.empty(3 * n_hyp, dtype=torch.int32, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    cls = torch.full((h * w,), 9, dtype=torch.uint8, device=dev)
    pose, state2 = torch.full((16,), 7.0, dtype=torch.float64, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    depth, cls2 = torch.full((h * w,), 7.0, device=dev), torch.full((h * w,), 9, dtype=torch.uint8, device=dev)
    err, cnt = torch.full((h * w,), 7.0, device=dev), torch.full((8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                       # one linear stream: no parallel branches
        L.call("dflow_epipolar_fit", h, w, tf.data_ptr(), L.EVAL_UVV, te.data_ptr(), 0.5, n_hyp, 1, 1, 5, 0, model.data_ptr(), models.data_ptr(),
               hc.data_ptr(), state.data_ptr(), cls.data_ptr(), None, None, L.stream(dev))
        L.call("dflow_two_view", h, w, tf.data_ptr(), L.EVAL_UVV, model.data_ptr(), cls.data_ptr(), float(w), float(w), (w - 1) * 0.5,
               (h - 1) * 0.5, 2, 0, pose.data_ptr(), state2.data_ptr(), depth.data_ptr(), cls2.data_ptr(), err.data_ptr(), cnt.data_ptr(),
               L.stream(dev))
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (pose == 7).all().item(), "a captured call must not run before the graph is replayed"
    graph.replay()
    torch.cuda.synchronize()
    got = dict(pose=pose.cpu().numpy(), votes=state2.cpu().numpy()[:4], depth=depth.cpu().numpy().reshape(h, w),
               cls=cls2.cpu().numpy().reshape(h, w), err=err.cpu().numpy().reshape(h, w), counts=cnt.cpu().numpy())
    assert model.cpu().numpy().tobytes() == fit["model"].tobytes()
    same(got, want, "replayed")


def test_the_wrapper_gives_what_the_call_gives(torch_):
    P = pkg("pipeline")
    h, w, (t, rot) = 33, 65, MIXED
    f, _ = R.field(h, w, 90)
    model = T.exact_model(h, w, t, rot)
    part = parts_of(f, 9)[1]
    want = T.two_view(f, model, part=part, step=2)
    pose, depth, cls, err, cnt = P.two_view(f, model.reshape(3, 3), part=part, step=2, depth=True, classes=True, err=True, counts=True)
    got = dict(pose=pose.cpu().numpy(), depth=depth.cpu().numpy(), cls=cls.cpu().numpy(), err=err.cpu().numpy(), counts=cnt.cpu().numpy(),
               votes=np.array(want["votes"]))
    same(got, want, "the wrapper")
    info = P.two_view_pose(pose.cpu().numpy())
    assert info["candidate"] == want["counts"][3] and abs(info["angle_deg"] - np.degrees(np.linalg.norm(rot))) < 1e-4
    # device tensors in, a side stream, other intrinsics, one output alone
    K = (70.0, 55.5, 40.25, 9.75)
    g = R.M.as_layout(T.camera_flow(h, w, 4, t, rot, *K)[0].astype(F), R.DYDX)
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        pose, depth = P.two_view(torch_.from_numpy(g).cuda(), torch_.from_numpy(T.exact_model(h, w, t, rot, *K)).cuda(), focal=K[:2],
                                 center=K[2:], depth=True)
    st.synchronize()
    want = T.two_view(g, T.exact_model(h, w, t, rot, *K), *K)
    assert pose.cpu().numpy().tobytes() == want["pose"].tobytes() and depth.cpu().numpy().tobytes() == want["depth"].tobytes()


def test_the_cli_and_run_batch_and_the_calls_they_issue(torch_, tmp_path, monkeypatch, capsys):
    flowio, tv, rb, P = pkg("flowio"), pkg("twoview"), pkg("run_batch"), pkg("pipeline")
    h, w = 33, 65
    f, _ = R.field(h, w, 94)
    K = (70.0, 55.5, 40.25, 9.75)
    monkeypatch.chdir(tmp_path)
    np.save("sparse.npy", f)
    names = record_calls(monkeypatch)
    assert tv.main(["sparse.npy", "--hyp", "50", "--seed", "3", "--thresh", "0.5", "--step", "2", "--depth", "d.npy", "--classes", "c.png",
                    "--err", "e.npy"]) == 0
    assert names == ["dflow_epipolar_fit", "dflow_two_view"]
    fit = R.fit(f, thresh=0.5, n_hyp=50, seed=3, step=2)
    want = T.two_view(f, fit["model"], part=fit["cls"], step=2)
    info = P.two_view_pose(want["pose"])
    out = capsys.readouterr().out.splitlines()
    assert want["counts"][3] >= 0 and out[1] == "t: " + " ".join("%.9g" % v for v in info["t"])
    assert out[0].startswith("rotation: %.6f deg" % info["angle_deg"])
    assert out[2] == "votes: %d of %d voters for candidate %d, %d for the runner-up" % (want["counts"][1], want["counts"][0], want["counts"][3],
                                                                                   want["counts"][2])
    assert out[3] == "pixels: %d in front of both cameras, %d behind one, %d without parallax" % tuple(want["counts"][4:7])
    assert np.load("d.npy").tobytes() == want["depth"].tobytes() and np.load("e.npy").tobytes() == want["err"].tobytes()
    assert np.array_equal(flowio.read_png8("c.png")[..., 0], want["cls"] * 85)
    # a .flo in, other intrinsics, JSON out
    dydx = R.M.as_layout(T.camera_flow(h, w, 4, *MIXED, *K)[0].astype(F), R.DYDX)
    flowio.write_flo("dense.flo", dydx)
    del names[:]
    assert tv.main(["dense.flo", "--hyp", "50", "--intrinsics"] + [repr(v) for v in K] + ["--json"]) == 0
    assert names == ["dflow_epipolar_fit", "dflow_two_view"]
    fit = R.fit(dydx, n_hyp=50)
    want = T.two_view(dydx, fit["model"], *K, part=fit["cls"])
    got = json.loads(capsys.readouterr().out)
    assert np.array(got["model"], F).tobytes() == fit["model"].tobytes() and np.array(got["pose"]).tobytes() == want["pose"].tobytes()
    assert [got[k] for k in T.COUNTS[:7]] == want["counts"][:7] and (got["fit_scored"], got["fit_inliers"]) == tuple(fit["counts"][:2])
    # the planted rotation, through the fit: a model that every inlier obeys to within thresh = 1 px can be turned by 1 px at the
    # focal length, 1 / 55.5 rad, and no further
    assert got["candidate"] >= 0 and T.rotation_error_deg(got["R"], MIXED[1]) < np.degrees(1.0 / min(K[:2]))
    # run_batch: without the option nothing new is called; with it one more call per pair, after the fit
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2", "--epipolar", "2"]
    del names[:]
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency", "dflow_epipolar_fit"], "without the option: the launches it always issued"
    plain = json.load(open(tmp_path / "a" / "epipolar.json"))
    assert "pose" not in plain["pairs"][0] and not (tmp_path / "a" / "depth_00.npy").exists()
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--pose", "48"])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency", "dflow_epipolar_fit", "dflow_two_view"]
    sparse = np.load(tmp_path / "b" / "sparse_field_00.npy")
    fit = R.fit(sparse, thresh=2.0, n_hyp=512, lo_rounds=1)
    want = T.two_view(sparse, fit["model"], 48.0, 48.0, part=fit["cls"])
    row = json.load(open(tmp_path / "b" / "epipolar.json"))["pairs"][0]
    assert {k: v for k, v in row.items() if k != "pose"} == plain["pairs"][0], "the rest of the row is what it was"
    info = P.two_view_pose(want["pose"])
    assert row["pose"]["focal"] == 48.0 and [row["pose"][k] for k in T.COUNTS[:7]] == want["counts"][:7]
    assert np.array(row["pose"]["R"]).tobytes() == info["R"].tobytes() and np.array(row["pose"]["t"]).tobytes() == info["t"].tobytes()
    assert np.load(tmp_path / "b" / "depth_00.npy").tobytes() == want["depth"].tobytes()
    assert "pair 0: pose: " in capsys.readouterr().out
    assert np.load(tmp_path / "b" / "sparse_field_00.npy").tobytes() == np.load(tmp_path / "a" / "sparse_field_00.npy").tobytes()
