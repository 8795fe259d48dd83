"""dflow_flow_eval (csrc/flow_eval.hip) against the numpy restatement eval_ref.py, and what is built on it:
pipeline.flow_eval / eval_stats, evaluate.error_metrics_gpu, visualization.py and run_batch --eval.  Run with `pytest -m gpu`.

Counts, max_err, the error plane and the picture are asserted exactly (the plane on its bits).  sum_err is a sum of n
non-negative doubles, each an exact float32: any order of additions stays within n * 2^-53 relative of the exact sum
(math.fsum), the bound asserted.
Shapes: a lane takes four pixels and a block 1024: 1x1, 1x7 and 3x5 are less than one group or end in a part of one, 37x53
(1961 px) is two blocks and no multiple of 4, 64x256 whole blocks, 131x257 several blocks and a one-pixel tail, 436x1024
the many-block reduction, 1025x1027 (1,052,675 px, a three-pixel tail) 1029 blocks' worth of groups: more than the 1024 blocks
of the capped grid, whose first blocks take a second grid-stride step."""
import json
import math
import os

import numpy as np
import pytest

import eval_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 1), (1, 7), (3, 5), (37, 53), (64, 256), (131, 257), (436, 1024), (1025, 1027)]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def planted(abs_thresh):
    """Rows (tU, tV, tvalid, gU, gV, gvalid) of the pixels every field carries, the most telling first."""
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    nan, inf = F(np.nan), F(np.inf)
    rows = [(106, 0, 1, 100, 0, 1),                                    # err 6 at gt (100,0): outlier by both rules
            (104, 0, 1, 100, 0, 1),                                    # err 4: by abs, not by KITTI (5 % of 100 is 5)
            (3, 0, 1, 0, 0, 1), (up(3), 0, 1, 0, 0, 1), (down(3), 0, 1, 0, 0, 1),      # err exactly 3 and its neighbours
            (7, 4 + abs_thresh, 1, 7, 4, 1), (0, up(abs_thresh), 1, 0, 0, 1), (0, down(abs_thresh), 1, 0, 0, 1),
            (9, 9, 0.5, 0, 0, 1), (9, 9, 1, 0, 0, 0.5), (9, 9, nan, 0, 0, 1), (9, 9, 1, 0, 0, nan),     # valid = 0.5, NaN
            (9, 9, up(0.5), 1, 2, 1),
            (nan, 0, 1, 0, 0, 1), (0, inf, 1, 0, 0, 1), (-inf, 1, 1, 0, 0, 1), (inf, 0, 1, inf, 0, 1), (1, 1, 1, nan, 0, 1),
            (1e30, 0, 1, -1e30, 0, 1),                                 # finite inputs, dfu * dfu overflows
            (1, 1, 1, 1, 1, 1)]                                        # err 0
    for i in range(257):                                               # every boundary of the picture's table
        e = F(3.0) * F(i) / F(256.0)
        rows += [(e, 0, 1, 0, 0, 1), (0, up(e), 1, 0, 0, 1), (down(e), 0, 1, 0, 0, 1)]
    return np.array(rows, F)


_cases = {}


def case(H, W, abs_thresh=3.0):
    """(test, gt, reference) of a shape, made once and shared read-only: random fields with about 30 % of each mask off, the
    planted pixels at random places (as many as fit into half the field) and one in the last pixel."""
    key = (H, W, abs_thresh)
    if key not in _cases:
        rng = np.random.default_rng(1000 * H + W)
        n = H * W
        gt = np.zeros((n, 3), F)
        gt[:, :2] = rng.normal(0, 30, (n, 2))
        gt[:, 2] = rng.random(n) > 0.3
        test = np.zeros((n, 3), F)
        test[:, :2] = gt[:, :2] + rng.normal(0, 2.0, (n, 2)).astype(F)
        test[:, 2] = rng.random(n) > 0.3
        rows = planted(abs_thresh)
        k = min(len(rows), max(1, n // 2))
        where = rng.permutation(n - 1)[:k - 1].tolist() + [n - 1]
        test[where], gt[where] = rows[:k, :3], rows[:k, 3:]
        test, gt = test.reshape(H, W, 3), gt.reshape(H, W, 3)
        ref = R.evaluate(test, gt, abs_thresh)
        for a in (ref["err"], ref["bgr"]):
            a.setflags(write=False)
        _cases[key] = (test, gt, ref)
    return _cases[key]


COUNTS = ("n", "n_out_abs", "n_out_kitti", "n_nonfinite", "n_gt_valid", "n_test_valid")


def check_stats(st, ref, label):
    print("%s: n %d, abs %d, kitti %d, nonfinite %d, max %r, sum %r (fsum %r, off by %.3g, bound %.3g)"
          % (label, st["n"], st["n_out_abs"], st["n_out_kitti"], st["n_nonfinite"], st["max_err"], st["sum_err"], ref["sum_err"],
             abs(st["sum_err"] - ref["sum_err"]), ref["n"] * 2.0 ** -53 * ref["sum_err"]))
    for k in COUNTS:
        assert st[k] == ref[k], (label, k, st[k], ref[k])
    assert st["max_err"] == ref["max_err"]
    assert abs(st["sum_err"] - ref["sum_err"]) <= ref["n"] * 2.0 ** -53 * ref["sum_err"]


def same_plane(got, want, test, gt, label):
    """got == want on the bytes; the first differing pixels are printed with their inputs."""
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere((g != w).reshape(g.shape[0], g.shape[1], -1).any(axis=-1))
    for y, x in bad[:8]:
        print("%s differs at (%d,%d): got %r want %r, test %r gt %r" % (label, y, x, g[y, x], w[y, x], test[y, x], gt[y, x]))
    return len(bad) == 0


def run(test, gt, abs_thresh=3.0, **kw):
    pipeline = pkg("pipeline")
    stats, err, img = pipeline.flow_eval(test, gt, abs_thresh, err=True, image=True, **kw)
    return stats, err.cpu().numpy(), img.cpu().numpy()


@pytest.mark.parametrize("H,W", SHAPES)
def test_matches_the_reference(torch_, H, W):
    pipeline = pkg("pipeline")
    abs_thresh = 1.5 if (H, W) in ((3, 5), (131, 257)) else 3.0
    test, gt, ref = case(H, W, abs_thresh)
    stats, err, img = run(test, gt, abs_thresh)
    st = pipeline.eval_stats(stats)
    check_stats(st, ref, "%dx%d UVV" % (H, W))
    assert err.dtype == np.float32 and err.shape == (H, W) and img.dtype == np.uint8 and img.shape == (H, W, 3)
    assert same_plane(err, ref["err"], test, gt, "err")
    assert same_plane(img, ref["bgr"], test, gt, "picture")
    if H * W >= 1600:
        assert ref["n_nonfinite"] >= 6 and ref["n_out_kitti"] >= 1 and len(np.unique(ref["bgr"].reshape(-1, 3), axis=0)) >= 250
    # the statistics do not depend on the optional outputs
    assert pipeline.flow_eval(test, gt, abs_thresh).cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
    # mean and percentages of the read-back
    if st["n"]:
        assert st["mean_epe"] == st["sum_err"] / st["n"] and st["outliers_pct"] == st["n_out_abs"] * 100 / st["n"]
        assert st["kitti_fl_pct"] == st["n_out_kitti"] * 100 / st["n"]
    else:
        assert all(np.isnan(st[k]) for k in ("mean_epe", "outliers_pct", "kitti_fl_pct"))


@pytest.mark.parametrize("H,W", SHAPES)
def test_dydx_layout_equals_uvv_with_every_pixel_valid(torch_, H, W):
    pipeline = pkg("pipeline")
    test, gt, _ = case(H, W)
    all_valid = test.copy()
    all_valid[..., 2] = 1.0
    dydx = np.ascontiguousarray(test[..., 1::-1])
    s1, e1, i1 = run(all_valid, gt)
    s2, e2, i2 = run(dydx, gt)
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    assert e1.tobytes() == e2.tobytes() and i1.tobytes() == i2.tobytes()
    ref = R.evaluate(dydx, gt)
    check_stats(pipeline.eval_stats(s2), ref, "%dx%d DYDX" % (H, W))
    assert same_plane(e2, ref["err"], dydx, gt, "err") and same_plane(i2, ref["bgr"], dydx, gt, "picture")


def test_nothing_compared(torch_):
    pipeline = pkg("pipeline")
    test, gt, _ = case(37, 53)
    none = gt.copy()
    none[..., 2] = 0.0
    stats, err, img = run(test, none)
    st = pipeline.eval_stats(stats)
    assert st["n"] == 0 and st["n_gt_valid"] == 0 and st["sum_err"] == 0.0 and st["max_err"] == 0.0 and np.isnan(st["mean_epe"])
    assert (err == -1).all() and not img.any()


def test_two_calls_give_identical_bytes(torch_):
    test, gt, _ = case(436, 1024)
    a, b = (pkg("pipeline").flow_eval(test, gt).cpu().numpy().tobytes() for _ in range(2))
    assert a == b and len(a) == 64


def test_accumulate_over_two_fields(torch_):
    torch = torch_
    pipeline = pkg("pipeline")
    t1, g1, r1 = case(131, 257, 1.5)
    t2, g2, r2 = case(37, 53)
    total = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    assert pipeline.flow_eval(t1, g1, 1.5, stats=total) is total
    pipeline.flow_eval(t2, g2, 3.0, stats=total)
    st = pipeline.eval_stats(total)
    ref = {k: r1[k] + r2[k] for k in COUNTS}
    ref["max_err"] = max(r1["max_err"], r2["max_err"])
    ref["sum_err"] = math.fsum([r1["sum_err"], r2["sum_err"]])
    check_stats(st, ref, "131x257 + 37x53 accumulated")
    # the same order of additions as the two separate sums added once
    s1, s2 = (pipeline.eval_stats(pipeline.flow_eval(t, g, th)) for t, g, th in ((t1, g1, 1.5), (t2, g2, 3.0)))
    assert st["sum_err"] == (0.0 + s1["sum_err"]) + s2["sum_err"]
    with pytest.raises(ValueError):
        pipeline.flow_eval(t1, g1, stats=torch.zeros(8, dtype=torch.float64, device="cuda:0"))


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L, pipeline = pkg("_lib"), pkg("pipeline")
    H, W = 131, 257
    test, gt, ref = case(H, W, 1.5)
    dev = torch.device("cuda", 0)
    t, g = torch.from_numpy(test).to(dev), torch.from_numpy(gt).to(dev)
    direct = pipeline.flow_eval(t, g, 1.5).cpu().numpy().tobytes()
    wsb = L.lib().dflow_eval_workspace_bytes(H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stats = torch.full((8,), -7, dtype=torch.int64, device=dev)
    err = torch.full((H, W), -7.0, dtype=torch.float32, device=dev)
    img = torch.full((H, W, 3), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert torch.cuda.current_stream(dev) == side
        L.call("dflow_flow_eval", H, W, t.data_ptr(), L.EVAL_UVV, g.data_ptr(), 1.5, 0, stats.data_ptr(), err.data_ptr(),
               img.data_ptr(), ws.data_ptr(), wsb, L.stream(dev))
    torch.cuda.synchronize()
    assert (stats == -7).all().item() and (err == -7.0).all().item(), "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert stats.cpu().numpy().tobytes() == direct
        assert np.array_equal(err.cpu().numpy().view(np.uint32), ref["err"].view(np.uint32))
        assert np.array_equal(img.cpu().numpy(), ref["bgr"])
        err.fill_(-7.0)
        torch.cuda.synchronize()


def test_error_metrics_gpu(torch_, golden):
    ev = pkg("evaluate")
    g = golden("a40x48_c5x6")
    gt = ev.to_uv_valid(g["gt"], g["gt_valid"])
    mean, outliers, n = ev.error_metrics(g["sparse_t3"], gt)
    gmean, goutliers, gn = ev.error_metrics_gpu(g["sparse_t3"], gt)
    assert (gn, goutliers) == (n, outliers) and isinstance(goutliers, float)
    assert abs(gmean - mean) <= (int(np.ceil(np.log2(n))) + 2) * 2.0 ** -24 * mean


def test_visualization_command(torch_, golden, tmp_path, monkeypatch, capsys):
    ev, flowio, vis = pkg("evaluate"), pkg("flowio"), pkg("visualization")
    from test_eval_ref import decode_png8
    g = golden("b36x40_c9x8")
    gt = ev.to_uv_valid(g["gt"], g["gt_valid"])
    monkeypatch.chdir(tmp_path)
    flowio.write_kitti_flow_png("gt.png", gt)
    flow = g["b0_flow00"].astype(np.float64)                 # [dy,dx], as the hot path saves it
    np.save("test.npy", flow)
    flowio.write_flo("test.flo", flow)
    gt_read, test_read = ev.ucitajFlow("gt.png"), ev.ucitajFlow("test.npy")
    mean, outliers, n = ev.error_metrics(test_read, gt_read)
    ref = R.evaluate(test_read, gt_read)
    assert vis.main(["gt.png", "test.npy"]) == 0
    assert sorted(os.listdir(".")) == ["gt.png", "procenat_outliera.txt", "srednja_greska.txt", "test.flo", "test.npy"]
    assert vis.main(["gt.png", "test.flo", "err.png"]) == 0 and vis.main(["gt.png", "test.npy", "err.ppm"]) == 0
    assert capsys.readouterr().err == ""
    assert open("procenat_outliera.txt").read().split("\n") == [str(outliers)] * 3 + [""]
    assert str(outliers) == str(ref["n_out_abs"] * 100 / ref["n"])
    lines = open("srednja_greska.txt").read().split("\n")
    assert lines[1:] == [lines[0]] * 2 + [""]
    assert abs(float(lines[0]) - mean) <= (int(np.ceil(np.log2(n))) + 3) * 2.0 ** -24 * mean      # + the rounding to float32
    assert lines[0] == str(np.float32(float(lines[0])))
    want = pkg("pipeline").flow_eval(test_read, gt_read, image=True)[1].cpu().numpy()
    assert np.array_equal(want, ref["bgr"]) and want.any()
    assert np.array_equal(decode_png8("err.png"), want[..., ::-1])
    ppm = open("err.ppm", "rb").read()
    head = b"P6\n40 36\n255\n"
    assert ppm[:len(head)] == head and ppm[len(head):] == want[..., ::-1].tobytes()
    # nothing valid in both: 'nan' in both files, status 0; a NaN in the test flow: a warning
    none = gt.copy()
    none[..., 2] = 0
    flowio.write_kitti_flow_png("none.png", none)
    assert vis.main(["none.png", "test.npy"]) == 0
    assert open("procenat_outliera.txt").read().split("\n")[3] == "nan" and open("srednja_greska.txt").read().split("\n")[3] == "nan"
    bad = flow.copy()
    bad[np.nonzero(g["gt_valid"])[0][0], np.nonzero(g["gt_valid"])[1][0]] = np.nan
    np.save("bad.npy", bad)
    capsys.readouterr()
    assert vis.main(["gt.png", "bad.npy"]) == 0
    assert "1 compared pixels" in capsys.readouterr().err


def test_run_batch_eval(torch_, synth, tmp_path):
    H, W = 48, 64
    rb, ev, pipeline = pkg("run_batch"), pkg("evaluate"), pkg("pipeline")
    plain, with_eval = os.path.join(tmp_path, "plain"), os.path.join(tmp_path, "eval")
    common = ["--pairs", "2", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--epic"]
    rb.main(common + ["--out", plain])
    rb.main(common + ["--out", with_eval, "--eval"])
    assert sorted(os.listdir(with_eval)) == sorted(os.listdir(plain) + ["eval.json"])
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(with_eval, name), "rb").read(), name
    doc = json.load(open(os.path.join(with_eval, "eval.json")))
    assert [r["pair"] for r in doc["pairs"]] == [0, 1] and set(doc["totals"]) == {"fwd", "sparse", "epic"}
    for kind, tot in doc["totals"].items():
        rows = [r[kind] for r in doc["pairs"]]
        for k in COUNTS:
            assert tot[k] == sum(r[k] for r in rows)
        assert tot["max_err"] == max(r["max_err"] for r in rows)
        assert tot["sum_err"] == (0.0 + rows[0]["sum_err"]) + rows[1]["sum_err"]
        assert tot["mean_epe"] == tot["sum_err"] / tot["n"]
    # pair 0's rows are the evaluation of the files the run wrote, against the pair's true flow
    gt = ev.to_uv_valid(synth.make_pair(H, W, seed=synth.pair_seed(0, 0))[2])
    sparse = np.load(os.path.join(with_eval, "sparse_field_00.npy"))
    epic = np.ascontiguousarray(pkg("flowio").read_flo(os.path.join(with_eval, "epic_00.flo"))[..., ::-1])
    for kind, field in (("sparse", sparse), ("epic", epic)):
        ref = R.evaluate(field, gt)
        row = doc["pairs"][0][kind]
        assert all(row[k] == ref[k] for k in COUNTS) and row["max_err"] == ref["max_err"]
        assert abs(row["sum_err"] - ref["sum_err"]) <= ref["n"] * 2.0 ** -53 * ref["sum_err"]
    assert doc["pairs"][0]["epic"]["n"] == H * W and doc["pairs"][0]["sparse"]["n"] == int(sparse[..., 2].sum())
