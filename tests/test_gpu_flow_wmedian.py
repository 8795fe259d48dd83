"""dflow_flow_wmedian on the device against its numpy definition (tests/flow_wmedian_ref.py), byte for byte: the output plane and
the counts; and the layers above it: pipeline.flow_wmedian, flowfilter.py, run_batch.py --wmedian / --wmedian-reject and the
calls they issue.  The kernel takes a 32x8 tile per block with a halo of the radius: 1x1, 1x7 and 5x1 are smaller than any
window, 17x19 is smaller than a tile in one direction and than the window at radius 8, 33x65 has more than one tile in both
directions, ragged in both.  Everything here needs a real MI355X: run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import flow_wmedian_ref as R
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu
F = np.float32
FLAG_SETS = ((R.KEEP_HOLES, 0.0),) + tuple((R.REJECT, t) for t in R.REJECTS) + ((R.REJECT | R.KEEP_HOLES, 1.5),)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def device(torch_, flow, bgr=None, radius=3, wspace=None, wcolor=None, reject_thresh=0.0, flags=0, counts=True):
    """One dflow_flow_wmedian through the C-ABI, the output planes filled with garbage first -> (out, counts or None)."""
    L = pkg("_lib")
    h, w = flow.shape[:2]
    up = lambda a: None if a is None else torch_.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    dflow, dbgr, dws, dwc = up(flow), up(bgr), up(wspace), up(wcolor)
    out = torch_.full((h, w, 3), float("nan"), dtype=torch_.float32, device="cuda")
    cnt = torch_.full((4,), 0x5A5A5A5A, dtype=torch_.int32, device="cuda") if counts else None
    ptr = lambda x: None if x is None else x.data_ptr()
    L.call("dflow_flow_wmedian", h, w, dflow.data_ptr(), L.EVAL_UVV if flow.shape[2] == 3 else L.EVAL_DYDX, ptr(dbgr), radius, ptr(dws),
           ptr(dwc), float(reject_thresh), flags, out.data_ptr(), ptr(cnt), L.stream(dflow.device))
    torch_.cuda.synchronize()
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().tolist()


def same(got, want, what):
    g, v = (np.ascontiguousarray(x[0]).view(np.uint32).reshape(-1, 3) for x in (got, want))
    bad = np.flatnonzero((g != v).any(axis=1))
    assert bad.size == 0, "%s: the output differs at %d pixels, the first at raster index %s" % (what, bad.size, bad[:5])
    if got[1] is not None:
        assert got[1] == want[1], what


def check(torch_, flow, bgr=None, what="", counts=True, **kw):
    want = R.flow_wmedian(flow, bgr, **kw)
    same(device(torch_, flow, bgr, counts=counts, **kw), want, "%s %s" % (what, {k: v for k, v in kw.items() if k[0] != "w"}))
    return want


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_size_radius_field_layout_table_and_flag(torch_, shape, radius):
    h, w = shape
    img = R.image(h, w, h * 100 + w)
    sets = R.table_sets(radius, h + w)
    fields = {kind: R.field(h, w, h * 1000 + w * 10 + radius, kind) for kind in R.KINDS}
    # every field in both layouts, unguided and without tables
    for kind, f in fields.items():
        for layout in (R.UVV, R.DYDX):
            want = check(torch_, R.as_layout(f, layout), None, "%s layout %d" % (kind, layout), radius=radius)
            if kind == "const" or (layout == R.DYDX and kind != "holes"):
                assert want[1][1] == h * w and want[1][2] == 0, "every pixel is good: every window has a sample"
            if kind == "none" and layout == R.UVV:
                assert want[1] == [0, 0, 0, 0]
    # every table set, with and without holes
    for kind in ("holes", "frac", "wide"):
        for name, (space, color) in sets.items():
            want = check(torch_, fields[kind], img if color is not None else None, "%s tables %s" % (kind, name), radius=radius,
                         wspace=space, wcolor=color)
            if name == "nothing":
                assert want[1][1] == 0 and want[1][3] == want[1][0], "W == 0 at every pixel, the good ones included"
            if name == "zero_space" and kind == "frac" and h <= radius:
                assert want[1][1] == 0, "only the rows `radius` away weigh, and they lie outside"
    # every flag and threshold
    space, color = sets["both"]
    for kind in ("holes", "int", "zeros"):
        for flags, thresh in FLAG_SETS:
            want = check(torch_, fields[kind], img, "%s flags %d" % (kind, flags), radius=radius, wspace=space, wcolor=color,
                         reject_thresh=thresh, flags=flags)
            if kind == "holes":
                assert want[1][2] == 0, "no flag fills"
            if flags & R.REJECT and thresh == 1e30:
                assert want[1][3] == 0 and want[1][0] == want[1][1]
    want = check(torch_, fields["holes"], img, "rejecting from a filled window", radius=radius, wspace=sets["zeros"][0],
                 wcolor=sets["zeros"][1], reject_thresh=0.0, flags=R.REJECT)
    check(torch_, fields["holes"], img, "no counts", counts=False, radius=radius, wspace=space, wcolor=color)


def test_the_largest_weights(torch_):
    # every weight 255 * 255 over the 289 samples of radius 8: W = 18 792 225, 2 W still fits 32 bits
    h, w = 33, 65
    f = R.field(h, w, 5, "frac")
    img = np.full((h, w, 3), 9, np.uint8)
    space, color = R.table_sets(8, 0)["full"]
    want = check(torch_, f, img, "all 255", radius=8, wspace=space, wcolor=color)
    assert want[1] == [h * w, h * w, 0, want[1][3]] and want[1][3] > h * w // 2


def test_two_calls_give_the_same_bytes_and_the_wrapper_the_same_as_the_call(torch_):
    P = pkg("pipeline")
    h, w = 33, 65
    f, img = R.field(h, w, 6, "holes"), R.image(h, w, 7)
    space, color = R.tables(3, 1.5, 10.0)
    a = device(torch_, f, img, radius=3, wspace=space, wcolor=color)
    b = device(torch_, f, img, radius=3, wspace=space, wcolor=color)
    same(a, b, "second call")
    out, cnt = P.flow_wmedian(f, img, radius=3, sigma_space=1.5, counts=True)
    same((out.cpu().numpy(), cnt.cpu().tolist()), a, "the wrapper")
    same(a, R.flow_wmedian(f, img, radius=3, wspace=space, wcolor=color), "the definition")
    # device tensors in, the current stream, and the defaults: radius 3, no space table, sigma_color 10
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        again = P.flow_wmedian(torch_.from_numpy(f).cuda(), torch_.from_numpy(img).cuda())
    st.synchronize()
    assert again.cpu().numpy().tobytes() == R.flow_wmedian(f, img, radius=3, wcolor=R.tables(3, None, 10.0)[1])[0].tobytes()
    # reject and keep_holes through the wrapper; tables= overrides the sigmas
    out, cnt = P.flow_wmedian(f, None, radius=1, reject=1.5, counts=True)
    same((out.cpu().numpy(), cnt.cpu().tolist()), R.flow_wmedian(f, radius=1, reject_thresh=1.5, flags=R.REJECT), "reject")
    zs, zc = R.table_sets(3, 1)["zeros"]
    out = P.flow_wmedian(f, img, radius=3, sigma_space=9.0, keep_holes=True, tables=(zs, zc))
    same((out.cpu().numpy(), None), R.flow_wmedian(f, img, radius=3, wspace=zs, wcolor=zc, flags=R.KEEP_HOLES), "tables=")


def test_three_iterations_are_three_passes(torch_):
    P = pkg("pipeline")
    h, w = 33, 65
    img = R.image(h, w, 8)
    color = R.tables(2, None, 10.0)[1]
    for f in (R.as_layout(R.field(h, w, 9, "frac"), R.DYDX), R.field(h, w, 10, "holes")):
        want = (f, None)
        for _ in range(3):
            want = R.flow_wmedian(want[0], img, radius=2, wcolor=color)
        out, cnt = P.flow_wmedian(f, img, radius=2, iterations=3, counts=True)
        same((out.cpu().numpy(), cnt.cpu().tolist()), want, "three passes")
        one = P.flow_wmedian(f, img, radius=2)
        assert one.cpu().numpy().tobytes() == R.flow_wmedian(f, img, radius=2, wcolor=color)[0].tobytes()


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    h, w = 33, 65
    f, img = R.field(h, w, 11, "holes"), R.image(h, w, 12)
    space, color = R.tables(3, 2.0, 10.0)
    want = R.flow_wmedian(f, img, radius=3, wspace=space, wcolor=color)
    dev = torch.device("cuda", 0)
    tf, ti, ts, tc = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in (f, img, space, color))
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((4,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_flow_wmedian", h, w, tf.data_ptr(), L.EVAL_UVV, ti.data_ptr(), 3, ts.data_ptr(), tc.data_ptr(), 0.0, 0, out.data_ptr(),
               cnt.data_ptr(), L.stream(dev))
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (out == 7).all().item(), "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        same((out.cpu().numpy(), cnt.cpu().tolist()), want, "graph replay")


# ---- the command lines
def test_flowfilter_cli_equals_the_definition(torch_, tmp_path, monkeypatch, capsys):
    flowio, ff = pkg("flowio"), pkg("flowfilter")
    h, w = 33, 65
    f, img = R.field(h, w, 13, "holes"), R.image(h, w, 14)
    dydx = R.as_layout(R.field(h, w, 15, "frac"), R.DYDX)
    monkeypatch.chdir(tmp_path)
    np.save("img.npy", img)
    np.save("sparse.npy", f)
    flowio.write_flo("dense.flo", dydx)
    names = record_calls(monkeypatch)
    assert ff.main(["sparse.npy", "out.npy", "--image", "img.npy", "--radius", "2", "--sigma-space", "1.5", "--sigma-color", "8",
                    "--counts"]) == 0
    assert names == ["dflow_flow_wmedian"]
    space, color = R.tables(2, 1.5, 8.0)
    want = R.flow_wmedian(f, img, radius=2, wspace=space, wcolor=color)
    assert np.load("out.npy").tobytes() == want[0].tobytes()
    assert capsys.readouterr().out.strip() == "good=%d valid=%d filled=%d altered=%d" % tuple(want[1])
    # a .flo in, a .flo out, unguided, two passes, no --counts: nothing printed
    del names[:]
    assert ff.main(["dense.flo", "out.flo", "--radius", "1", "--iterations", "2"]) == 0
    assert names == ["dflow_flow_wmedian"] * 2 and capsys.readouterr().out == ""
    two = R.flow_wmedian(R.flow_wmedian(dydx, radius=1)[0], radius=1)[0]
    assert flowio.read_flo("out.flo").tobytes() == np.ascontiguousarray(two[..., :2]).tobytes()
    # reject and keep-holes
    assert ff.main(["sparse.npy", "rej.npy", "--reject", "1.5", "--counts"]) == 0
    want = R.flow_wmedian(f, radius=3, reject_thresh=1.5, flags=R.REJECT)
    assert np.load("rej.npy").tobytes() == want[0].tobytes() and capsys.readouterr().out.split()[3] == "altered=%d" % want[1][3]
    assert ff.main(["sparse.npy", "keep.npy", "--keep-holes"]) == 0
    assert np.load("keep.npy").tobytes() == R.flow_wmedian(f, radius=3, flags=R.KEEP_HOLES)[0].tobytes()


def test_run_batch_wmedian(torch_, synth, tmp_path, monkeypatch, capsys):
    P, flowio, rb = pkg("pipeline"), pkg("flowio"), pkg("run_batch")
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2", "--eval"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a")])
    plain = BATCH_FLOWS + ["dflow_fb_consistency"] + 4 * ["dflow_flow_eval"]
    assert names == plain, "without the options: the launches it always issued"
    assert not (tmp_path / "a" / "wmedian_00.flo").exists()
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--wmedian", "3", "--wmedian-reject", "3", "2"])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency", "dflow_flow_wmedian", "dflow_flow_wmedian"] + 6 * ["dflow_flow_eval"]
    fwd = np.load(tmp_path / "b" / flowio.flow_name(0, 0, 2)).astype(F)
    assert np.array_equal(fwd, np.load(tmp_path / "a" / flowio.flow_name(0, 0, 2)).astype(F))
    img1 = synth.make_pair(40, 48, seed=synth.pair_seed(0, 0))[0]
    color = R.tables(3, None, 10.0)[1]
    # wmedian_00.flo: the forward flow filtered, guided by the first image
    want = R.flow_wmedian(fwd, img1, radius=3, wcolor=color)[0]
    assert flowio.read_flo(str(tmp_path / "b" / "wmedian_00.flo")).tobytes() == np.ascontiguousarray(want[..., :2]).tobytes()
    # the sparse field: the checked field of the plain run with the outliers of its windows removed, the rest bit for bit
    checked = np.load(tmp_path / "a" / "sparse_field_00.npy")
    want, counts = R.flow_wmedian(checked, img1, radius=3, wcolor=color, reject_thresh=2.0, flags=R.REJECT)
    assert np.load(tmp_path / "b" / "sparse_field_00.npy").tobytes() == want.tobytes()
    printed = capsys.readouterr().out
    assert "pair 0: weighted median rejection: good=%d valid=%d filled=%d altered=%d" % tuple(counts) in printed
    ej = json.load(open(tmp_path / "b" / "eval.json"))
    assert ej["wmedian"] == 3 and ej["wmedian_reject"] == [3, 2.0]
    assert list(ej["pairs"][0]) == ["pair", "fwd", "sparse", "filtered"] and set(ej["totals"]) == {"fwd", "sparse", "filtered"}
    assert ej["pairs"][0]["sparse"]["n_test_valid"] == counts[1] and "filtered EPE" in printed
    plain_eval = json.load(open(tmp_path / "a" / "eval.json"))
    assert "wmedian" not in plain_eval and plain_eval["pairs"][0]["fwd"] == ej["pairs"][0]["fwd"]
