"""dflow_frame_interp on the device against its numpy definition (tests/frame_interp_ref.py), byte for byte: the frame, the keys,
the motion field, the provenance plane and the counts; and the layers above it: pipeline.frame_interp and frame_sequence,
midframe.py, run_batch.py --midframe and the calls they issue.  The kernels take one pixel per lane in blocks of 256: 33x65 has
a ragged last block, a row of 64x257 spans blocks.  Everything here needs a real MI355X: run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import frame_interp_ref as R
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def device(torch_, img1, img2, fwd, bwd=None, t=0.5, fill_rounds=8, occl_thresh=30.0, optional=True):
    """One dflow_frame_interp through the C-ABI, every output plane filled with garbage first -> the dict frame_interp_ref makes."""
    L = pkg("_lib")
    h, w = img1.shape[:2]
    up = lambda a: None if a is None else torch_.from_numpy(np.ascontiguousarray(a)).cuda()
    d1, d2, dfwd, dbwd = up(img1), up(img2), up(fwd), up(bwd)
    poison = {torch_.uint8: 0x5A, torch_.int32: 0x5A5A5A5A, torch_.int64: 0x5A5A5A5A5A5A5A5A, torch_.float32: float("nan")}
    junk = lambda shape, dtype: torch_.full(shape, poison[dtype], dtype=dtype, device="cuda")
    out, keys = junk((h, w, 3), torch_.uint8), junk((h, w), torch_.int64)
    mot, tmp = junk((h, w, 3), torch_.float32), junk((h, w, 3), torch_.float32) if fill_rounds else None
    src, cnt = (junk((h, w), torch_.uint8), junk((8,), torch_.int32)) if optional else (None, None)
    ptr = lambda x: None if x is None else x.data_ptr()
    lay = lambda f: L.EVAL_UVV if f.shape[2] == 3 else L.EVAL_DYDX
    L.call("dflow_frame_interp", h, w, d1.data_ptr(), d2.data_ptr(), dfwd.data_ptr(), lay(fwd), ptr(dbwd), lay(bwd) if bwd is not None else 0,
           float(F(t)), fill_rounds, float(occl_thresh), 0, out.data_ptr(), keys.data_ptr(), mot.data_ptr(), ptr(tmp), ptr(src), ptr(cnt),
           L.stream(d1.device))
    torch_.cuda.synchronize()
    return dict(out=out.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint64), motion=mot.cpu().numpy(),
                source=None if src is None else src.cpu().numpy(), counts=None if cnt is None else cnt.cpu().tolist())


def same(got, want, what):
    for k in ("out", "keys", "motion", "source"):
        if got[k] is None:
            continue
        npix = got[k].shape[0] * got[k].shape[1]
        g, v = (np.ascontiguousarray(x[k]).view(np.uint8).reshape(npix, -1) for x in (got, want))
        bad = np.flatnonzero((g != v).any(axis=1))
        assert bad.size == 0, "%s: %s differs at %d pixels, the first at raster index %s" % (what, k, bad.size, bad[:5])
    if got["counts"] is not None:
        assert got["counts"] == want["counts"], what


def check(torch_, img1, img2, fwd, bwd=None, what="", optional=True, **kw):
    want = R.frame_interp(img1, img2, fwd, bwd, **kw)
    same(device(torch_, img1, img2, fwd, bwd, optional=optional, **kw), want, "%s %s" % (what, kw))
    return want


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_size_layout_and_side(torch_, shape):
    h, w = shape
    img1, img2 = R.images(h, w, h * 1000 + w)
    rest = np.zeros((h, w, 3), F)
    rest[..., 2] = 1
    want = check(torch_, img1, img2, rest, rest, "at rest", fill_rounds=2)
    assert want["counts"][0] == h * w and want["counts"][7] == h * w, "every pixel claims itself, frame 1 first"
    claimed = 0
    for kind in ("int", "frac"):
        fwd, bwd = R.flow_field(h, w, 1, kind), R.flow_field(h, w, 2, kind)
        for lf in (R.UVV, R.DYDX):
            want = check(torch_, img1, img2, R.as_layout(fwd, lf), None, "%s forward only, layout %d" % (kind, lf), fill_rounds=2)
            for lb in (R.UVV, R.DYDX):
                want = check(torch_, img1, img2, R.as_layout(fwd, lf), R.as_layout(bwd, lb), "%s layouts %d %d" % (kind, lf, lb), fill_rounds=2)
                claimed += want["counts"][0] + want["counts"][1]
    assert claimed > 0 or h * w < 8


@pytest.mark.parametrize("t", R.T_VALUES)
def test_every_time(torch_, t):
    h, w = 33, 65
    img1, img2 = R.images(h, w, 7)
    assert 0 < float(F(t)) < 1
    for kind in ("int", "frac"):
        fwd, bwd = R.flow_field(h, w, 3, kind), R.as_layout(R.flow_field(h, w, 4, kind), R.DYDX)
        want = check(torch_, img1, img2, fwd, bwd, kind, t=t)
        assert want["counts"][0] > 0 and want["counts"][1] > 0 and want["counts"][7] > 0
        check(torch_, img1, img2, fwd, None, kind, t=t)


@pytest.mark.parametrize("rounds", R.FILL_ROUNDS)
def test_the_fill_rounds(torch_, rounds):
    for h, w in ((33, 65), (64, 257)):
        img1, img2 = R.images(h, w, 8)
        fwd = R.flow_field(h, w, 5, "frac")
        fwd[..., 2] *= np.random.default_rng(6).random((h, w)) < 0.005       # few claims: the holes are many rounds deep
        want = check(torch_, img1, img2, fwd, None, "%dx%d sparse" % (h, w), fill_rounds=rounds)
        assert want["counts"][0] > 0 and (want["counts"][2] > 0) == (rounds > 0)
        if rounds in (1, 8):
            assert want["counts"][3] > 0, "the rounds stop before every hole is filled"
        bwd = R.flow_field(h, w, 9, "frac")
        check(torch_, img1, img2, fwd, bwd, "%dx%d two-sided" % (h, w), fill_rounds=rounds, optional=False)


@pytest.mark.parametrize("occl", R.OCCL)
def test_the_occlusion_threshold(torch_, occl):
    h, w = 33, 65
    img1, img2 = R.images(h, w, 10)
    fwd, bwd = R.flow_field(h, w, 11, "frac"), R.flow_field(h, w, 12, "int")
    for t in (0.25, 0.75):
        want = check(torch_, img1, img2, fwd, bwd, "occl", t=t, occl_thresh=occl)
        c = want["counts"]
        assert c[4] + c[5] + c[6] == h * w
        if occl == 0.0:
            assert c[5] > c[4]
        if occl == 3e38:
            assert c[4] > 0 and c[4] > c[5]


def test_crafted_border_vectors(torch_):
    img1, img2, fwd, bwd = R.edge_case()
    for t in (0.5, 0.25):
        for back in (None, bwd):
            want = check(torch_, img1, img2, fwd, back, "edges", t=t, fill_rounds=1, occl_thresh=3e38)
            assert want["counts"][5] > 0, "some pixels have one usable side"


def test_every_source_on_one_target(torch_):
    for h, w in ((33, 65), (64, 257)):
        img1, img2 = R.images(h, w, 13)
        one = R.flow_field(h, w, 0, "one")
        want = check(torch_, img1, img2, one, one, "one target", fill_rounds=64)
        assert want["counts"][0] + want["counts"][1] == 1 and want["counts"][7] > h * w // 8
        # constant frames: every error ties at 0 and the smallest raster index wins
        flat = np.full((h, w, 3), 77, np.uint8)
        want = check(torch_, flat, flat, one, one, "one target, all errors equal", fill_rounds=0)
        assert want["counts"][0] == 1 and want["counts"][1] == 0
        assert want["keys"][h // 2, w // 3] == R.claims(flat.astype(F), flat.astype(F), one, F(0.5), 0)[1].min()


def test_nobody_takes_part(torch_):
    h, w = 33, 65
    img1, img2 = R.images(h, w, 14)
    none = R.flow_field(h, w, 0, "none")
    for back in (None, none, R.as_layout(none, R.DYDX)):
        want = check(torch_, img1, img2, none, back, "none", fill_rounds=8)
        assert want["counts"] == [0, 0, 0, h * w, 0, 0, h * w, 0]


def test_two_calls_give_the_same_bytes_and_the_wrapper_the_same_as_the_call(torch_):
    P = pkg("pipeline")
    h, w = 64, 257
    img1, img2 = R.images(h, w, 15)
    fwd, bwd = R.flow_field(h, w, 16, "frac"), R.flow_field(h, w, 17, "frac")
    a = device(torch_, img1, img2, fwd, bwd, t=0.25)
    b = device(torch_, img1, img2, fwd, bwd, t=0.25)
    same(a, b, "second call")
    frame, motion, source, counts = P.frame_interp(img1, img2, fwd, bwd, t=0.25, motion=True, source=True, counts=True)
    got = dict(out=frame.cpu().numpy(), keys=None, motion=motion.cpu().numpy(), source=source.cpu().numpy(), counts=counts.cpu().tolist())
    same(got, a, "the wrapper")
    # device tensors in, the current stream, and the defaults
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        again = P.frame_interp(*(torch_.from_numpy(x).cuda() for x in (img1, img2, fwd)))
    st.synchronize()
    assert again.cpu().numpy().tobytes() == R.frame_interp(img1, img2, fwd)["out"].tobytes()


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    h, w = 33, 65
    img1, img2 = R.images(h, w, 24)
    fwd, bwd = R.flow_field(h, w, 25, "frac"), R.flow_field(h, w, 26, "int")
    want = R.frame_interp(img1, img2, fwd, bwd, t=0.25, fill_rounds=3)
    dev = torch.device("cuda", 0)
    t1, t2, tf, tb = (torch.from_numpy(a).to(dev) for a in (img1, img2, fwd, bwd))
    out = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
    keys = torch.full((h, w), 7, dtype=torch.int64, device=dev)
    mot, tmp = (torch.full((h, w, 3), 7.0, dtype=torch.float32, device=dev) for _ in range(2))
    cnt = torch.full((8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_frame_interp", h, w, t1.data_ptr(), t2.data_ptr(), tf.data_ptr(), L.EVAL_UVV, tb.data_ptr(), L.EVAL_UVV, 0.25, 3, 30.0,
               0, out.data_ptr(), keys.data_ptr(), mot.data_ptr(), tmp.data_ptr(), None, cnt.data_ptr(), L.stream(dev))
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (keys == 7).all().item(), "a captured call must not run before the graph is replayed"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = dict(out=out.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint64), motion=mot.cpu().numpy(), source=None,
                   counts=cnt.cpu().tolist())
        same(got, want, "graph replay")


def test_frame_sequence_equals_single_calls(torch_):
    P = pkg("pipeline")
    h, w = 33, 65
    img1, img2 = R.images(h, w, 18)
    fwd, bwd = R.flow_field(h, w, 19, "frac"), R.flow_field(h, w, 20, "int")
    frames, counts = P.frame_sequence(img1, img2, fwd, bwd, n=3, fill_rounds=3, counts=True)
    for k, (frame, cnt) in enumerate(zip(frames, counts), 1):
        single, c1 = P.frame_interp(img1, img2, fwd, bwd, t=k / 4, fill_rounds=3, counts=True)
        assert frame.cpu().numpy().tobytes() == single.cpu().numpy().tobytes() and cnt.cpu().tolist() == c1.cpu().tolist()
        want = R.frame_interp(img1, img2, fwd, bwd, t=k / 4, fill_rounds=3)
        assert frame.cpu().numpy().tobytes() == want["out"].tobytes() and cnt.cpu().tolist() == want["counts"]
    assert len(P.frame_sequence(img1, img2, fwd, n=2, fill_rounds=0)) == 2


# ---- the command lines
def test_midframe_cli_equals_the_wrapper(torch_, tmp_path, monkeypatch, capsys):
    P, flowio, mf = pkg("pipeline"), pkg("flowio"), pkg("midframe")
    h, w = 33, 65
    img1, img2 = R.images(h, w, 21)
    fwd, bwd = R.flow_field(h, w, 22, "int"), R.flow_field(h, w, 23, "frac")
    bwd[..., :2] = np.where(np.isfinite(bwd[..., :2]), bwd[..., :2], 0)
    monkeypatch.chdir(tmp_path)
    np.save("a.npy", img1)
    np.save("b.npy", img2)
    np.save("fwd.npy", fwd[..., [1, 0]].astype(np.float64))                 # the hot path's [dy,dx] file
    flowio.write_flo("bwd.flo", bwd[..., :2])
    read = pkg("evaluate").ucitajFlow
    f, b = read("fwd.npy"), read("bwd.flo")
    names = record_calls(monkeypatch)
    assert mf.main(["a.npy", "b.npy", "fwd.npy", "mid.png", "--backward", "bwd.flo", "--t", "0.25", "--fill-rounds", "3",
                    "--occl-thresh", "20", "--source", "src.png"]) == 0
    assert names == ["dflow_frame_interp"]
    frame, source, counts = P.frame_interp(img1, img2, f, b, t=0.25, fill_rounds=3, occl_thresh=20, source=True, counts=True)
    assert np.array_equal(flowio.read_image("mid.png"), frame.cpu().numpy())
    assert np.array_equal(flowio.read_image("src.png"), np.array(mf.SOURCE_BGR, np.uint8)[source.cpu().numpy()])
    assert capsys.readouterr().out.strip() == mf.count_line(0.25, counts.cpu().tolist())
    want = R.frame_interp(img1, img2, f, b, t=0.25, fill_rounds=3, occl_thresh=20)
    assert frame.cpu().numpy().tobytes() == want["out"].tobytes() and counts.cpu().tolist() == want["counts"]
    del names[:]
    assert mf.main(["a.npy", "b.npy", "fwd.npy", "seq.png", "--frames", "2"]) == 0
    assert names == ["dflow_frame_interp"] * 2
    lines = capsys.readouterr().out.strip().split("\n")
    for k in (1, 2):
        single, c1 = P.frame_interp(img1, img2, f, t=k / 3, counts=True)
        assert np.array_equal(flowio.read_image("seq_%02d.png" % k), single.cpu().numpy())
        assert lines[k - 1] == mf.count_line(float(F(k / 3)), c1.cpu().tolist())


def test_run_batch_midframe(torch_, synth, tmp_path, monkeypatch, capsys):
    P, flowio, rb = pkg("pipeline"), pkg("flowio"), pkg("run_batch")
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency"], "without the option: the launches it always issued"
    assert not (tmp_path / "a" / "midframe.json").exists() and not (tmp_path / "a" / "mid_00.png").exists()
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--midframe", "--mid-fill-rounds", "4"])
    assert names == BATCH_FLOWS + ["dflow_fb_consistency", "dflow_frame_interp"]
    flows = []
    for d in (0, 1):
        flows.append(np.load(tmp_path / "b" / flowio.flow_name(0, d, 2)))
        assert np.array_equal(flows[d], np.load(tmp_path / "a" / flowio.flow_name(0, d, 2)))
    img1, img2, _ = synth.make_pair(40, 48, seed=synth.pair_seed(0, 0))
    want = R.frame_interp(img1, img2, flows[0].astype(F), flows[1].astype(F), t=0.5, fill_rounds=4, occl_thresh=30.0)
    got = flowio.read_image(str(tmp_path / "b" / "mid_00.png"))
    assert np.array_equal(got, want["out"])
    truth, mask = synth.make_mid(40, 48, seed=synth.pair_seed(0, 0), t=0.5)
    blend = np.floor(F(0.5) * img1.astype(F) + F(0.5) * img2.astype(F) + F(0.5)).astype(np.uint8)
    mj = json.load(open(tmp_path / "b" / "midframe.json"))
    assert mj["size"] == [40, 48] and mj["bcd_times"] == 2 and mj["t"] == 0.5 and mj["fill_rounds"] == 4 and mj["occl_thresh"] == 30.0
    row, = mj["pairs"]
    assert row["pair"] == 0 and list(row["counts"].values()) == want["counts"] and list(row["counts"]) == list(R.COUNTS)
    assert row["n"] == int(mask.sum())
    assert abs(row["psnr"] - R.psnr(want["out"], truth, mask)) < 1e-9 and abs(row["psnr_blend"] - R.psnr(blend, truth, mask)) < 1e-9
    printed = capsys.readouterr().out
    assert "pair 0: middle frame from1=%d from2=%d" % tuple(want["counts"][:2]) in printed
    assert "PSNR %.2f dB, plain blend %.2f dB, over %d px" % (row["psnr"], row["psnr_blend"], row["n"]) in printed
