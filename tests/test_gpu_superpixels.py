"""dflow_superpixels and dflow_segment_fit on the device against their numpy restatements (tests/superpixel_ref.py), byte for
byte on every output plane and count, with every plane exact-size between guards at its lowest alignment (ws_guard.GuardedWs);
the properties the header promises checked with this file's own search, independently of the restatement; the recovery of a
piecewise-affine field under gross outliers; a graph capture.  Shapes are chosen where the kernels can go wrong (ragged cells
and tiles, one row, one column, one centre, the most centres per tile, more block sums than the scan's block has threads), not
where the workload lives.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import superpixel_ref as R
import ws_guard as G
from conftest import pkg

pytestmark = pytest.mark.gpu
F32 = np.float32
POISON = 0xFF


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


# ------------------------------------------------------------------------------------------------ placed calls
class Placed:
    """Device planes of one call, each exactly its bytes between guards, `align` bytes past a 256-byte boundary."""

    def __init__(self, torch):
        self.torch, self.dev, self.planes = torch, torch.device("cuda", 0), {}

    def put(self, name, align, data=None, dtype=None, shape=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype, shape = data.dtype, data.shape
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        g = G.GuardedWs(self.torch, nbytes, POISON, self.dev, offset=align)
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


def device_superpixels(torch, img, S, m, iters, min_size):
    L = pkg("_lib")
    h, w, _ = img.shape
    K = R.grid(h, w, S)[2]
    P = Placed(torch)
    i32 = np.int32
    args = [P.put("bgr", 1, img), S, m, iters, min_size, 0, P.put("label", 4, None, i32, (h, w)), P.put("centers", 4, None, i32, (K, 8)),
            P.put("slic", 4, None, i32, (h, w)), P.put("counts", 4, None, i32, (8,)), P.put("sums", 4, None, i32, (K, 8)),
            P.put("comp", 4, None, i32, (h, w)), P.put("size", 4, None, i32, (h, w)), P.put("final", 4, None, i32, (h, w)),
            P.put("scan", 4, None, i32, (R.scan_len(h, w),))]
    L.call("dflow_superpixels", h, w, *args, L.stream(P.dev))
    P.check("dflow_superpixels %dx%d S=%d" % (w, h, S))
    return {k: P.get(k) for k in ("label", "centers", "slic", "counts")}


def device_fit(torch, flow, label, n_seg, thresh, rounds):
    L = pkg("_lib")
    h, w, c = flow.shape
    P = Placed(torch)
    args = [P.put("flow", 4, flow), L.EVAL_UVV if c == 3 else L.EVAL_DYDX, P.put("labels", 4, label), n_seg, float(thresh), rounds, 0,
            P.put("models", 4, None, F32, (n_seg, 6)), P.put("seg_counts", 4, None, np.int32, (n_seg, 4)),
            P.put("out", 4, None, F32, (h, w, 3)), P.put("cls", 1, None, np.uint8, (h, w)), P.put("counts", 4, None, np.int32, (8,)),
            P.put("acc", 8, None, np.int64, (n_seg, 12))]
    L.call("dflow_segment_fit", h, w, *args, L.stream(P.dev))
    P.check("dflow_segment_fit %dx%d n_seg=%d" % (w, h, n_seg))
    assert not P.get("acc").any(), "every round leaves d_acc zeroed"
    return {k: P.get(k) for k in ("models", "seg_counts", "out", "cls", "counts")}


def same(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        nd = int((a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)).sum())
        assert nd == 0, "%s: %s differs in %d of %d bytes" % (what, k, nd, a.nbytes)


# ------------------------------------------------------------------------------------------------ images
def image(content, h, w, synth):
    if content == "uniform":
        return np.full((h, w, 3), 131, np.uint8)
    if content == "stripes":                          # 2-pixel diagonal stripes: SLIC labels fall apart into many components
        yy, xx = np.mgrid[0:h, 0:w]
        return np.where((((xx + yy) // 2) % 2 == 0)[..., None], np.uint8(20), np.uint8(230)) * np.ones(3, np.uint8)
    if content == "noise":
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert content == "synth"
    return np.ascontiguousarray(synth.make_pair(max(h, 16), max(w, 16), seed=3)[0][:h, :w])


# h, w, S, m, iters, min_size, content
CASES = [(37, 53, 8, 10, 10, 16, "synth"), (37, 53, 8, 10, 2, 64, "noise"), (37, 53, 8, 10, 10, 8, "noise"), (37, 53, 8, 0, 1, 0, "stripes"),
         (37, 53, 8, 10, 10, 8, "uniform"),
         (1, 70, 4, 10, 10, 4, "noise"), (1, 70, 4, 10, 2, 0, "uniform"), (70, 1, 4, 10, 10, 4, "noise"), (70, 1, 4, 255, 1, 1, "stripes"),
         (5, 6, 64, 10, 10, 8, "noise"), (5, 6, 64, 10, 1, 0, "uniform"),
         (64, 96, 16, 0, 10, 64, "synth"), (64, 96, 16, 10, 10, 64, "synth"), (64, 96, 16, 255, 10, 64, "synth"),
         (64, 96, 16, 10, 2, 256, "noise"), (64, 96, 16, 10, 1, 1, "noise"), (64, 96, 16, 10, 10, 8, "stripes"),
         (48, 80, 4, 10, 10, 4, "synth"), (48, 80, 4, 10, 2, 16, "noise"), (48, 80, 4, 0, 10, 0, "noise"), (48, 80, 4, 255, 10, 8, "uniform"),
         (33, 67, 5, 30, 2, 1 << 26, "noise"),
         # the smallest frame whose 259 block sums are more than one per thread of the scan's block, the last chunk ragged;
         # 3876 final roots over those blocks (one iteration: the restatement takes a third of a second)
         (257, 257, 8, 10, 1, 3, "noise")]


def own_components(lab):
    """This file's own flood fill (a stack, 4 neighbours): the number of connected pieces of every value."""
    h, w = lab.shape
    seen = np.zeros((h, w), bool)
    pieces = {}
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0]:
                continue
            v = lab[y0, x0]
            pieces[v] = pieces.get(v, 0) + 1
            stack = [(y0, x0)]
            seen[y0, x0] = True
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx] and lab[yy, xx] == v:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
    return pieces


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_S%d_m%d_i%d_min%d_%s" % c)
def test_superpixels_are_the_restatement_byte_for_byte_and_keep_their_promises(torch_, synth, case):
    h, w, S, m, iters, min_size, content = case
    img = image(content, h, w, synth)
    want = R.superpixels(img, S, m, iters, min_size)
    got = device_superpixels(torch_, img, S, m, iters, min_size)
    print("%s: K %d, counts %s" % (case, want["centers"].shape[0], got["counts"].tolist()))
    same(got, want, str(case))
    same(device_superpixels(torch_, img, S, m, iters, min_size), got, "a second call")
    # the promises, from the device's planes alone
    lab, cnt = got["label"], got["counts"].tolist()
    n_seg = cnt[5]
    pieces = own_components(lab)
    assert sorted(pieces) == list(range(n_seg)) and set(pieces.values()) == {1}, "every segment is one 4-connected piece, numbered 0..n_seg-1"
    first = [int(np.flatnonzero(lab.ravel() == s)[0]) for s in range(n_seg)]
    assert first == sorted(first) and first[0] == 0, "numbered in the order of their first pixels"
    sizes = np.bincount(lab.ravel(), minlength=n_seg)
    assert (sizes[1:] >= min_size).all() and sizes.max() == cnt[6] and sizes.sum() == h * w
    raw_pieces = own_components(got["slic"])
    assert cnt[0] == R.grid(h, w, S)[2] and cnt[2] == sum(raw_pieces.values()) and cnt[3] <= cnt[2] and cnt[7] == 0
    assert cnt[5] >= cnt[2] - cnt[3] and cnt[5] <= cnt[2] - cnt[3] + 1, "the finals are the components that are not small, and maybe pixel 0's"
    assert got["centers"][:, 5].sum() == h * w and cnt[1] == int((got["centers"][:, 5] == 0).sum()) and not got["centers"][:, 6:].any()
    assert 0 <= got["slic"].min() and got["slic"].max() < cnt[0]
    if min_size <= 1:
        assert cnt[3] == 0 and cnt[4] == 0 and n_seg == cnt[2], "min_size 0 or 1 merges nothing"
    if min_size == 1 << 26:
        assert n_seg == 1 and cnt[4] == h * w - np.count_nonzero(R.components(got["slic"])[0] == 0)


# ------------------------------------------------------------------------------------------------ the fit
def dirty_flow(h, w, seed, layout3):
    """A field with holes, NaN and +-Inf vectors and vectors just inside and just outside the 32768 range."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    U = np.rint((0.05 * xx - 0.02 * yy + 1.5 + rng.normal(0, 0.4, (h, w))) * 64) / 64
    V = np.rint((0.03 * yy + 0.01 * xx - 0.75 + rng.normal(0, 0.4, (h, w))) * 64) / 64
    f = np.stack([U, V, np.ones((h, w))], axis=2).astype(F32)
    out = rng.random((h, w)) < 0.1                     # gross outliers
    f[out, 0] += F32(25.0)
    pick = rng.permutation(h * w)
    flat = f.reshape(-1, 3)
    specials = [(np.nan, 0.5), (0.25, np.nan), (np.inf, 1.0), (1.0, -np.inf), (32768.0, -32768.0), (-32768.0, 0.0), (32768.004, 0.0),
                (0.0, -32770.0), (1e30, 1.0), (3.4e38, -3.4e38)]
    for k, (u, v) in enumerate(specials * 2):
        flat[pick[k], :2] = (u, v)
    holes = pick[len(specials) * 2: len(specials) * 2 + h * w // 6]
    if layout3:
        flat[holes] = (7.0, -7.0, 0.0)                 # not valid: the numbers are not looked at
        flat[pick[-3:], 2] = (0.5, 0.25, np.nan)       # valid needs > 0.5
        return f
    flat[holes, 0] = np.nan
    return np.ascontiguousarray(f[..., [1, 0]])


def hand_labels(h, w, n_seg):
    """Blocks of 11 x 7 pixels numbered modulo n_seg + 3 from -2: labels below 0 and at or above n_seg are out of range."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // 7) * -(-w // 11) + xx // 11) % (n_seg + 3) - 2).astype(np.int32)


@pytest.mark.parametrize("rounds", [1, 3, 6])
@pytest.mark.parametrize("layout3", [True, False], ids=["uvv", "dydx"])
def test_the_fit_is_the_restatement_byte_for_byte(torch_, synth, layout3, rounds):
    h, w = 37, 53
    flow = dirty_flow(h, w, 11 + rounds, layout3)
    sp = R.superpixels(image("synth", h, w, synth), 8, 10, 5, 16)
    cases = [("superpixels", sp["label"], int(sp["counts"][5]), 1.0), ("hand", hand_labels(h, w, 9), 9, 1.0),
             # so small that segments lose every vector after round 0 and keep the model they had
             ("tiny thresh", hand_labels(h, w, 9), 9, 2.0 ** -12), ("one segment", np.zeros((h, w), np.int32), 1, 0.5),
             ("more segments than labels", sp["label"], int(sp["counts"][5]) + 300, 1.0)]
    for name, label, n_seg, thresh in cases:
        want = R.segment_fit(flow, label, n_seg, thresh, rounds)
        got = device_fit(torch_, flow, label, n_seg, thresh, rounds)
        what = "%s, R=%d, %s" % (name, rounds, "uvv" if layout3 else "dydx")
        print("%s: counts %s" % (what, got["counts"].tolist()))
        same(got, want, what)
        cls, cnt, sc = got["cls"], got["counts"].tolist(), got["seg_counts"]
        with_model = np.isin(label, np.flatnonzero(sc[:, 3] != 0)) & (label >= 0) & (label < n_seg)
        assert np.count_nonzero(cls == 1) + np.count_nonzero(cls == 2) == np.count_nonzero((cls != 0) & with_model)
        assert cnt[0] == np.count_nonzero(cls != 0) == sc[:, 1].sum() and cnt[1] == np.count_nonzero(cls == 1) == sc[:, 2].sum()
        assert cnt[2] == cnt[3] + cnt[4] and cnt[5] == np.count_nonzero((label < 0) | (label >= n_seg)) and cnt[6] >= 4
        assert sc[:, 0].sum() == h * w - cnt[5] and (got["out"][..., 2] == with_model).all()
        if name == "tiny thresh" and rounds > 1:
            assert ((sc[:, 1] > 0) & (sc[:, 2] == 0) & (sc[:, 3] != 0)).any(), "a segment that lost every vector keeps its model"
    same(device_fit(torch_, flow, label, n_seg, thresh, rounds), got, "a second call")


# ------------------------------------------------------------------------------------------------ recovery
RECOVERY = dict(h=48, w=64, fraction=0.15, seed=5, rounds=6, thresh=1.0)
# the restatement's largest coefficient error against the truth over the segments of at least 16 members, measured on the CPU with
# RECOVERY: it recovers them exactly, the last round holding inliers alone whose flow is exact on the 1/64 grid
RECOVERY_REF_ERROR = 0.0


def recovery_case(h, w, fraction, seed, **_):
    """A piecewise-affine flow, exact on the 1/64 grid, over blocks of 16 x 16 pixels with three small segments cut out of them,
    and `fraction` of the vectors replaced by gross outliers: (flow [U,V,valid], labels, n_seg, true models)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    label = ((yy // 16) * (w // 16) + xx // 16).astype(np.int32)
    n_big = int(label.max()) + 1
    label[5, 5:8], label[20, 40:50], label[40:42, 10] = n_big, n_big + 1, n_big + 2          # 3, 10 and 2 members
    n_seg = n_big + 3
    truth = np.zeros((n_seg, 6), np.float64)
    truth[:, [0, 1, 3, 4]] = rng.integers(-8, 9, (n_seg, 4)) / 64.0
    truth[:, [2, 5]] = rng.integers(-256, 257, (n_seg, 2)) / 64.0
    t = truth[label]
    U, V = t[..., 0] * xx + t[..., 1] * yy + t[..., 2], t[..., 3] * xx + t[..., 4] * yy + t[..., 5]
    assert np.array_equal(U * 64, np.rint(U * 64)) and np.array_equal(V * 64, np.rint(V * 64))
    bad = rng.random((h, w)) < fraction
    U = np.where(bad, U + rng.choice([-1.0, 1.0], (h, w)) * rng.integers(40 * 64, 80 * 64, (h, w)) / 64.0, U)
    V = np.where(bad, V + rng.choice([-1.0, 1.0], (h, w)) * rng.integers(40 * 64, 80 * 64, (h, w)) / 64.0, V)
    return np.stack([U, V, np.ones((h, w))], axis=2).astype(F32), label, n_seg, truth.astype(F32)


def test_a_piecewise_affine_field_is_recovered_under_gross_outliers(torch_):
    flow, label, n_seg, truth = recovery_case(**RECOVERY)
    want = R.segment_fit(flow, label, n_seg, RECOVERY["thresh"], RECOVERY["rounds"])
    got = device_fit(torch_, flow, label, n_seg, RECOVERY["thresh"], RECOVERY["rounds"])
    same(got, want, "recovery")
    big = got["seg_counts"][:, 0] >= 16
    assert big.sum() == 12 and (got["seg_counts"][big, 3] == 2).all()
    err = float(np.abs(got["models"][big].astype(np.float64) - truth[big]).max())
    print("largest coefficient error over %d segments: %g (the restatement's, measured: %g)" % (big.sum(), err, RECOVERY_REF_ERROR))
    assert err <= 4 * RECOVERY_REF_ERROR


# ------------------------------------------------------------------------------------------------ a graph
def test_both_calls_captured_into_a_graph_and_replayed(torch_, synth):
    torch, L = torch_, pkg("_lib")
    h, w, S = 37, 53, 8
    img, flow = image("synth", h, w, synth), dirty_flow(h, w, 4, True)
    sp = R.superpixels(img, S, 10, 3, 16)
    n_seg = int(sp["counts"][5])
    fit = R.segment_fit(flow, sp["label"], n_seg, 1.0, 3)
    dev = torch.device("cuda", 0)
    K = R.grid(h, w, S)[2]
    i32 = torch.int32
    new = lambda n, dt=i32: torch.full((n,), -7, dtype=dt, device=dev)                     # noqa: E731
    timg, tflow = (torch.from_numpy(a.reshape(-1)).to(dev) for a in (img, flow))
    label, centers, slic, cnt, sums, comp, size, fin, scan = (new(n) for n in (h * w, K * 8, h * w, 8, K * 8, h * w, h * w, h * w,
                                                                              R.scan_len(h, w)))
    models, segc, out, cls, fcnt, acc = (new(n_seg * 6, torch.float32), new(n_seg * 4), new(h * w * 3, torch.float32),
                                         torch.full((h * w,), 9, dtype=torch.uint8, device=dev), new(8), new(n_seg * 12, torch.int64))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st = L.stream(dev)
        L.call("dflow_superpixels", h, w, timg.data_ptr(), S, 10, 3, 16, 0, label.data_ptr(), centers.data_ptr(), slic.data_ptr(),
               cnt.data_ptr(), sums.data_ptr(), comp.data_ptr(), size.data_ptr(), fin.data_ptr(), scan.data_ptr(), st)
        L.call("dflow_segment_fit", h, w, tflow.data_ptr(), L.EVAL_UVV, label.data_ptr(), n_seg, 1.0, 3, 0, models.data_ptr(), segc.data_ptr(),
               out.data_ptr(), cls.data_ptr(), fcnt.data_ptr(), acc.data_ptr(), st)
    torch.cuda.synchronize()
    assert (cnt == -7).all().item() and (label == -7).all().item() and (fcnt == -7).all().item(), "a captured call runs at the replay"
    graph.replay()
    torch.cuda.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()                                              # noqa: E731
    for t, a in ((label, sp["label"]), (centers, sp["centers"]), (slic, sp["slic"]), (cnt, sp["counts"]), (models, fit["models"]),
                 (segc, fit["seg_counts"]), (out, fit["out"]), (cls, fit["cls"]), (fcnt, fit["counts"])):
        assert raw(t) == np.ascontiguousarray(a).tobytes()


def test_the_wrappers_and_the_cli_on_the_device(torch_, synth, tmp_path, capsys):
    P, sp_cli, flowio = pkg("pipeline"), pkg("superpixels"), pkg("flowio")
    h, w = 37, 53
    img, flow = image("synth", h, w, synth), dirty_flow(h, w, 4, False)
    want = R.superpixels(img, 8, 10, 10, 16)
    lab, cen, raw, cnt = P.superpixels(img, step=8, centers=True, slic=True, counts=True)
    same(dict(label=lab.cpu().numpy(), centers=cen.cpu().numpy(), slic=raw.cpu().numpy(), counts=cnt.cpu().numpy()), want, "superpixels")
    n_seg = int(want["counts"][5])
    fit = R.segment_fit(flow, want["label"], n_seg, 1.0, 3)
    res = P.superpixel_flow(img, flow, step=8, classes=True, counts=True)
    assert res[1].shape[0] == n_seg
    same(dict(zip(("label", "models", "seg_counts", "out", "cls", "counts"), (t.cpu().numpy() for t in res))),
         dict(fit, label=want["label"]), "superpixel_flow")
    np.save(tmp_path / "i.npy", img)
    np.save(tmp_path / "f.npy", flow)
    argv = [str(tmp_path / "i.npy"), str(tmp_path / "l.npy"), "--step", "8", "--boundaries", str(tmp_path / "b.png"), "--flow",
            str(tmp_path / "f.npy"), "--fit", str(tmp_path / "o.npy"), "--classes", str(tmp_path / "c.png"), "--models", str(tmp_path / "m.npy"),
            "--json"]
    assert sp_cli.main(argv) == 0
    rep = __import__("json").loads(capsys.readouterr().out)
    assert rep["n_seg"] == n_seg and rep["agree"] == int(fit["counts"][1]) and rep["affine"] == int(fit["counts"][3])
    assert np.array_equal(np.load(tmp_path / "l.npy"), want["label"]) and np.load(tmp_path / "o.npy").tobytes() == fit["out"].tobytes()
    assert np.load(tmp_path / "m.npy").tobytes() == fit["models"].tobytes()
    assert np.array_equal(flowio.read_png8(str(tmp_path / "c.png"))[..., 0], fit["cls"] * 85)
    assert flowio.read_png8(str(tmp_path / "b.png")).shape == (h, w, 3)
    assert sp_cli.main([str(tmp_path / "i.npy"), str(tmp_path / "l.png"), "--step", "8"]) == 0 and "segments: %d" % n_seg in capsys.readouterr().out
    assert np.array_equal(flowio.read_png8(str(tmp_path / "l.png")), sp_cli.label_picture(want["label"], np))
