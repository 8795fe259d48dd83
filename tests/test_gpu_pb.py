"""dflow_pb_edges (csrc/pb_edges.hip) against the numpy restatement pb_ref.py, and the drop-ins built on it: pipeline.pb_edges,
edge.pb_ivice and spremiZaEpic.main(... 'pb', '--gpu-epic').  Run with `pytest -m gpu`.

Tolerance against the float64 reference: 1e-5.  An m_o is at most 48 correctly rounded float32 divisions and about 60
additions and multiplications of terms <= 1: below 110 * 2^-24 = 6.6e-6.  The float32 variant of the reference performs the
same IEEE operations in the same order, so it is asserted bit for bit as well.
The kernel's tile is 32x8 pixels: 19x71 spans three tiles each way and is a multiple of neither."""
import ctypes as C
import os

import numpy as np
import pytest

import pb_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

TOL = 1e-5
MULTI = (19, 71)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def random_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


_refs = {}


def reference(key, img, radius):
    """pb_ref of (img, radius), computed once per key and shared read-only."""
    if key not in _refs:
        (e64, m64), (e32, m32) = R.pb_both(img, radius)
        for a in (e64, m64, e32, m32):
            a.setflags(write=False)
        _refs[key] = (e64, m64, e32, m32)
    return _refs[key]


def gpu_pb(img, radius=5):
    e, m = pkg("pipeline").pb_edges(img, radius, per_orientation=True)
    return e.cpu().numpy(), m.cpu().numpy()


def check(key, img, radius=5):
    e, m = gpu_pb(img, radius)
    e64, m64, e32, m32 = reference(key, img, radius)
    assert e.shape == e64.shape and m.shape == m64.shape and e.dtype == np.float32 and m.dtype == np.float32
    de, dm = np.abs(e - e64).max(), np.abs(m - m64).max()
    print("%s R=%d: |e - e64| %.3g, |m - m64| %.3g, e bits differ from float32 ref at %d px, m at %d values"
          % (key, radius, de, dm, (e.view(np.uint32) != e32.view(np.uint32)).sum(),
             (m.view(np.uint32) != m32.view(np.uint32)).sum()))
    assert de <= TOL and dm <= TOL
    assert e.tobytes() == e32.tobytes() and m.tobytes() == m32.tobytes()
    return e, m


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (3, 3)])
def test_frames_smaller_than_the_disc(torch_, size):
    check("random%dx%d" % size, random_image(*size, seed=size[0] * 16 + size[1]))


@pytest.mark.parametrize("radius", [1, 5, 7])
def test_frame_of_one_disc(torch_, radius):
    n = 2 * radius + 1
    check("disc%d" % radius, random_image(n, n, seed=radius), radius)


@pytest.mark.parametrize("radius", [1, 2, 5, 7])
def test_partial_tiles_every_radius(torch_, radius):
    e, _ = check("multi_r%d" % radius, random_image(*MULTI, seed=3), radius)
    assert e.max() > 0.3


@pytest.mark.parametrize("radius", [3, 4, 6])
def test_remaining_radii(torch_, radius):
    check("small_r%d" % radius, random_image(11, 37, seed=radius), radius)


@pytest.mark.parametrize("name", ["a40x48_c5x6", "b36x40_c9x8", "c45x35_c9x7"])
def test_golden_first_images(torch_, golden, name):
    img = np.ascontiguousarray(golden(name)["img1"])
    assert img.dtype == np.uint8 and img.ndim == 3
    check(name, img)


def test_flat_image_is_exactly_zero(torch_):
    for v in ((0, 0, 0), (255, 255, 255), (16, 239, 15)):
        img = np.empty(MULTI + (3,), np.uint8)
        img[:] = v
        e, m = gpu_pb(img)
        assert not e.any() and not m.any() and not np.signbit(e).any()


def test_channels_at_bin_boundaries(torch_):
    img = R.boundary_frame(*MULTI, seed=4)
    assert set(np.unique(img)) <= {0, 15, 16, 239, 240, 255}
    e, _ = check("boundary", img)
    assert e.max() > 0.3


def test_two_region_boundary(torch_):
    e, _ = check("two_region", R.two_region_frame())
    assert e[:, 27:29].mean() >= 3 * e[:, 5:20].mean()


def raw_call(torch, bgr, radius, e, m, ws, ws_bytes):
    L = pkg("_lib")
    H, W, _ = bgr.shape
    return L.lib().dflow_pb_edges(H, W, bgr.data_ptr(), radius, e.data_ptr(), m.data_ptr() if m is not None else None,
                                  ws.data_ptr() if ws is not None else None, ws_bytes,
                                  C.c_void_p(torch.cuda.current_stream(bgr.device).cuda_stream))


def test_null_orientation_plane_repeat_and_canaries(torch_):
    torch = torch_
    L = pkg("_lib")
    H, W = MULTI
    img = random_image(H, W, seed=3)
    e64, m64, e32, m32 = reference("multi_r5", img, 5)
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(img).to(dev)
    n = H * W
    wsb = L.lib().dflow_pb_workspace_bytes(H, W)
    ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device=dev)
    e = torch.full((n + 64,), -7.0, dtype=torch.float32, device=dev)
    m = torch.full((n * 8 + 64,), -7.0, dtype=torch.float32, device=dev)
    L.check(raw_call(torch, bgr, 5, e, None, ws, wsb), "dflow_pb_edges")         # without the (h,w,8) plane
    torch.cuda.synchronize()
    first = e[:n].cpu().numpy().tobytes()
    assert first == e32.tobytes()
    assert (m == -7.0).all().item() and (e[n:] == -7.0).all().item() and (ws[wsb:] == 0xA5).all().item()
    e[:n] = -7.0
    L.check(raw_call(torch, bgr, 5, e, m, ws, wsb), "dflow_pb_edges")            # with it, on the used workspace: the same e
    torch.cuda.synchronize()
    assert e[:n].cpu().numpy().tobytes() == first and m[:n * 8].cpu().numpy().tobytes() == m32.tobytes()
    assert (m[n * 8:] == -7.0).all().item() and (e[n:] == -7.0).all().item() and (ws[wsb:] == 0xA5).all().item()
    e2 = torch.empty(n, dtype=torch.float32, device=dev)
    m2 = torch.empty(n * 8, dtype=torch.float32, device=dev)
    L.check(raw_call(torch, bgr, 5, e2, m2, ws, wsb), "dflow_pb_edges")          # twice: the same bytes
    torch.cuda.synchronize()
    assert e2.cpu().numpy().tobytes() == first and m2.cpu().numpy().tobytes() == m32.tobytes()


def test_workspace_one_byte_short_is_refused_and_writes_nothing(torch_):
    torch = torch_
    L = pkg("_lib")
    H, W = MULTI
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(random_image(H, W, seed=3)).to(dev)
    wsb = L.lib().dflow_pb_workspace_bytes(H, W)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=dev)
    e = torch.full((H * W,), -7.0, dtype=torch.float32, device=dev)
    m = torch.full((H * W * 8,), -7.0, dtype=torch.float32, device=dev)
    assert raw_call(torch, bgr, 5, e, m, ws, wsb - 1) == -2 and b"workspace" in L.lib().dflow_last_error()
    assert raw_call(torch, bgr, 5, e, m, None, wsb) == -2
    torch.cuda.synchronize()
    assert (e == -7.0).all().item() and (m == -7.0).all().item() and (ws == 0xA5).all().item()


def test_captured_into_a_graph_on_a_side_stream(torch_):
    torch = torch_
    L = pkg("_lib")
    H, W = MULTI
    img = random_image(H, W, seed=3)
    e64, m64, e32, m32 = reference("multi_r5", img, 5)
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(img).to(dev)
    wsb = L.lib().dflow_pb_workspace_bytes(H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    e = torch.full((H, W), -7.0, dtype=torch.float32, device=dev)
    m = torch.full((H, W, 8), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert torch.cuda.current_stream(dev) == side
        L.check(raw_call(torch, bgr, 5, e, m, ws, wsb), "dflow_pb_edges")
    torch.cuda.synchronize()
    assert (e == -7.0).all().item(), "a captured call must not run before the graph is replayed"
    graph.replay()
    torch.cuda.synchronize()
    assert e.cpu().numpy().tobytes() == e32.tobytes() and m.cpu().numpy().tobytes() == m32.tobytes()


def test_runs_on_a_side_stream_without_waiting(torch_, synth):
    torch = torch_
    img = synth.make_pair(120, 200, seed=6)[0]
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(img).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=dev)
        for _ in range(8):
            big = big @ big.T / 4096.0                      # keeps the side stream busy well past the host call
        e = pkg("pipeline").pb_edges(bgr)
        pending = not side.query()
    side.synchronize()
    assert pending, "pb_edges waited for its stream"
    e64 = reference("synth120x200", img, 5)[0]
    assert np.abs(e.cpu().numpy() - e64).max() <= TOL


def test_edge_pb_ivice_writes_one_minus_e(torch_, synth, tmp_path):
    from PIL import Image
    img = synth.make_pair(40, 56, seed=8)[0]
    png = os.path.join(tmp_path, "a.png")
    Image.fromarray(img[..., ::-1].copy()).save(png)                     # BGR -> RGB on disk
    out = os.path.join(tmp_path, "ivice.bin")
    edge = pkg("edge")
    data = edge.pb_ivice(png, out)
    e32 = reference("synth40x56", img, 5)[2]
    want = (np.float32(1.0) - e32).astype(np.float32)
    assert open(out, "rb").read() == want.tobytes() and data.tobytes() == want.tobytes()
    assert edge.pb_strength_tensor(png).cpu().numpy().tobytes() == e32.tobytes()
    out3 = os.path.join(tmp_path, "ivice3.bin")
    edge.pb_ivice(png, out3, radius=3)
    assert open(out3, "rb").read() == (np.float32(1.0) - reference("synth40x56_r3", img, 3)[2]).tobytes()


@pytest.mark.parametrize("tail", [["--gpu-epic"], ["--gpu-epic", "--prefilter"]])
def test_spremi_za_epic_pb_gpu_epic(torch_, tmp_path, monkeypatch, capsys, synth, tail):
    torch = torch_
    H, W = 40, 56
    rng = np.random.default_rng(12)
    fwd = rng.integers(-4, 5, (H, W, 2)).astype(np.float64)
    bwd = np.where(rng.random((H, W, 1)) < 0.7, -fwd, rng.integers(-4, 5, (H, W, 2))).astype(np.float64)
    img1 = synth.make_pair(H, W, seed=8)[0]
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img1[..., ::-1].copy()).save("a.png")
    Image.fromarray(img1[..., ::-1].copy()).save("b.png")
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    assert pkg("spremiZaEpic").main(["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "pb"] + tail) == 0
    assert "epic.flo written" in capsys.readouterr().out
    pipeline = pkg("pipeline")
    dev = torch.device("cuda", 0)
    e = pipeline.pb_edges(img1)
    e_host = e.cpu().numpy()
    assert e_host.tobytes() == reference("synth40x56", img1, 5)[2].tobytes()
    assert open("ivice.bin", "rb").read() == (np.float32(1.0) - e_host).tobytes()
    sparse = pipeline.fb_consistency(torch.from_numpy(fwd.astype(np.float32)).to(dev),
                                     torch.from_numpy(bwd.astype(np.float32)).to(dev), 3)
    assert np.array_equal(np.load("sparse_field.npy"), sparse.cpu().numpy()) and 0 < sparse[..., 2].sum().item() < H * W
    if "--prefilter" in tail:
        sparse = pipeline.epic_prefilter(sparse, e, img1)
    want = pipeline.epic_interpolate(sparse, e).cpu().numpy()            # e itself, not 1 - e
    got = pkg("flowio").read_flo("epic.flo")[..., ::-1]                  # the file holds [u,v], the tensor [dy,dx]
    assert got.shape == want.shape and np.array_equal(got, want)
    other = pipeline.epic_interpolate(sparse, 1.0 - e).cpu().numpy()
    assert not np.array_equal(other, want), "the pair cannot tell e from 1 - e"


def test_run_batch_edge_kind_pb(torch_, synth, tmp_path):
    H, W = 48, 64
    rb = pkg("run_batch")
    rb.main(["--pairs", "1", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--out", str(tmp_path), "--edges", "--epic",
             "--edge-kind", "pb"])
    img1 = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))[0]
    e32 = reference("batch48x64", img1, 5)[2]
    assert open(os.path.join(tmp_path, "ivice_00.bin"), "rb").read() == (np.float32(1.0) - e32).tobytes()
    pipeline = pkg("pipeline")
    sparse = np.load(os.path.join(tmp_path, "sparse_field_00.npy"))
    want = pipeline.epic_interpolate(sparse, pipeline.pb_edges(img1)).cpu().numpy()
    assert np.array_equal(pkg("flowio").read_flo(os.path.join(tmp_path, "epic_00.flo"))[..., ::-1], want)
