"""dflow_canny_edges (csrc/edges.hip) against the numpy restatement canny_ref.py, byte for byte, and the drop-ins built on it:
edge.canny_ivice, spremiZaEpic.main and run_batch --edges.  Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import ndimage

import canny_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def gpu_edges(img, low=100, high=200):
    e, iv = pkg("pipeline").canny_edges(img, low, high)
    return e.cpu().numpy(), iv.cpu().numpy()


def check(img, low=100, high=200):
    e, iv = gpu_edges(img, low, high)
    ref = R.canny(img, low, high)
    assert e.shape == ref.shape and e.dtype == np.uint8
    bad = np.argwhere(e != ref)
    assert bad.size == 0, "%d pixels differ, first at %s" % (len(bad), bad[:5].tolist())
    assert iv.dtype == np.float32 and iv.tobytes() == R.ivice(ref).tobytes()
    return ref


def noise_image(H, W, seed, smooth=1.0):
    rng = np.random.default_rng(seed)
    a = rng.random((H, W, 3)) * 255
    if smooth:
        a = ndimage.gaussian_filter(a, (smooth, smooth, 0))
        a = (a - a.min()) * (255.0 / max(np.ptp(a), 1e-9))
    return np.ascontiguousarray(a.astype(np.uint8))


@pytest.mark.parametrize("style", ["dense", "low_texture"])
@pytest.mark.parametrize("size", [(436, 1024), (375, 1242)])
def test_synth_frames(torch_, synth, size, style):
    img = synth.make_pair(*size, seed=5, style=style)[0]
    check(img)
    assert check(img, 20, 50).mean() > 0.05 * 255                      # the smooth synthetic texture at lower thresholds


def test_large_frame_many_tiles(torch_, synth):
    base = synth.make_pair(540, 960, seed=9)[0]
    img = np.ascontiguousarray(np.tile(base, (4, 4, 1)))
    assert img.shape == (2160, 3840, 3)
    check(img)
    assert check(img, 20, 50).any()


@pytest.mark.parametrize("size", [(1, 1), (1, 17), (17, 1), (2, 2), (3, 5), (8, 8), (33, 65)])
@pytest.mark.parametrize("seed", [0, 1])
def test_small_and_partial_tiles(torch_, size, seed):
    img = noise_image(*size, seed, smooth=0)
    for low, high in ((100, 200), (10, 30), (0, 0)):
        check(img, low, high)


@pytest.mark.parametrize("low,high", [(100, 200), (0, 0), (200, 100), (10, 1000), (100.5, 200.9), (20, 40), (40.7, 20.2)])
def test_thresholds(torch_, synth, low, high):
    img = synth.make_pair(375, 1242, seed=3)[0]
    check(img, low, high)


def test_swapped_and_fractional_thresholds_are_the_integer_ones(torch_, synth):
    img = synth.make_pair(120, 200, seed=4)[0]
    e = gpu_edges(img, 100, 200)[0]
    assert np.array_equal(gpu_edges(img, 200, 100)[0], e) and np.array_equal(gpu_edges(img, 100.5, 200.9)[0], e)


def test_noise_component_spans_the_frame(torch_):
    img = noise_image(375, 1242, 11, smooth=0)
    ref = check(img, 10, 200)
    lab, _ = ndimage.label(ref > 0, structure=np.ones((3, 3), bool))
    big = lab == np.bincount(lab.ravel())[1:].argmax() + 1
    ys, _ = np.nonzero(big)
    assert ys.min() == 0 and ys.max() == 374 and big.sum() > 30000     # one component from the top row to the bottom one


def serpentine(H, W, strong, band=8, gap=8, v=50, vs=110):
    """A band of gray v, 8 px wide, traced boustrophedon over the frame: its outline is one closed 1-px chain of weak
    candidates (magnitudes 152..210 < 300) across hundreds of tiles.  With `strong`, the free end of the last pass is
    brighter (vs): the only strong pixels of the frame lie there."""
    g = np.zeros((H, W), np.uint8)
    y, k = 8, 0
    while y + 2 * band + gap <= H - 8:
        g[y:y + band, 8:W - 8] = v
        x0 = W - 8 - band if k % 2 == 0 else 8
        g[y:y + 2 * band + gap, x0:x0 + band] = v
        y += band + gap
        k += 1
    g[y:y + band, 8:W - 8] = v
    if strong:
        x = 8 if (k - 1) % 2 == 0 else W - 8 - band
        g[y:y + band, x:x + band] = vs
    return np.repeat(g[..., None], 3, axis=2)


@pytest.mark.parametrize("size", [(436, 1024), (375, 1242)])
def test_serpentine_is_kept_or_dropped_whole(torch_, size):
    low, high = 60, 300
    img = serpentine(*size, strong=False)
    cand, strong = R.classes(R.blur(R.gray(img)), low, high)
    lab, n = ndimage.label(cand, structure=np.ones((3, 3), bool))
    ys, xs = np.nonzero(cand)
    assert n == 1 and not strong.any() and len(set(zip(ys // 16, xs // 64))) > 400
    assert not check(img, low, high).any()                            # no strong pixel: every pixel dropped
    img = serpentine(*size, strong=True)
    cand, strong = R.classes(R.blur(R.gray(img)), low, high)
    lab, _ = ndimage.label(cand, structure=np.ones((3, 3), bool))
    loop = lab == np.bincount(lab.ravel())[1:].argmax() + 1
    assert loop.sum() > 50000 and strong.any() and np.nonzero(strong)[0].min() > size[0] - 40
    e = check(img, low, high)
    assert np.array_equal(e[loop], np.full(loop.sum(), 255, np.uint8))  # one strong end: every pixel of the chain kept


def test_raw_abi_null_ivice_and_canaries(torch_, synth):
    torch = torch_
    L = pkg("_lib")
    lib = L.lib()
    H, W = 37, 101
    img = synth.make_pair(H, W, seed=2)[0]
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(img).to(dev)
    n = H * W
    edges = torch.full((n + 256,), 0x5A, dtype=torch.uint8, device=dev)
    sentinel = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    wsb = lib.dflow_canny_workspace_bytes(H, W)
    ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.dflow_canny_edges(H, W, bgr.data_ptr(), 100.0, 200.0, edges.data_ptr(), None, ws.data_ptr(), wsb, s),
            "dflow_canny_edges")
    torch.cuda.synchronize()
    ref = R.canny(img)
    assert np.array_equal(edges[:n].cpu().numpy().reshape(H, W), ref)
    assert (edges[n:] == 0x5A).all().item() and (ws[wsb:] == 0xA5).all().item()
    assert (sentinel == -7.0).all().item()
    # the same workspace again with the float plane: identical edges, the plane matches them exactly
    L.check(lib.dflow_canny_edges(H, W, bgr.data_ptr(), 100.0, 200.0, edges.data_ptr(), sentinel.data_ptr(), ws.data_ptr(),
                                  wsb, s), "dflow_canny_edges")
    torch.cuda.synchronize()
    assert np.array_equal(edges[:n].cpu().numpy().reshape(H, W), ref)
    assert sentinel.cpu().numpy().reshape(H, W).tobytes() == R.ivice(ref).tobytes()


def test_runs_on_a_side_stream_without_waiting(torch_, synth):
    torch = torch_
    img = synth.make_pair(436, 1024, seed=6)[0]
    dev = torch.device("cuda", 0)
    bgr = torch.from_numpy(img).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=dev)
        for _ in range(8):
            big = big @ big.T / 4096.0                      # keeps the side stream busy well past the host call
        e, iv = pkg("pipeline").canny_edges(bgr)
        pending = not side.query()
    side.synchronize()
    assert pending, "canny_edges waited for its stream"
    ref = R.canny(img)
    assert np.array_equal(e.cpu().numpy(), ref) and iv.cpu().numpy().tobytes() == R.ivice(ref).tobytes()


def test_edge_canny_ivice_writes_the_reference_file(torch_, synth, tmp_path):
    from PIL import Image
    img = synth.make_pair(375, 1242, seed=8)[0]
    png = os.path.join(tmp_path, "a.png")
    Image.fromarray(img[..., ::-1].copy()).save(png)                     # BGR -> RGB on disk
    out = os.path.join(tmp_path, "ivice.bin")
    pkg("edge").canny_ivice(png, out)
    data = open(out, "rb").read()
    assert len(data) == 375 * 1242 * 4 and data == R.ivice(R.canny(img)).tobytes()


def test_spremi_za_epic_without_the_binary(torch_, tmp_path, monkeypatch, capsys, synth):
    torch = torch_
    H, W = 60, 90
    rng = np.random.default_rng(12)
    fwd = rng.integers(-4, 5, (H, W, 2)).astype(np.float64)
    bwd = np.where(rng.random((H, W, 1)) < 0.7, -fwd, rng.integers(-4, 5, (H, W, 2))).astype(np.float64)
    img1 = synth.make_pair(H, W, seed=13)[0]
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img1[..., ::-1].copy()).save("a.png")
    Image.fromarray(img1[..., ::-1].copy()).save("b.png")
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    spz = pkg("spremiZaEpic")
    assert spz.main(["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny"]) == 0
    assert "absent" in capsys.readouterr().out
    dev = torch.device("cuda", 0)
    want = pkg("pipeline").fb_consistency(torch.from_numpy(fwd.astype(np.float32)).to(dev),
                                          torch.from_numpy(bwd.astype(np.float32)).to(dev), 3).cpu().numpy()
    got = np.load("sparse_field.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want) and 0 < want[..., 2].sum() < H * W
    pkg("evaluate").parovi(want, "want.txt")
    assert open("parovi.txt").read() == open("want.txt").read()
    assert open("ivice.bin", "rb").read() == R.ivice(R.canny(img1)).tobytes()
    assert spz.main(["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "sed"]) != 0
    assert "model.yml" in capsys.readouterr().err


def test_run_batch_edges(torch_, synth, tmp_path):
    H, W = 48, 64
    rb = pkg("run_batch")
    rb.main(["--pairs", "1", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--out", str(tmp_path), "--edges"])
    img1 = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))[0]
    data = open(os.path.join(tmp_path, "ivice_00.bin"), "rb").read()
    assert data == R.ivice(R.canny(img1)).tobytes()
    plain = os.path.join(tmp_path, "plain")
    rb.main(["--pairs", "1", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--out", plain])
    assert not any(f.startswith("ivice") for f in os.listdir(plain))
