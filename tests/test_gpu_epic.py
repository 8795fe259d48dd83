"""dflow_epic_interpolate (csrc/epic.hip) against the numpy restatement epic_ref.py: the Voronoi diagram S, D and the
neighbour lists byte for byte, the flow within 1e-3 px; and the drop-ins built on it: epicflow.py, spremiZaEpic.py
--gpu-epic and run_batch --epic.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import canny_ref as CR
import epic_ref as R
from conftest import GOLDEN_NAMES, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def gpu(sparse, edges, nn=100, k=0.8, method="LA", lists=True):
    flow, S, D, lst, lg = pkg("pipeline").epic_interpolate(sparse, edges, nn, k, method, aux=True, lists=lists)
    out = [flow.cpu().numpy(), S.cpu().numpy(), D.cpu().numpy().view(np.uint32)]
    return out + ([lst.cpu().numpy(), lg.cpu().numpy()] if lists else [None, None])


def random_field(H, W, frac, seed, edge_style="random"):
    rng = np.random.default_rng(seed)
    sp = np.zeros((H, W, 3), np.float32)
    m = rng.random((H, W)) < frac
    sp[..., 0] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 1] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 2] = m
    e = rng.random((H, W)).astype(np.float32) if edge_style == "random" else (rng.random((H, W)) < 0.1).astype(np.float32)
    return sp, e


def check_exact(sparse, edges, nn=100, k=0.8):
    """S, D and the lists byte-equal to the reference; the flow of both methods within 1e-3 px (seeds whose lambda_min is
    within 1 % of TAU excluded)."""
    H, W = sparse.shape[:2]
    for method in ("LA", "NW"):
        ref = R.interpolate(sparse, edges, nn, k, method)
        flow, S, D, lst, lg = gpu(sparse, edges, nn, k, method)
        assert np.array_equal(S, ref["S"]), "S differs at %s" % np.argwhere(S != ref["S"])[:5].tolist()
        assert np.array_equal(D.astype(np.int64), ref["D"]), "D differs at %s" % np.argwhere(D != ref["D"])[:5].tolist()
        want = np.full((H * W, nn), -1, np.int64)
        want_g = np.full((H * W, nn), -1, np.int64)
        for s, l in ref["lists"].items():
            want[s, :len(l)] = [t for t, _ in l]
            want_g[s, :len(l)] = [g for _, g in l]
        bad = np.argwhere((lst != want).any(axis=1))
        assert bad.size == 0, "lists differ for seeds %s" % bad[:5].ravel().tolist()
        assert np.array_equal(lg, want_g)
        near = [s for s, v in ref["lmin"].items() if v is not None and abs(v - R.TAU) <= 0.01 * R.TAU]
        ok = ~np.isin(ref["S"], near)
        err = np.abs(flow - ref["flow"])[ok]
        assert err.size == 0 or err.max() < 1e-3, (method, err.max())
    return ref


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_fixtures(torch_, golden, name):
    z = golden(name)
    edges = CR.ivice(CR.canny(z["img1"]))                  # ivice.bin as the reference writes it
    check_exact(z["sparse_t3"], edges)


@pytest.mark.parametrize("size", [(1, 1), (1, 70), (70, 1), (33, 65)])
def test_small_sizes(torch_, size):
    sp, e = random_field(*size, 0.3, seed=size[0] * 100 + size[1])
    if not sp[..., 2].any():
        sp[0, 0] = (1.5, -0.5, 1.0)
    check_exact(sp, e, nn=16)


@pytest.mark.parametrize("case", ["none", "one", "two", "all", "1%", "30%"])
def test_seed_sets(torch_, case):
    H, W = 40, 60
    frac = {"none": 0.0, "all": 1.0, "1%": 0.01, "30%": 0.3}.get(case, 0.0)
    sp, e = random_field(H, W, frac, seed=3, edge_style="sparse")
    if case in ("one", "two"):
        sp[7, 11] = (2.0, -1.0, 1.0)
    if case == "two":
        sp[30, 50] = (-3.0, 0.5, 1.0)
    ref = check_exact(sp, e, nn=24)
    if case == "none":
        flow = gpu(sp, e)[0]
        assert not flow.any() and (ref["S"] == -1).all()


def synthetic_dense(H, W, seed):
    """About 94 % of the pixels seeded (the share of the golden fixture c45x35) and a Canny ivice map of a synthetic frame."""
    synth = pkg("synth")
    img = synth.make_pair(H, W, seed=seed)[0]
    sp, _ = random_field(H, W, 0.94, seed)
    return sp, CR.ivice(CR.canny(img))


@pytest.mark.parametrize("size", [(436, 1024), (375, 1242)])
def test_fixed_point_at_bench_sizes(torch_, size):
    sp, e = synthetic_dense(*size, seed=21)
    flow, S, D, _, _ = gpu(sp, e, lists=False)
    assert R.verify_fixed_point(sp, e, S, D) is None
    sub = np.zeros_like(sp)
    sub[::4, ::4] = sp[::4, ::4]                           # the 1-in-16 grid subsample
    flow, S, D, _, _ = gpu(sub, e, lists=False)
    assert R.verify_fixed_point(sub, e, S, D) is None


def test_fixed_point_4k_single_corner_seed(torch_):
    H, W = 2160, 3840
    rng = np.random.default_rng(5)
    e = (rng.random((H, W)) < 0.05).astype(np.float32)
    sp = np.zeros((H, W, 3), np.float32)
    sp[H - 1, W - 1] = (1.0, 2.0, 1.0)
    flow, S, D, _, _ = gpu(sp, e, lists=False)
    assert R.verify_fixed_point(sp, e, S, D) is None
    assert (S == H * W - 1).all() and D[0, 0] >= 2 * (H + W - 2)
    assert np.array_equal(flow[..., 0], np.full((H, W), 2.0, np.float32))     # one seed: its flow everywhere
    sp[0, 0] = (-1.0, 0.0, 1.0)
    flow, S, D, _, _ = gpu(sp, e, lists=False)
    assert R.verify_fixed_point(sp, e, S, D) is None


def test_comb_of_walls_winds_across_tiles(torch_):
    """Walls of e = 1, 6 px thick, every 16 columns, open alternately at the top and the bottom: from the one seed in the
    top-left corner the cheap path runs down and up every channel (crossing a wall costs 6 * 2002, a detour at most
    2 * 2 * 436), through hundreds of tiles."""
    H, W = 436, 1024
    e = np.zeros((H, W), np.float32)
    for i, x in enumerate(range(10, W - 6, 16)):
        e[:, x:x + 6] = 1.0
        if i % 2 == 0:
            e[H - 8:, x:x + 6] = 0.0
        else:
            e[:8, x:x + 6] = 0.0
    sp = np.zeros((H, W, 3), np.float32)
    sp[0, 0] = (0.5, 0.25, 1.0)
    flow, S, D, _, _ = gpu(sp, e, lists=False)
    assert R.verify_fixed_point(sp, e, S, D) is None
    rounds, ms = pkg("pipeline").epic_last_stats()
    walls = len(range(10, W - 6, 16))
    assert D[0, W - 1] > walls * (H - 16) * 2 and D[0, W - 1] < 6 * 2002 * walls     # wound, not crossed
    assert rounds > 1 and set(ms) == {"voronoi", "graph", "lists", "fill"}


def test_lists_of_sampled_seeds_at_bench_size(torch_):
    H, W = 436, 1024
    sp, e = synthetic_dense(H, W, seed=33)
    for method in ("LA", "NW"):
        flow, S, D, lst, lg = gpu(sp, e, method=method)
        if method == "LA":
            assert R.verify_fixed_point(sp, e, S, D) is None
            graph = R.seed_graph(S, D.astype(np.int64), e)
        seeds = np.flatnonzero(R.seed_mask(sp).ravel())
        for s in np.random.default_rng(4).choice(seeds, 64, replace=False).tolist():
            ref = R.neighbour_list(graph, s, 100)
            assert lst[s, :len(ref)].tolist() == [t for t, _ in ref] and (lst[s, len(ref):] == -1).all()
            assert lg[s, :len(ref)].tolist() == [g for _, g in ref]
            model, lmin = R.fit(sp, s, ref, 0.8, method)
            if lmin is not None and abs(lmin - R.TAU) <= 0.01 * R.TAU:
                continue
            ys, xs = np.nonzero(S == s)
            want_u = model[0] + model[1] * (xs - s % W) + model[2] * (ys - s // W)
            want_v = model[3] + model[4] * (xs - s % W) + model[5] * (ys - s // W)
            assert np.abs(flow[ys, xs, 1] - want_u).max() < 1e-3 and np.abs(flow[ys, xs, 0] - want_v).max() < 1e-3


def test_edge_separates_two_motions(torch_):
    """A 1-px band of e = 1 divides two regions with different motions.  Crossing it costs more than 2000 while the nn-th
    neighbour on the same side is a few units away, so every list stays on its side: NW gives each pixel its own side's
    flow, LA its own side's affine field.  Euclidean NW, blind to the band, mixes the sides."""
    H, W, band, nn = 40, 64, 32, 20
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    left = xs < band
    A = (3.0 + 0.25 * xs - 0.125 * ys, -1.0 + 0.5 * ys)
    B = (-2.0 - 0.5 * xs + 0.25 * ys, 4.0 + 0.125 * xs)
    sp = np.zeros((H, W, 3), np.float32)
    for which, (fu, fv) in ((left, A), (xs > band, B)):
        sp[which, 0], sp[which, 1], sp[which, 2] = fu[which], fv[which], 1.0
    e = np.zeros((H, W), np.float32)
    e[:, band] = 1.0
    const = sp.copy()
    const[left, 0], const[left, 1] = 3.0, -1.0
    const[xs > band, 0], const[xs > band, 1] = -2.0, 4.0
    flow, S, _, lst, _ = gpu(const, e, nn=nn, method="NW")
    side = (S % W) < band
    rows = lst[R.seed_mask(const).ravel()]
    assert all(((r[r >= 0] % W) < band).all() or ((r[r >= 0] % W) > band).all() for r in rows)
    assert np.array_equal(flow[..., 1], np.where(side, 3.0, -2.0).astype(np.float32))
    assert np.array_equal(flow[..., 0], np.where(side, -1.0, 4.0).astype(np.float32))
    flow, S, _, _, _ = gpu(sp, e, nn=nn, method="LA")
    side = (S % W) < band
    assert np.abs(flow[..., 1] - np.where(side, A[0], B[0])).max() < 1e-3
    assert np.abs(flow[..., 0] - np.where(side, A[1], B[1])).max() < 1e-3
    # Euclidean NW at the pixels next to the band takes neighbours from both sides
    seeds = np.flatnonzero(R.seed_mask(const).ravel())
    sy, sx = np.divmod(seeds, W)
    worst = 0.0
    for y in range(0, H, 5):
        d = np.hypot(sy - y, sx - (band - 1))
        near = np.argsort(d, kind="stable")[:nn]
        w = np.exp(-0.8 * d[near])
        worst = max(worst, abs((w * const.reshape(-1, 3)[seeds[near], 0]).sum() / w.sum() - 3.0))
    assert worst > 0.5


def test_side_stream_matches_default(torch_):
    torch = torch_
    sp, e = synthetic_dense(120, 200, seed=8)
    want = gpu(sp, e)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn(2048, 2048, device=dev)
        for _ in range(4):
            big = big @ big.T / 2048.0                     # work queued ahead on the side stream
        got = gpu(torch.from_numpy(sp).to(dev), torch.from_numpy(e).to(dev))
    side.synchronize()
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()


def _png(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)


def test_epicflow_cli_on_a_golden_fixture(torch_, golden, tmp_path):
    z = golden("c45x35_c9x7")
    H, W = z["img1"].shape[:2]
    _png(os.path.join(tmp_path, "a.png"), z["img1"])
    _png(os.path.join(tmp_path, "b.png"), z["img2"])
    with open(os.path.join(tmp_path, "m.txt"), "wb") as f:
        f.write(z["parovi_t3_txt"].tobytes())
    edges = CR.ivice(CR.canny(z["img1"]))
    edges.tofile(os.path.join(tmp_path, "e.bin"))
    # the matches parsed here, independently: x1 y1 x2 y2 -> seed (rint x1, rint y1) with flow (x2 - x1, y2 - y1)
    sp = np.zeros((H, W, 3), np.float32)
    for line in z["parovi_t3_txt"].tobytes().decode().splitlines():
        x1, y1, x2, y2 = (float(v) for v in line.split())
        sp[int(np.rint(y1)), int(np.rint(x1))] = (np.float32(x2 - x1), np.float32(y2 - y1), 1.0)
    ef, flowio = pkg("epicflow"), pkg("flowio")
    for extra, method, nn, k in (([], "LA", 100, 0.8), (["-nw", "-nn", "12", "-k", "2.5"], "NW", 12, 2.5)):
        out = os.path.join(tmp_path, "o.flo")
        assert ef.main([os.path.join(tmp_path, n) for n in ("a.png", "b.png", "e.bin", "m.txt", "o.flo")] + extra) == 0
        want = pkg("pipeline").epic_interpolate(sp, edges, nn, k, method).cpu().numpy()
        assert flowio.read_flo(out).tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    with open(os.path.join(tmp_path, "short.bin"), "wb") as f:
        f.write(b"\0" * 12)
    assert ef.main([os.path.join(tmp_path, n) for n in ("a.png", "b.png", "short.bin", "m.txt", "o.flo")]) == 2


def test_spremi_za_epic_gpu_epic(torch_, synth, tmp_path, monkeypatch, capsys):
    H, W = 60, 90
    rng = np.random.default_rng(12)
    fwd = rng.integers(-4, 5, (H, W, 2)).astype(np.float64)
    bwd = np.where(rng.random((H, W, 1)) < 0.7, -fwd, rng.integers(-4, 5, (H, W, 2))).astype(np.float64)
    img1 = synth.make_pair(H, W, seed=13)[0]
    monkeypatch.chdir(tmp_path)
    _png("a.png", img1)
    _png("b.png", img1)
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    spz = pkg("spremiZaEpic")
    assert spz.main(["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny", "--gpu-epic"]) == 0
    assert "epic.flo" in capsys.readouterr().out
    sparse = np.load("sparse_field.npy")
    edges = np.fromfile("ivice.bin", np.float32).reshape(H, W)
    assert edges.tobytes() == CR.ivice(CR.canny(img1)).tobytes()
    got = pkg("flowio").read_flo("epic.flo")
    want = pkg("pipeline").epic_interpolate(sparse, edges).cpu().numpy()
    assert got.shape == (H, W, 2) and got.tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    assert spz.main(["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny", "--other"]) == 2


def test_run_batch_epic(torch_, synth, tmp_path):
    H, W = 48, 64
    rb = pkg("run_batch")
    rb.main(["--pairs", "1", "--bcd-times", "1", "--size", "%dx%d" % (H, W), "--out", str(tmp_path), "--epic"])
    sparse = np.load(os.path.join(tmp_path, "sparse_field_00.npy"))
    img1 = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))[0]
    want = pkg("pipeline").epic_interpolate(sparse, CR.ivice(CR.canny(img1))).cpu().numpy()
    got = pkg("flowio").read_flo(os.path.join(tmp_path, "epic_00.flo"))
    assert got.tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()
    assert not os.path.exists(os.path.join(tmp_path, "ivice_00.bin"))
