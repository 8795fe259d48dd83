"""dflow_klt_pyramid, dflow_corners and dflow_klt_track on the GPU against tests/klt_ref.py (the definitions of
include/dflow_klt.h in numpy), through ctypes.  No step of the definitions depends on an order, so every comparison is bit for
bit: float planes as their uint32 words; pyramid, mask, states and counts equal.  Every plane the calls write, the scratch
included, has its exact size at its lowest alignment between guard bands (tests/ws_guard.py), poisoned where the call must write
all of it.  The shapes are the smallest at which each path can go wrong: 1x1, 3x70 (one row of tiles, a tail of the four-pixel
groups), 33x65 with 2 levels (odd sizes, more than one tile), 96x128 with 4 levels (the top level, 12x16, is smaller than the
17x17 window).  pipeline.TrackSet and klt.py are followed through three frames with reseeding.  Run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import klt_ref as R
from conftest import pkg
from ws_guard import GuardedWs

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x7F
KLT = dict(r=7, iters=20, eps=0.01, min_eig=1.0, max_err=0.0, fb=0.5)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    got, want = words(got).reshape(-1), words(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s differs at %d of %d entries, first %d: got %r, expected %r" % (what, bad.size, got.size, bad[0], got[bad[0]],
                                                                                          want[bad[0]])


class Plane:
    """An array in a guarded device plane of its exact size, `offset` bytes after a 256-byte boundary; without data, poison."""

    def __init__(self, torch, like, offset, data=True):
        like = np.array(like, order="C")
        self.dtype, self.shape = like.dtype, like.shape
        self.g = GuardedWs(torch, like.nbytes, POISON, torch.device("cuda", 0), offset)
        if data and like.nbytes:
            self.g.region.copy_(torch.from_numpy(like.view(np.uint8).reshape(-1)))
        self.ptr = self.g.ptr

    def get(self, what):
        self.g.assert_guards(what)
        return np.frombuffer(self.g.snapshot(), self.dtype).reshape(self.shape)


def stream(torch):
    return pkg("_lib").stream(torch.device("cuda", 0))


# ---------------------------------------------------------------- the cases, made once
def pair(synth, h, w, seed):
    """Two images of one texture, the second moved by about a pixel and a half."""
    if min(h, w) < 8:
        rng = np.random.default_rng(seed)
        big = rng.integers(0, 256, (h + 2, w + 2, 3), dtype=np.uint8)
        return np.ascontiguousarray(big[:h, :w]), np.ascontiguousarray(big[:h, 1:w + 1] if w > 1 else big[:h, :w] // 2)
    img1, img2, _ = synth.make_pair(h, w, seed, amp_x=2.5, amp_y=1.5)
    return img1, img2


SHAPES = {"1x1": (1, 1, 1, 11), "3x70": (3, 70, 3, 12), "33x65": (33, 65, 2, 13), "96x128": (96, 128, 4, 14)}      # h, w, levels, seed


@pytest.fixture(scope="module")
def cases(synth):
    """name -> dict(h, w, levels, img1, img2, pyr1, pyr2): the reference pyramids, computed once and left unchanged."""
    out = {}
    for name, (h, w, levels, seed) in SHAPES.items():
        img1, img2 = pair(synth, h, w, seed)
        out[name] = dict(h=h, w=w, levels=levels, img1=img1, img2=img2, pyr1=R.pyramid(img1, levels), pyr2=R.pyramid(img2, levels))
    return out


def some_tracks(rng, h, w, cap, corners):
    """A set of capacity cap: positions all over and around the frame, on its border, on whole pixels, at corners, a NaN; three
    quarters live, the others in every other state."""
    pos = (rng.random((cap, 2)) * [w + 2, h + 2] - 1).astype(F)
    pos[::5] = np.rint(pos[::5])
    k = min(len(corners), cap // 3)
    if k:
        pos[1:1 + 3 * k:3] = corners[rng.permutation(len(corners))[:k]] + rng.random((k, 2)).astype(F) * F(0.5)
    edge = np.array([[0, 0], [w - 1, h - 1], [0, h / 2], [w - 1, h / 3], [w / 2, 0], [w / 3, h - 1], [w - 1, 0], [-0.0, h - 1]], F)
    if cap >= 17:
        at = np.arange(2, cap, 3)[:len(edge)]
        pos[at] = edge[:len(at)]
        pos[6] = (np.nan, 1)
        pos[9] = (3, np.inf)
    state = np.where(rng.random(cap) < 0.75, R.LIVE, rng.integers(0, 8, cap)).astype(np.int32)
    if cap == 1:
        pos[0], state[0] = (corners[0] if len(corners) else (0, 0)), R.LIVE
    return np.ascontiguousarray(pos), state


# ---------------------------------------------------------------- the calls
def gpu_pyramid(torch, img, levels):
    L = pkg("_lib")
    h, w, _ = img.shape
    total = R.level_offsets(h, w, levels)[1]
    assert L.lib().dflow_klt_pyramid_bytes(h, w, levels) == total
    bgr, pyr = Plane(torch, img, 4), Plane(torch, np.zeros(total, np.uint8), 4, data=False)
    L.call("dflow_klt_pyramid", h, w, levels, bgr.ptr, pyr.ptr, stream(torch))
    torch.cuda.synchronize()
    same(bgr.get("d_bgr"), img, "the picture")
    return pyr.get("d_pyr")


def gpu_corners(torch, Y, rc=2, min_dist=4, border=4, quality=0.01, min_response=0.0, tracks=None, counts=True):
    L = pkg("_lib")
    h, w = Y.shape
    grey = Plane(torch, Y, 1)
    resp, mask = Plane(torch, np.zeros((h, w), F), 4, data=False), Plane(torch, np.zeros((h, w), np.uint8), 1, data=False)
    rmax, cnt = Plane(torch, np.zeros(1, np.uint32), 4, data=False), Plane(torch, np.zeros(4, np.int32), 4, data=False)
    set_args, occ = (0, None, None, None), None
    if tracks is not None:
        pos, state, n = tracks
        ppos, pstate, pn = Plane(torch, pos, 8), Plane(torch, state, 4), Plane(torch, np.array([n], np.int32), 4)
        occ = Plane(torch, np.zeros((h, w), np.uint8), 1, data=False)
        set_args = (len(state), ppos.ptr, pstate.ptr, pn.ptr)
    L.call("dflow_corners", h, w, grey.ptr, rc, min_dist, border, quality, min_response, *set_args, resp.ptr, mask.ptr,
           occ.ptr if occ else None, rmax.ptr, cnt.ptr if counts else None, stream(torch))
    torch.cuda.synchronize()
    if tracks is not None:
        same(ppos.get("d_pos"), tracks[0], "the set's positions")
        same(pstate.get("d_state"), tracks[1], "the set's states")
        same(occ.get("d_occ"), R.occupation(h, w, *tracks), "d_occ")
    same(grey.get("d_pyr"), Y, "level 0")
    return resp.get("d_response"), mask.get("d_mask"), cnt.get("d_counts"), rmax.get("d_rmax").view(F)[0]


def check_corners(torch, Y, what, **kw):
    want = R.corners(Y, **kw)
    got = gpu_corners(torch, Y, **kw)
    for name, g, e in zip(("response", "mask", "counts", "rmax"), got, want):
        same(np.asarray(g), np.asarray(e), "%s: %s" % (what, name))
    return want


def gpu_track(torch, c, pos, state, inplace=False, err=True, back=True, counts=True, **kw):
    L = pkg("_lib")
    a = dict(KLT, **kw)
    cap = len(state)
    p1, p2 = Plane(torch, R.pack(c["pyr1"]), 1), Plane(torch, R.pack(c["pyr2"]), 1)
    pin, sin = Plane(torch, pos, 8), Plane(torch, state, 4)
    pout, sout = (pin, sin) if inplace else (Plane(torch, pos, 8, data=False), Plane(torch, state, 4, data=False))
    perr, pback = Plane(torch, np.zeros(cap, F), 4, data=False), Plane(torch, np.zeros((cap, 2), F), 8, data=False)
    pcnt = Plane(torch, np.zeros(8, np.int32), 4, data=False)
    L.call("dflow_klt_track", c["h"], c["w"], c["levels"], p1.ptr, p2.ptr, cap, pin.ptr, sin.ptr, a["r"], a["iters"], a["eps"], a["min_eig"],
           a["max_err"], a["fb"], 0, pout.ptr, sout.ptr, perr.ptr if err else None, pback.ptr if back else None, pcnt.ptr if counts else None,
           stream(torch))
    torch.cuda.synchronize()
    out = [pout.get("pos_out"), sout.get("state_out"), perr.get("err"), pback.get("back"), pcnt.get("counts")]
    p1.get("d_pyr1"), p2.get("d_pyr2")
    if not inplace:
        same(pin.get("pos_in"), pos, "the input positions")
        same(sin.get("state_in"), state, "the input states")
    for given, plane in ((err, out[2]), (back, out[3]), (counts, out[4])):
        assert given or (plane.view(np.uint8) == POISON).all(), "an output that is NULL: nothing is written"
    return out


def check_track(torch, c, pos, state, what, want=None, **kw):
    a = dict(KLT, **{k: v for k, v in kw.items() if k in KLT})
    want = want or R.track(c["pyr1"], c["pyr2"], pos, state, **a)
    got = gpu_track(torch, c, pos, state, **kw)
    for name, g, e in zip(("pos", "state", "err", "back", "counts"), got, want):
        if kw.get({"err": "err", "back": "back", "counts": "counts"}.get(name, ""), True):
            same(g, e, "%s: %s" % (what, name))
    return want


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pyramid_is_the_reference(torch_, cases, name):
    c = cases[name]
    for img, pyr in ((c["img1"], c["pyr1"]), (c["img2"], c["pyr2"])):
        same(gpu_pyramid(torch_, img, c["levels"]), R.pack(pyr), "%s pyramid" % name)
    for levels in {1, 8} - {c["levels"]}:
        same(gpu_pyramid(torch_, c["img1"], levels), R.pack(R.pyramid(c["img1"], levels)), "%s with %d levels" % (name, levels))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_corners_are_the_reference(torch_, cases, name):
    c = cases[name]
    Y, h, w = c["pyr1"][0], c["h"], c["w"]
    border = min(4, (min(h, w) - 1) // 2)
    want = check_corners(torch_, Y, name, border=border)
    print(name, "corners", want[2].tolist())
    for kw in (dict(quality=0.0, border=0), dict(quality=1.0, border=0), dict(rc=1, min_dist=1, border=0), dict(rc=7, min_dist=9, border=1),
               dict(min_response=float(want[3]) * 0.5, border=0), dict(border=max(h, w)), dict(min_dist=32, quality=0.0, border=0)):
        check_corners(torch_, Y, "%s %r" % (name, kw), **kw)
    got = gpu_corners(torch_, Y, border=border, counts=False)
    same(got[1], want[1], "%s without counts: mask" % name)
    assert (got[2].view(np.uint8) == POISON).all()
    if name in ("33x65", "96x128"):
        assert want[2][3] > 3
        # with a set: live tracks near every other corner, ended ones and ones beyond n near the others
        pos = R.corner_positions(want[1])
        n = len(pos)
        rng = np.random.default_rng(n)
        tp = np.concatenate([pos + (rng.random((n, 2)).astype(F) * F(4) - F(2)), (rng.random((40, 2)) * [w + 4, h + 4] - 2).astype(F)])
        tp[-1] = np.nan
        ts = np.concatenate([np.where(np.arange(n) % 2 == 0, R.LIVE, R.LEFT), np.full(40, R.LIVE)]).astype(np.int32)
        for m in (n + 20, n + 40, n + 1000, 0, -5):
            check_corners(torch_, Y, "%s with a set, n = %d" % (name, m), border=border, tracks=(tp, ts, m))
        assert check_corners(torch_, Y, name + " with a set", border=border, tracks=(tp, ts, n + 20))[2][2] >= n // 2


def test_corners_twice_give_the_same_bytes_and_a_flat_image_none(torch_, cases):
    Y = cases["96x128"]["pyr1"][0]
    a, b = gpu_corners(torch_, Y), gpu_corners(torch_, Y)
    for name, g, e in zip(("response", "mask", "counts"), a, b):
        same(g, e, "the second call: %s" % name)
    flat = np.full((33, 65), 77, np.uint8)
    want = check_corners(torch_, flat, "a constant image", quality=0.0, border=0)
    assert want[2].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("cap", [1, 17, 300])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_track_is_the_reference(torch_, cases, name, cap):
    c = cases[name]
    rng = np.random.default_rng(cap * 1000 + c["h"])
    corners = R.corner_positions(R.corners(c["pyr1"][0], border=min(4, (min(c["h"], c["w"]) - 1) // 2))[1])
    pos, state = some_tracks(rng, c["h"], c["w"], cap, corners)
    what = "%s cap %d" % (name, cap)
    want = check_track(torch_, c, pos, state, what, min_eig=0.05)
    print(what, want[4].tolist())
    assert want[4][:6].sum() == cap
    if cap == 300 and name in ("33x65", "96x128"):
        assert want[4][0] > 10 and want[4][1] > 10 and want[4][5] > 30 and want[4][6] > 10


@pytest.mark.parametrize("r", [1, 7, 10])
def test_track_window_radii_and_options(torch_, cases, r):
    c = cases["96x128"]
    rng = np.random.default_rng(r)
    corners = R.corner_positions(R.corners(c["pyr1"][0])[1])
    pos, state = some_tracks(rng, c["h"], c["w"], 150, corners)
    what = "96x128 r %d" % r
    want = check_track(torch_, c, pos, state, what, r=r, min_eig=0.05)
    print(what, want[4].tolist())
    assert want[4][0] > 5
    # two calls give the same bytes
    a, b = (gpu_track(torch_, c, pos, state, r=r, min_eig=0.05) for _ in range(2))
    for name, g, e in zip(("pos", "state", "err", "back", "counts"), a, b):
        same(g, e, "%s, the second call: %s" % (what, name))
    if r == 7:
        for kw in (dict(fb=0.0), dict(max_err=1.5), dict(max_err=0.25, fb=0.0), dict(iters=1), dict(iters=64, eps=1e-4), dict(eps=2.0),
                   dict(min_eig=40.0), dict(min_eig=0.0), dict(fb=0.02), dict(inplace=True), dict(inplace=True, err=False, back=False),
                   dict(err=False), dict(back=False), dict(counts=False), dict(err=False, back=False, counts=False)):
            got = check_track(torch_, c, pos, state, "%s %r" % (what, kw), **kw)
            if "max_err" in kw:
                assert got[4][3] > 0, "some tracks fail the residual test"
            if kw.get("min_eig") == 40.0:
                assert got[4][2] > 0, "some windows are flat"
            if kw.get("fb") == 0.02:
                assert got[4][4] > 0, "some tracks fail the backward test"
            if kw.get("fb") == 0.0:
                assert got[4][4] == 0 and np.isnan(got[3]).all()


def test_a_constant_image_is_flat(torch_):
    img = np.full((33, 65, 3), 120, np.uint8)
    pyr = R.pyramid(img, 2)
    c = dict(h=33, w=65, levels=2, pyr1=pyr, pyr2=pyr)
    pos = (np.random.default_rng(3).random((17, 2)) * [64, 32]).astype(F)
    want = check_track(torch_, c, pos, np.full(17, R.LIVE, np.int32), "a constant image")
    assert want[4].tolist() == [0, 0, 17, 0, 0, 0, 0, 0]


def reference_sequence(imgs, levels, cap, corner_args, klt_args):
    """What TrackSet does with seed_corners and advance_klt after every frame: (snapshots [(pos, state)], birth, n)."""
    h, w = imgs[0].shape[:2]
    pyrs = [R.pyramid(img, levels) for img in imgs]
    pos, state, birth, n = np.zeros((cap, 2), F), np.zeros(cap, np.int32), np.zeros(cap, np.int32), 0
    snaps = []
    for t, pyr in enumerate(pyrs):
        if t:
            pos, state = R.track(pyrs[t - 1], pyr, pos, state, **klt_args)[:2]
        new = R.corner_positions(R.corners(pyr[0], tracks=(pos, state, n), **corner_args)[1])[:cap - n]
        pos, state, birth = pos.copy(), state.copy(), birth.copy()
        pos[n:n + len(new)], state[n:n + len(new)], birth[n:n + len(new)] = new, R.LIVE, t
        n += len(new)
        snaps.append((pos, state))
    return snaps, birth, n


@pytest.fixture(scope="module")
def sequence(synth):
    img0, img1, _ = synth.make_pair(64, 96, 21, amp_x=3, amp_y=2)
    imgs = [img0, img1, np.ascontiguousarray(np.roll(img1, (1, -2), (0, 1)))]
    corner_args, klt_args = dict(min_dist=5, quality=0.02), dict(KLT, r=5, min_eig=0.05)
    return imgs, corner_args, klt_args, reference_sequence(imgs, 3, 400, corner_args, klt_args)


def test_trackset_three_frames_with_reseeding(torch_, sequence):
    P = pkg("pipeline")
    imgs, corner_args, klt_args, (snaps, birth, n) = sequence
    h, w = imgs[0].shape[:2]
    ts = P.TrackSet(h, w, cap=400, step=1)
    pyrs = [P.klt_pyramid(img, 3) for img in imgs]
    ts.seed_corners(pyrs[0], **corner_args)
    for a, b in zip(pyrs, pyrs[1:]):
        ts.advance_klt(a, b, **klt_args).seed_corners(b, **corner_args)
    assert ts.frame == 2 and len(ts.snapshots) == 3
    got = ts.read()
    assert got["pos"].shape == (3, n, 2) and 0 < n < 400
    same(got["birth"], birth[:n], "birth")
    assert len(np.unique(got["birth"])) == 3, "tracks were started at every frame"
    for t, (pos, state) in enumerate(snaps):
        same(got["state"][t], state[:n], "frame %d: state" % t)
        born = birth[:n] <= t
        same(got["pos"][t][born], pos[:n][born], "frame %d: pos" % t)
    c = ts.counts()
    assert c["advance"].cpu()[:6].sum() == 400 and c["corners"].cpu()[2] > 0 and c["seed"].cpu()[3] == 0
    for a, b in ((0, 2), (1, 2)):
        same(ts.flow(a, b).cpu().numpy(), R.sparse_flow(h, w, snaps[a][0], snaps[a][1], snaps[b][0], snaps[b][1]), "flow %d -> %d" % (a, b))
    # the wrappers on host arrays, one call each
    p0 = R.pyramid(imgs[0], 3)
    same(P.klt_pyramid(imgs[0], 3).cpu().numpy(), R.pack(p0), "klt_pyramid")
    mask, resp, cnt = P.corners(R.pack(p0), h, w, response=True, counts=True, **corner_args)
    for name, g, e in zip(("response", "mask", "counts"), (resp, mask, cnt), R.corners(p0[0], **corner_args)):
        same(g.cpu().numpy(), e, "corners on host arrays: %s" % name)
    out = P.klt_track(R.pack(p0), R.pack(R.pyramid(imgs[1], 3)), h, w, 3, snaps[0][0], snaps[0][1], err=True, counts=True, **klt_args)
    want = R.track(p0, R.pyramid(imgs[1], 3), snaps[0][0], snaps[0][1], **klt_args)
    for name, g, e in zip(("pos", "state", "err", "counts"), out, (want[0], want[1], want[2], want[4])):
        same(g.cpu().numpy(), e, "klt_track on host arrays: %s" % name)


def test_sparse_flow_into_epic(torch_, sequence):
    P = pkg("pipeline")
    imgs, corner_args, klt_args, (snaps, _, _) = sequence
    h, w = imgs[0].shape[:2]
    sparse = P.klt_sparse_flow(imgs[0], imgs[1], levels=3, cap=400, corner_args=corner_args, **klt_args)
    pyr0, pyr1 = R.pyramid(imgs[0], 3), R.pyramid(imgs[1], 3)
    pos = R.corner_positions(R.corners(pyr0[0], **corner_args)[1])
    st = np.full(len(pos), R.LIVE, np.int32)
    po, so = R.track(pyr0, pyr1, pos, st, **klt_args)[:2]
    same(sparse.cpu().numpy(), R.sparse_flow(h, w, pos, st, po, so), "klt_sparse_flow")
    dense = P.epic_interpolate(sparse, P.pb_edges(imgs[0])).cpu().numpy()
    assert dense.shape == (h, w, 2) and np.isfinite(dense).all() and int((sparse[..., 2] > 0.5).sum().cpu()) > 20


def test_the_chain_captured_into_a_graph_on_a_side_stream(torch_, cases):
    """The calls allocate nothing, read nothing back and wait for nothing: pyramids, corners, seed and track captured one after
    the other run only when the graph is replayed, and every replay on a cleared set gives the reference's bytes."""
    torch, L = torch_, pkg("_lib")
    c = cases["96x128"]
    h, w, levels, cap = c["h"], c["w"], c["levels"], 300
    dev = torch.device("cuda", 0)
    total = R.level_offsets(h, w, levels)[1]
    img1, img2 = torch.from_numpy(c["img1"]).to(dev), torch.from_numpy(c["img2"]).to(dev)
    u8, i32 = dict(dtype=torch.uint8, device=dev), dict(dtype=torch.int32, device=dev)
    pyr1, pyr2 = torch.zeros(total, **u8), torch.zeros(total, **u8)
    resp, mask, rmax = torch.full((h, w), 7.0, device=dev), torch.full((h, w), 7, **u8), torch.zeros(1, **i32)
    pos, state, birth, n = torch.zeros((cap, 2), device=dev), torch.zeros(cap, **i32), torch.zeros(cap, **i32), torch.zeros(1, **i32)
    scan = torch.empty(h * w + -(-h * w // 1024) + 1, **i32)
    pos1, state1, err = torch.full((cap, 2), 7.0, device=dev), torch.full((cap,), -7, **i32), torch.full((cap,), 7.0, device=dev)
    cnts = [torch.full((k,), -7, **i32) for k in (4, 4, 8)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    a = dict(KLT, min_eig=0.05)
    with torch.cuda.graph(graph, stream=side):
        st = L.stream(dev)
        L.call("dflow_klt_pyramid", h, w, levels, img1.data_ptr(), pyr1.data_ptr(), st)
        L.call("dflow_klt_pyramid", h, w, levels, img2.data_ptr(), pyr2.data_ptr(), st)
        L.call("dflow_corners", h, w, pyr1.data_ptr(), 2, 4, 4, 0.01, 0.0, 0, None, None, None, resp.data_ptr(), mask.data_ptr(), None,
               rmax.data_ptr(), cnts[0].data_ptr(), st)
        L.call("dflow_track_seed", h, w, cap, 1, 0, mask.data_ptr(), pos.data_ptr(), state.data_ptr(), birth.data_ptr(), n.data_ptr(),
               scan.data_ptr(), cnts[1].data_ptr(), st)
        L.call("dflow_klt_track", h, w, levels, pyr1.data_ptr(), pyr2.data_ptr(), cap, pos.data_ptr(), state.data_ptr(), a["r"], a["iters"],
               a["eps"], a["min_eig"], a["max_err"], a["fb"], 0, pos1.data_ptr(), state1.data_ptr(), err.data_ptr(), None, cnts[2].data_ptr(), st)
    torch.cuda.synchronize()
    assert all((t == -7).all().item() for t in cnts) and (n == 0).all().item(), "a captured call must not run before the graph is replayed"
    R_, m_, c_, _ = R.corners(c["pyr1"][0])
    found = R.corner_positions(m_)
    k = len(found)
    assert 10 < k < cap
    p0, s0 = np.zeros((cap, 2), F), np.zeros(cap, np.int32)
    p0[:k], s0[:k] = found, R.LIVE
    p1, s1, e1, _, c1 = R.track(c["pyr1"], c["pyr2"], p0, s0, **a)
    for _ in range(2):
        for t in (pos, state, birth, n):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, g, e in (("pyr1", pyr1, R.pack(c["pyr1"])), ("pyr2", pyr2, R.pack(c["pyr2"])), ("response", resp, R_), ("mask", mask, m_),
                           ("corner counts", cnts[0], c_), ("pos", pos, p0), ("state", state, s0), ("n", n, np.array([k], np.int32)),
                           ("pos1", pos1, p1), ("state1", state1, s1), ("err", err, e1), ("track counts", cnts[2], c1)):
            same(g.cpu().numpy(), e, "replayed: %s" % name)


def test_klt_cli_end_to_end(torch_, sequence, tmp_path, monkeypatch, capsys):
    flowio, cli = pkg("flowio"), pkg("klt")
    imgs, _, _, _ = sequence
    h, w = imgs[0].shape[:2]
    monkeypatch.chdir(tmp_path)
    for t, img in enumerate(imgs):
        np.save("i%d.npy" % t, img)
    argv = ["i0.npy", "i1.npy", "i2.npy", "--out", "t.npz", "--radius", "5", "--min-dist", "5", "--quality", "0.02", "--reseed", "--cap", "400",
            "--flow", "0", "2", "f02.flo", "--epic", "e01.flo", "--json"]
    assert cli.main(argv) == 0
    summary = json.loads(capsys.readouterr().out)
    snaps, birth, n = reference_sequence(imgs, 3, 400, dict(min_dist=5, quality=0.02), dict(KLT, r=5))
    got = np.load("t.npz")
    assert sorted(got.files) == ["birth", "length", "pos", "state"] and got["pos"].shape == (3, n, 2)
    same(got["birth"], birth[:n], "birth")
    for t, (pos, state) in enumerate(snaps):
        same(got["state"][t], state[:n], "frame %d: state" % t)
        born = birth[:n] <= t
        same(got["pos"][t][born], pos[:n][born], "frame %d: pos" % t)
    last = snaps[-1][1][:n]
    assert summary["frames"] == 3 and summary["tracks"] == n and summary["live"] == (last == R.LIVE).sum() > 10
    assert summary["flat"] == (last == R.FLAT).sum() and summary["inconsistent"] == (last == R.INCONSISTENT).sum()
    want = R.sparse_flow(h, w, snaps[0][0], snaps[0][1], snaps[2][0], snaps[2][1])
    same(flowio.read_flo("f02.flo"), want[..., :2], "--flow 0 2")
    assert summary["flow_vectors"] == int(want[..., 2].sum()) > 0
    dense = flowio.read_flo("e01.flo")
    assert dense.shape == (h, w, 2) and np.isfinite(dense).all()
