"""dflow_track_advance, dflow_track_seed and dflow_track_flow on the GPU against tests/track_ref.py (the definitions in numpy
float32), through ctypes.  No step of the definitions depends on an order, so every comparison is bit for bit: float planes as
their uint32 words, states, slots, winners and counts equal.  Every plane the calls write, the scratch included, has its exact size
at its lowest alignment between guard bands (tests/ws_guard.py), poisoned where the call must write all of it.  pipeline.TrackSet and
tracks.py are followed through four frames with reseeding.  Run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import track_ref as R
from conftest import pkg
from ws_guard import GuardedWs

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x7F


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def coverage():
    return R.coverage_case()


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    got, want = words(got).reshape(-1), words(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s differs at %d of %d entries, first %d: got %r, expected %r" % (what, bad.size, got.size, bad[0], got[bad[0]],
                                                                                          want[bad[0]])


class Plane:
    """An array in a guarded device plane of its exact size, `offset` bytes after a 256-byte boundary; without data, poison."""

    def __init__(self, torch, like, offset, data=True):
        like = np.array(like, order="C")                # a writable copy
        self.torch, self.dtype, self.shape = torch, like.dtype, like.shape
        self.g = GuardedWs(torch, like.nbytes, POISON, torch.device("cuda", 0), offset)
        if data and like.nbytes:
            self.g.region.copy_(torch.from_numpy(like.view(np.uint8).reshape(-1)))
        self.ptr = self.g.ptr

    def get(self, what):
        self.g.assert_guards(what)
        return np.frombuffer(self.g.snapshot(), self.dtype).reshape(self.shape)


def upload(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def layout_of(L, flow):
    return L.EVAL_UVV if flow.shape[2] == 3 else L.EVAL_DYDX


def gpu_advance(torch, h, w, fwd, bwd, pos, state, rel=0.01, abs=0.5, err=True, counts=True, inplace=False):
    L = pkg("_lib")
    cap = len(state)
    d_fwd, d_bwd = upload(torch, fwd), upload(torch, bwd)
    pin, sin = Plane(torch, pos, 8), Plane(torch, state, 4)
    pout, sout = (pin, sin) if inplace else (Plane(torch, pos, 8, data=False), Plane(torch, state, 4, data=False))
    perr, pcnt = Plane(torch, np.zeros(cap, F), 4, data=False), Plane(torch, np.zeros(6, np.int32), 4, data=False)
    L.call("dflow_track_advance", h, w, d_fwd.data_ptr(), layout_of(L, fwd), d_bwd.data_ptr() if bwd is not None else None,
           layout_of(L, bwd) if bwd is not None else 0, cap, pin.ptr, sin.ptr, rel, abs, 0, pout.ptr, sout.ptr, perr.ptr if err else None,
           pcnt.ptr if counts else None, L.stream(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    out = [pout.get("pos_out"), sout.get("state_out"), perr.get("err"), pcnt.get("counts")]
    if not inplace:
        same(pin.get("pos_in"), pos, "the input positions")
        same(sin.get("state_in"), state, "the input states")
    if not err:
        assert (out[2].view(np.uint8) == POISON).all(), "d_err = NULL: nothing is written"
    if not counts:
        assert (out[3].view(np.uint8) == POISON).all()
    return out


def check_advance(torch, h, w, fwd, bwd, pos, state, what, **kw):
    want = R.advance(h, w, fwd, bwd, pos, state)
    got = gpu_advance(torch, h, w, fwd, bwd, pos, state, **kw)
    for name, g, e in zip(("pos", "state", "err", "counts"), got, want):
        if (name == "err" and not kw.get("err", True)) or (name == "counts" and not kw.get("counts", True)):
            continue
        same(g, e, "%s: %s" % (what, name))
    return want


@pytest.mark.parametrize("layout", ["uvv", "dydx"])
@pytest.mark.parametrize("back", [True, False])
def test_advance_coverage_case(torch_, coverage, layout, back):
    h, w, fwd, bwd, pos, state = coverage
    if layout == "dydx":
        fwd, bwd = R.to_dydx(fwd), R.to_dydx(bwd)
    bwd = bwd if back else None
    what = "37x53 %s %s" % (layout, "with bwd" if back else "without bwd")
    want = check_advance(torch_, h, w, fwd, bwd, pos, state, what)
    print(what, want[3].tolist())
    assert (want[3][[0, 1, 2, 5]] > 0).all() and ((want[3][3:5] > 0).all() if back else (want[3][3:5] == 0).all())
    for kw in (dict(err=False), dict(counts=False), dict(err=False, counts=False), dict(inplace=True), dict(inplace=True, err=False)):
        check_advance(torch_, h, w, fwd, bwd, pos, state, "%s %r" % (what, kw), **kw)
    # tails, and the wave's edge
    for cap in (1, 63, 64, 65, 1000):
        check_advance(torch_, h, w, fwd, bwd, pos[12:12 + cap], state[12:12 + cap], "%s cap %d" % (what, cap))
    # mixed layouts, and other tolerances
    if layout == "uvv" and back:
        check_advance(torch_, h, w, fwd, R.to_dydx(bwd), pos, state, "uvv forward, dydx backward")
        for rel, abs_ in ((0.0, 0.0), (0.5, 0.0), (0.0, 4.0)):
            want = R.advance(h, w, fwd, bwd, pos, state, rel, abs_)
            got = gpu_advance(torch_, h, w, fwd, bwd, pos, state, rel, abs_)
            for name, g, e in zip(("pos", "state", "err", "counts"), got, want):
                same(g, e, "rel %g abs %g: %s" % (rel, abs_, name))


def test_advance_follows_the_rotation_call_after_call(torch_):
    h = w = 65
    for angle in (0.05, -0.05):
        fwd, bwd = R.rotation_field(h, w, angle), R.rotation_field(h, w, -angle)
        pos = R.grid_seeds(h, w, 4)
        state = np.full(len(pos), R.LIVE, np.int32)
        gpos, gstate = pos, state
        for t in range(1, 9):
            pos, state, err, counts = R.advance(h, w, fwd, bwd, pos, state)
            gpos, gstate, gerr, gcounts = gpu_advance(torch_, h, w, fwd, bwd, gpos, gstate)
            for name, g, e in zip(("pos", "state", "err", "counts"), (gpos, gstate, gerr, gcounts), (pos, state, err, counts)):
                same(g, e, "rotation %+.2f frame %d: %s" % (angle, t, name))
        assert (state == R.LEFT).sum() == 32 and (state == R.LIVE).sum() == 256 - 32


def gpu_seed(torch, h, w, step, frame, mask, pos, state, birth, n, counts=True):
    L = pkg("_lib")
    cap = len(state)
    d_mask = upload(torch, mask)
    ppos, pstate, pbirth = Plane(torch, pos, 8), Plane(torch, state, 4), Plane(torch, birth, 4)
    pn = Plane(torch, np.array([n], np.int32), 4)
    pscan = Plane(torch, np.zeros(R.scan_len(h, w, step), np.int32), 4, data=False)
    pcnt = Plane(torch, np.zeros(4, np.int32), 4, data=False)
    L.call("dflow_track_seed", h, w, cap, step, frame, d_mask.data_ptr() if mask is not None else None, ppos.ptr, pstate.ptr, pbirth.ptr,
           pn.ptr, pscan.ptr, pcnt.ptr if counts else None, L.stream(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    pscan.get("scan")
    return ppos.get("pos"), pstate.get("state"), pbirth.get("birth"), int(pn.get("n")[0]), pcnt.get("counts")


def check_seed(torch, h, w, step, frame, mask, pos, state, birth, n, what):
    want = R.seed(h, w, step, frame, mask, pos, state, birth, n)
    got = gpu_seed(torch, h, w, step, frame, mask, pos, state, birth, n)
    for name, g, e in zip(("pos", "state", "birth", "n", "counts"), got, want):
        same(np.asarray(g), np.asarray(e, np.asarray(g).dtype), "%s: %s" % (what, name))
    return want


def some_tracks(rng, h, w, cap, n0):
    """A set of capacity cap whose first n0 slots hold tracks all over (and around) the frame, a fifth of them ended; the slots
    beyond hold what a caller's buffer may: anything."""
    pos = (rng.random((cap, 2)) * [w + 3, h + 3] - 2).astype(F)
    state = np.where(rng.random(cap) < 0.8, R.LIVE, rng.integers(2, 6, cap)).astype(np.int32)
    birth = rng.integers(0, 5, cap).astype(np.int32)
    if n0:
        pos[0] = np.nan
    return pos, state, birth


@pytest.mark.parametrize("h,w,step", [(37, 53, 1), (37, 53, 4), (37, 53, 64), (67, 131, 2), (1100, 1100, 1)])
def test_seed_matches_the_reference(torch_, h, w, step):
    rng = np.random.default_rng(h * 1000 + step)
    ncells = -(-h // step) * -(-w // step)
    what = "%dx%d step %d" % (h, w, step)
    # an empty set: every cell is seeded, in raster order
    cap = ncells + 5
    pos, state, birth = np.zeros((cap, 2), F), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    want = check_seed(torch_, h, w, step, 7, None, pos, state, birth, 0, what + " empty")
    assert want[3] == ncells and want[4].tolist() == [0, ncells, ncells, 0]
    # a set with tracks in it, with and without a mask; the cap is not reached
    n0 = min(ncells // 3 + 1, 4000)
    cap = n0 + ncells + 3
    pos, state, birth = some_tracks(rng, h, w, cap, n0)
    mask = (rng.random((h, w)) < 0.7).astype(np.uint8) * 200
    for m in (None, mask):
        want = check_seed(torch_, h, w, step, 3, m, pos, state, birth, n0, "%s with tracks%s" % (what, "" if m is None else " and a mask"))
        print(what, "mask" if m is not None else "no mask", want[4].tolist())
        assert want[4][3] == 0 and (ncells == 1 or 0 < want[4][1] < ncells)
    # the cap is reached in the middle: the rest is dropped
    seedable = int(want[4][1])
    if seedable > 1:
        cap = n0 + seedable // 2
        want = check_seed(torch_, h, w, step, 3, mask, pos[:cap], state[:cap], birth[:cap], n0, what + " cap reached")
        assert want[3] == cap and want[4][3] == seedable - seedable // 2
    # *d_n out of range is clamped; a full set takes nothing
    for n in (-3, cap, cap + 1000, 2 ** 31 - 1):
        check_seed(torch_, h, w, step, 3, mask, pos[:cap], state[:cap], birth[:cap], n, "%s n = %d" % (what, n))
    got = gpu_seed(torch_, h, w, step, 3, mask, pos[:cap], state[:cap], birth[:cap], n0, counts=False)
    assert (got[4].view(np.uint8) == POISON).all()


def test_a_second_seed_after_an_advance_fills_only_the_uncovered_cells(torch_, coverage):
    h, w, fwd, bwd, _, _ = coverage
    step, cap = 4, 400
    pos, state, birth = np.zeros((cap, 2), F), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    pos, state, birth, n, counts = check_seed(torch_, h, w, step, 0, None, pos, state, birth, 0, "first seed")
    assert n == 10 * 14
    pos, state, _, adv = check_advance(torch_, h, w, fwd, bwd, pos, state, "advance")
    assert adv[0] < n and adv[5] == cap - n
    pos2, state2, birth2, n2, counts2 = check_seed(torch_, h, w, step, 1, None, pos, state, birth, n, "second seed")
    assert counts2[0] + counts2[1] == 140 and 0 < counts2[1] < 140 and n2 == n + counts2[1] and counts2[3] == 0
    same(pos2[:n], pos[:n], "the tracks that were there")
    assert (birth2[n:n2] == 1).all() and (birth2[:n] == 0).all() and (state2[n:n2] == R.LIVE).all()


def gpu_flow(torch, h, w, pos_a, state_a, pos_b, state_b, counts=True):
    L = pkg("_lib")
    pa, sa, pb, sb = Plane(torch, pos_a, 8), Plane(torch, state_a, 4), Plane(torch, pos_b, 8), Plane(torch, state_b, 4)
    own = Plane(torch, np.zeros((h, w), np.int32), 4, data=False)
    out = Plane(torch, np.zeros((h, w, 3), F), 4, data=False)
    cnt = Plane(torch, np.zeros(3, np.int32), 4, data=False)
    L.call("dflow_track_flow", h, w, len(state_a), pa.ptr, sa.ptr, pb.ptr, sb.ptr, own.ptr, out.ptr, cnt.ptr if counts else None,
           L.stream(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    return own.get("owner"), out.get("out"), cnt.get("counts")


def test_flow_matches_the_reference_in_both_orders(torch_, coverage):
    h, w, fwd, bwd, pos, state = coverage
    pos_b, state_b, _, _ = R.advance(h, w, fwd, bwd, pos, state)
    # colliding tracks: every position once more, and a block of tracks on one pixel
    pos_a2 = np.concatenate([pos, pos[::-1], np.full((70, 2), 5.25, F)])
    state_a2 = np.concatenate([state, state[::-1], np.full(70, R.LIVE, np.int32)])
    pos_b2 = np.concatenate([pos_b, pos_b[::-1], np.full((70, 2), 7.5, F) + np.arange(70, dtype=F)[:, None]])
    state_b2 = np.concatenate([state_b, state_b[::-1], np.full(70, R.LIVE, np.int32)])
    for what, a, b in (("a -> b", (pos_a2, state_a2), (pos_b2, state_b2)), ("b -> a", (pos_b2, state_b2), (pos_a2, state_a2)),
                       ("a -> a", (pos_a2, state_a2), (pos_a2, state_a2)), ("one track", (pos[20:21], state[20:21]), (pos_b[20:21], state_b[20:21])),
                       ("63 tracks", (pos[:63], state[:63]), (pos_b[:63], state_b[:63]))):
        want = R.flow(h, w, a[0], a[1], b[0], b[1])
        got = gpu_flow(torch_, h, w, a[0], a[1], b[0], b[1])
        for name, g, e in zip(("owner", "out", "counts"), got, want):
            same(g, e, "%s: %s" % (what, name))
        print(what, want[2].tolist())
        assert want[2].sum() == len(a[1])
    want = R.flow(h, w, pos_a2, state_a2, pos_b2, state_b2)
    on55 = np.flatnonzero((state_a2 == R.LIVE) & (state_b2 == R.LIVE) & (np.rint(pos_a2) == 5).all(1))
    assert want[2][1] > 400 and want[2][2] > 100 and len(on55) >= 70 and want[0][5, 5] == on55[0], "the block on (5, 5): the smallest index wins"
    got = gpu_flow(torch_, h, w, pos_a2, state_a2, pos_b2, state_b2, counts=False)
    same(got[1], want[1], "without counts: out")
    assert (got[2].view(np.uint8) == POISON).all()
    # more tracks than pixels and more pixels than tracks: both roles of a lane
    hs, ws = 3, 5
    pa = (np.random.default_rng(1).random((300, 2)) * [ws - 1, hs - 1]).astype(F)
    st = np.full(300, R.LIVE, np.int32)
    for name, g, e in zip(("owner", "out", "counts"), gpu_flow(torch_, hs, ws, pa, st, pa + F(1), st), R.flow(hs, ws, pa, st, pa + F(1), st)):
        same(g, e, "3x5 with 300 tracks: %s" % name)


def reference_sequence(h, w, flows, step, cap, reseed):
    """What TrackSet does, through track_ref: (snapshots [(pos, state)], birth, n)."""
    pos, state, birth = np.zeros((cap, 2), F), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    pos, state, birth, n, _ = R.seed(h, w, step, 0, None, pos, state, birth, 0)
    snaps = [(pos, state)]
    for t, (f, b) in enumerate(flows, 1):
        snaps[-1] = (pos, state)
        pos, state, _, _ = R.advance(h, w, f, b, pos, state)
        if reseed:
            pos, state, birth, n, _ = R.seed(h, w, step, t, None, pos, state, birth, n)
        snaps.append((pos, state))
    return snaps, birth, n


def sequence_flows(coverage):
    h, w, fwd, bwd, _, _ = coverage
    f2, b2 = fwd.copy(), bwd.copy()
    f2[..., :2] *= F(0.5)
    b2[..., :2] *= F(0.5)
    return h, w, [(fwd, bwd), (f2, b2), (f2, None), (fwd, bwd)]


def test_trackset_four_frames_with_reseeding(torch_, coverage):
    P = pkg("pipeline")
    h, w, flows = sequence_flows(coverage)
    step, cap = 4, 330                              # 140 cells: the cap is reached on the way
    snaps, birth, n = reference_sequence(h, w, flows, step, cap, True)
    ts = P.TrackSet(h, w, cap=cap, step=step)
    assert ts.counts() == {"seed": None, "advance": None}
    ts.seed()
    for f, b in flows:
        ts.advance(f, b).seed()
    assert ts.frame == 4 and len(ts.snapshots) == 5
    got = ts.read()
    assert n == cap and got["pos"].shape == (5, n, 2) and got["state"].shape == (5, n) and got["birth"].shape == (n,) and got["length"].shape == (n,)
    assert got["pos"].dtype == F and got["state"].dtype == np.int32 and got["length"].dtype == np.int32
    same(got["birth"], birth[:n], "birth")
    assert len(np.unique(got["birth"])) == 5, "tracks were started at every frame"
    for t, (pos, state) in enumerate(snaps):
        same(got["state"][t], state[:n], "frame %d: state" % t)
        born = birth[:n] <= t
        same(got["pos"][t][born], pos[:n][born], "frame %d: pos" % t)
        assert np.isnan(got["pos"][t][~born]).all() and (got["state"][t][~born] == R.FREE).all()
    same(got["length"], (got["state"] == R.LIVE).sum(0).astype(np.int32), "length")
    ended = np.flatnonzero((got["state"][2] >= 2) & (birth[:n] <= 2))
    assert ended.size and (got["pos"][3:, ended] == got["pos"][2, ended]).all(), "the last position is repeated after a track's end"
    c = ts.counts()
    assert c["seed"].is_cuda and c["seed"].cpu().tolist()[3] > 0, "the last seed dropped cells: the set is full"
    assert c["advance"].cpu().sum() == cap
    for a, b in ((0, 4), (4, 0), (1, 3), (2, 2)):
        flow, owner, cnt = ts.flow(a, b, owner=True, counts=True)
        want = R.flow(h, w, snaps[a][0], snaps[a][1], snaps[b][0], snaps[b][1])
        for name, g, e in zip(("owner", "out", "counts"), (owner, flow, cnt), want):
            same(g.cpu().numpy(), e, "flow %d -> %d: %s" % (a, b, name))
        assert want[2][0] > 0
    for bad in (-1, 5, 1.0):
        with pytest.raises(ValueError, match="TrackSet.flow"):
            ts.flow(0, bad)
    # the wrappers on host arrays, one call each
    pos, state = snaps[0]
    out = P.track_advance(h, w, pos, state, flows[0][0], flows[0][1], err=True, counts=True)
    for name, g, e in zip(("pos", "state", "err", "counts"), out, R.advance(h, w, flows[0][0], flows[0][1], pos, state)):
        same(g.cpu().numpy(), e, "track_advance on host arrays: %s" % name)
    out = P.track_seed(h, w, snaps[1][0], snaps[1][1], np.zeros(cap, np.int32), 140, step=step, frame=9, counts=True)
    want = R.seed(h, w, step, 9, None, snaps[1][0], snaps[1][1], np.zeros(cap, np.int32), 140)
    for name, g, e in zip(("pos", "state", "birth", "n", "counts"), out, want):
        same(g.cpu().numpy(), np.asarray(e, g.cpu().numpy().dtype), "track_seed on host arrays: %s" % name)


def test_the_three_calls_captured_into_a_graph_on_a_side_stream(torch_, coverage):
    """The calls allocate nothing, read nothing back and wait for nothing: seed, advance and flow captured one after the other run
    only when the graph is replayed, and every replay on a cleared set gives the reference's bytes."""
    torch, L = torch_, pkg("_lib")
    h, w, fwd, bwd, _, _ = coverage
    step, cap = 4, 300
    dev = torch.device("cuda", 0)
    d_fwd, d_bwd = torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pos, state, birth, n = torch.zeros((cap, 2), device=dev), torch.zeros(cap, **i32), torch.zeros(cap, **i32), torch.zeros(1, **i32)
    scan = torch.empty(R.scan_len(h, w, step), **i32)
    pos1, state1 = torch.full((cap, 2), 7.0, device=dev), torch.full((cap,), -7, **i32)
    owner, out = torch.empty((h, w), **i32), torch.full((h, w, 3), 7.0, device=dev)
    cnts = [torch.full((k,), -7, **i32) for k in (4, 6, 3)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st = L.stream(dev)
        L.call("dflow_track_seed", h, w, cap, step, 0, None, pos.data_ptr(), state.data_ptr(), birth.data_ptr(), n.data_ptr(), scan.data_ptr(),
               cnts[0].data_ptr(), st)
        L.call("dflow_track_advance", h, w, d_fwd.data_ptr(), L.EVAL_UVV, d_bwd.data_ptr(), L.EVAL_UVV, cap, pos.data_ptr(), state.data_ptr(),
               0.01, 0.5, 0, pos1.data_ptr(), state1.data_ptr(), None, cnts[1].data_ptr(), st)
        L.call("dflow_track_flow", h, w, cap, pos.data_ptr(), state.data_ptr(), pos1.data_ptr(), state1.data_ptr(), owner.data_ptr(),
               out.data_ptr(), cnts[2].data_ptr(), st)
    torch.cuda.synchronize()
    assert all((c == -7).all().item() for c in cnts) and (n == 0).all().item(), "a captured call must not run before the graph is replayed"
    z = np.zeros(cap, np.int32)
    p0, s0, b0, n0, c0 = R.seed(h, w, step, 0, None, np.zeros((cap, 2), F), z, z, 0)
    p1, s1, _, c1 = R.advance(h, w, fwd, bwd, p0, s0)
    own, flow, c2 = R.flow(h, w, p0, s0, p1, s1)
    for _ in range(2):
        for t in (pos, state, birth, n):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, g, e in (("pos", pos, p0), ("state", state, s0), ("birth", birth, b0), ("n", n, np.array([n0], np.int32)), ("pos1", pos1, p1),
                           ("state1", state1, s1), ("owner", owner, own), ("flow", out, flow), ("seed counts", cnts[0], c0),
                           ("advance counts", cnts[1], c1), ("flow counts", cnts[2], c2)):
            same(g.cpu().numpy(), e, "replayed: %s" % name)


def test_tracks_cli_end_to_end(torch_, tmp_path, monkeypatch, capsys):
    flowio, cli = pkg("flowio"), pkg("tracks")
    h, w = 45, 61
    monkeypatch.chdir(tmp_path)
    flows = []
    for t, angle in enumerate((0.04, 0.05, 0.06)):
        f, b = R.rotation_field(h, w, angle), R.rotation_field(h, w, -angle)
        if t == 1:
            b[10:30, 20:40, 0] += F(3)              # a patch that fails the check
        flowio.write_flo("f%d.flo" % t, f[..., [1, 0]])
        np.save("b%d.npy" % t, b)
        flows.append((np.ascontiguousarray(f[..., [1, 0]]), b))
    argv = ["f0.flo", "f1.flo", "f2.flo", "--backward", "b0.npy", "b1.npy", "b2.npy", "--step", "3", "--reseed", "--cap", "500", "--out",
            "t.npz", "--flow", "0", "3", "f03.flo", "--json"]
    assert cli.main(argv) == 0
    summary = json.loads(capsys.readouterr().out)
    snaps, birth, n = reference_sequence(h, w, flows, 3, 500, True)
    got = np.load("t.npz")
    assert sorted(got.files) == ["birth", "length", "pos", "state"] and got["pos"].shape == (4, n, 2)
    same(got["birth"], birth[:n], "birth")
    for t, (pos, state) in enumerate(snaps):
        same(got["state"][t], state[:n], "frame %d: state" % t)
        born = birth[:n] <= t
        same(got["pos"][t][born], pos[:n][born], "frame %d: pos" % t)
    last = snaps[-1][1][:n]
    assert summary["frames"] == 4 and summary["tracks"] == n and summary["live"] == (last == R.LIVE).sum()
    assert summary["inconsistent"] == (last == R.INCONSISTENT).sum() > 0 and summary["left"] == (last == R.LEFT).sum() > 0
    want = R.flow(h, w, snaps[0][0], snaps[0][1], snaps[3][0], snaps[3][1])
    same(flowio.read_flo("f03.flo"), want[1][..., :2], "--flow 0 3")
    assert summary["flow_vectors"] == want[2][0] > 0
    # the text form, without the options
    assert cli.main(["f0.flo", "--out", "u.npz"]) == 0
    assert "2 frames, 192 tracks (0 cells dropped): " in capsys.readouterr().out and np.load("u.npz")["pos"].shape == (2, 192, 2)
