"""dflow_bcd_stats / dflow_bcd_stats_batch and the stop rule of ceoBCD on the GPU, against tests/bcd_stats_ref.py (the
definition in numpy) and the golden labels.  Every entry point is called through _lib.  Run with `pytest -m gpu`.

What is asserted: the integer fields are equal; data_sum lies within (n - 1) * 2**-53 * sum|x| of math.fsum over the n float32
costs summed, the first-order bound of a recursive or pairwise double summation in ANY order (Higham, Accuracy and Stability
of Numerical Algorithms, section 4.2: |error| <= (n - 1) u sum|x_i| + O(u^2), u = 2**-53), derived and not measured; two calls
and the batch give identical bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

from bcd_stats_ref import INT_FIELDS, bcd_stats_ref
from conftest import GOLDEN_NAMES, pkg

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


class State:
    """A random labelling problem on the device: proposals, lcosts, nprop, labels as the C-ABI lays them out, and the same
    arrays in the reference's form."""

    def __init__(self, torch, H, W, seed, tpsi=8, tphi=2.5, maxnprop=150, label_pitch=160):
        L = pkg("_lib")
        self.torch, self.H, self.W = torch, H, W
        self.dev = torch.device("cuda", 0)
        self.p = L.default_params(H, W, 1, 1, tpsi=tpsi, tphi=tphi, maxnprop=maxnprop, label_pitch=label_pitch)
        rng = np.random.default_rng(seed)
        LP = label_pitch
        # flows in -4..4: L1 differences 0..16 straddle tpsi = 8 (and 1); costs in [0, 3) straddle tphi, a tenth exactly tphi
        self.flows = rng.integers(-4, 5, (H, W, LP, 2)).astype(np.int64)
        self.costs = (rng.random((H, W, LP)) * 3).astype(np.float32)
        self.costs[rng.random((H, W, LP)) < 0.1] = np.float32(tphi)
        self.nprop = rng.integers(1, maxnprop + 1, (H, W)).astype(np.int64)
        self.labels = self.random_labels(rng)
        packed = (self.flows[..., 0].astype(np.int16).view(np.uint16).astype(np.uint32)
                  | (self.flows[..., 1].astype(np.int16).view(np.uint16).astype(np.uint32) << 16))
        self.d_prop = torch.from_numpy(packed.view(np.int32)).to(self.dev)
        self.d_cost = torch.from_numpy(self.costs).to(self.dev)
        self.d_nprop = torch.from_numpy(self.nprop.astype(np.int32)).to(self.dev)
        self.d_labels = self.upload(self.labels)
        self.wsb = int(L.lib().dflow_bcd_stats_workspace_bytes(C.byref(self.p)))
        assert 0 < self.wsb <= 32768
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)

    def random_labels(self, rng):
        return (rng.random((self.H, self.W)) * self.nprop).astype(np.int64)

    def upload(self, labels):
        return self.torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(self.dev)

    def ref(self, labels=None, prev=None):
        return bcd_stats_ref(self.flows, self.costs, self.nprop, self.labels if labels is None else labels, self.p.tpsi,
                             self.p.tphi, prev=prev)

    def call(self, d_labels=None, d_prev=None, d_prev_out=None):
        """One dflow_bcd_stats through _lib; returns the 48 bytes."""
        L = pkg("_lib")
        out = self.torch.full((6,), SENTINEL, dtype=self.torch.int64, device=self.dev)
        L.call("dflow_bcd_stats", C.byref(self.p), self.d_prop.data_ptr(), self.d_cost.data_ptr(), self.d_nprop.data_ptr(),
               (self.d_labels if d_labels is None else d_labels).data_ptr(), d_prev.data_ptr() if d_prev is not None else None,
               d_prev_out.data_ptr() if d_prev_out is not None else None, out.data_ptr(), self.ws.data_ptr(), self.wsb,
               L.stream(self.dev))
        return out.cpu().numpy().tobytes()


def check(raw, ref, what=""):
    """The 48 bytes of a call against the reference's dict: prints, then asserts."""
    got = dict(zip(INT_FIELDS + ("data_sum",), struct.unpack("<5Qd", raw)))
    n = ref["n_data"]
    bound = max(n - 1, 0) * 2.0 ** -53 * ref["sum_abs"]
    print("%s got %s | ref data_sum %.17g, |diff| %.3g, bound %.3g (n = %d)"
          % (what, got, ref["data_sum"], abs(got["data_sum"] - ref["data_sum"]), bound, n))
    for k in INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert abs(got["data_sum"] - ref["data_sum"]) <= bound, (what, got["data_sum"], ref["data_sum"], bound)
    return got


# 1x1, 1x70, 70x1: no pairs in one or both directions; 33x65, 65x129: partial tiles in both axes, several blocks per axis
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (65, 129)]


@pytest.mark.parametrize("tpsi", (1, 8))
@pytest.mark.parametrize("shape", SHAPES)
def test_random_fields_match_the_reference(torch_, shape, tpsi):
    """Every shape and tpsi: without an earlier labelling, against the labelling itself (n_changed 0), against one that
    differs at known pixels, with d_prev_out aliasing d_prev_labels, and two calls byte for byte."""
    H, W = shape
    s = State(torch_, H, W, seed=100 * H + W + tpsi, tpsi=tpsi, maxnprop=40 if H * W > 4000 else 150)
    ref = s.ref()
    raw = s.call()
    got = check(raw, ref, "%dx%d tpsi %d, no prev:" % (H, W, tpsi))
    assert got["n_changed"] == 0 and got["n_bad_label"] == 0
    if H == 1 and W == 1:
        assert got["smooth_sum"] == 0 and got["n_pairs_trunc"] == 0
    assert s.call() == raw, "two calls must give identical bytes"
    # against itself
    assert check(s.call(d_prev=s.d_labels), s.ref(prev=s.labels), "prev = labels:")["n_changed"] == 0
    # an earlier labelling that differs at known pixels: the corners and every 7th pixel
    prev = s.labels.copy()
    flat = prev.reshape(-1)
    idx = np.unique(np.concatenate([[0, flat.size - 1], np.arange(0, flat.size, 7)]))
    flat[idx] = (flat[idx] + 1) % 200
    d_prev = s.upload(prev)
    got = check(s.call(d_prev=d_prev), s.ref(prev=prev), "prev differs at %d pixels:" % idx.size)
    assert got["n_changed"] == idx.size
    assert np.array_equal(d_prev.cpu().numpy(), prev), "d_prev_labels is read only when d_prev_out is another buffer"
    # d_prev_out = d_prev_labels: the same statistics, and the buffer then holds the labels
    out = torch_.full((H, W), SENTINEL, dtype=torch_.int32, device=s.dev)
    assert s.call(d_prev=d_prev, d_prev_out=out) == s.call(d_prev=d_prev)
    assert np.array_equal(out.cpu().numpy(), s.labels)
    raw_alias = s.call(d_prev=d_prev, d_prev_out=d_prev)
    assert raw_alias == s.call(d_prev=s.upload(prev))
    assert np.array_equal(d_prev.cpu().numpy(), s.labels)
    assert check(s.call(d_prev=d_prev, d_prev_out=d_prev), s.ref(prev=s.labels), "second aliased call:")["n_changed"] == 0


def test_labels_out_of_range_at_three_pixels(torch_):
    H, W = 33, 65
    s = State(torch_, H, W, seed=9)
    lab = s.labels.copy()
    lab[0, 0] = -1                                   # a tile corner
    lab[7, 31] = s.nprop[7, 31]                      # the last pixel of the first tile: its pairs cross into two other tiles
    lab[32, 64] = 1000                               # the last pixel of the frame, beyond label_pitch
    ref = s.ref(labels=lab, prev=lab)
    got = check(s.call(d_labels=s.upload(lab), d_prev=s.upload(lab)), ref, "three bad labels:")
    assert got["n_bad_label"] == 3 and got["n_changed"] == 3
    clean = s.ref()
    assert ref["smooth_sum"] < clean["smooth_sum"] and ref["n_data"] == H * W - 3
    assert check(s.call(d_labels=s.upload(lab)), s.ref(labels=lab), "three bad labels, no prev:")["n_changed"] == 0


def test_batch_of_three_equals_three_single_calls(torch_):
    """Three passes of one geometry with different proposals and labels; the second without an earlier labelling."""
    torch = torch_
    L = pkg("_lib")
    H, W = 65, 129
    states = [State(torch, H, W, seed=40 + k, maxnprop=40) for k in range(3)]
    rng = np.random.default_rng(5)
    prevs = [s.random_labels(rng) for s in states]
    single, d_prevs = [], []
    for k, s in enumerate(states):
        dp = None if k == 1 else s.upload(prevs[k])
        single.append(s.call(d_prev=dp, d_prev_out=dp))
        check(single[-1], s.ref(prev=None if k == 1 else prevs[k]), "pass %d:" % k)
        d_prevs.append(None if k == 1 else s.upload(prevs[k]))
    dev = states[0].dev
    out = torch.full((3, 6), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(3 * states[0].wsb, dtype=torch.uint8, device=dev)

    def arr(get):
        return (C.c_void_p * 3)(*[get(s) for s in states])
    pv = (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in d_prevs])
    L.call("dflow_bcd_stats_batch", C.byref(states[0].p), 3, arr(lambda s: s.d_prop.data_ptr()), arr(lambda s: s.d_cost.data_ptr()),
           arr(lambda s: s.d_nprop.data_ptr()), arr(lambda s: s.d_labels.data_ptr()), pv, out.data_ptr(), ws.data_ptr(),
           3 * states[0].wsb, L.stream(dev))
    raw = out.cpu().numpy().tobytes()
    for k in range(3):
        assert raw[48 * k:48 * (k + 1)] == single[k], "pass %d of the batch differs from the single call" % k
    for k in (0, 2):
        assert np.array_equal(d_prevs[k].cpu().numpy(), states[k].labels), "d_prev[%d] must hold the labels afterwards" % k
    # the whole d_prev array may be NULL
    L.call("dflow_bcd_stats_batch", C.byref(states[0].p), 3, arr(lambda s: s.d_prop.data_ptr()), arr(lambda s: s.d_cost.data_ptr()),
           arr(lambda s: s.d_nprop.data_ptr()), arr(lambda s: s.d_labels.data_ptr()), None, out.data_ptr(), ws.data_ptr(),
           3 * states[0].wsb, L.stream(dev))
    raw = out.cpu().numpy().tobytes()
    for k, s in enumerate(states):
        assert raw[48 * k:48 * (k + 1)] == s.call()


def test_batch_of_nine_goes_through_two_pairs_of_launches(torch_):
    """More passes than one launch's arguments carry (8): the ninth goes into a second pair of launches.  Nine labellings of
    one small problem, every one against its own earlier labelling, byte for byte what nine single calls write."""
    torch = torch_
    L = pkg("_lib")
    s = State(torch, 33, 65, seed=77, maxnprop=40)
    rng = np.random.default_rng(6)
    labs = [s.random_labels(rng) for _ in range(9)]
    prevs = [s.random_labels(rng) for _ in range(9)]
    single = [s.call(d_labels=s.upload(labs[k]), d_prev=s.upload(prevs[k])) for k in range(9)]
    assert len(set(single)) == 9
    check(single[8], s.ref(labels=labs[8], prev=prevs[8]), "pass 8:")
    d_labs, d_prevs = [s.upload(a) for a in labs], [s.upload(a) for a in prevs]
    out = torch.full((9, 6), SENTINEL, dtype=torch.int64, device=s.dev)
    ws = torch.empty(9 * s.wsb, dtype=torch.uint8, device=s.dev)
    same = lambda t: (C.c_void_p * 9)(*[t.data_ptr()] * 9)                # noqa: E731
    each = lambda ts: (C.c_void_p * 9)(*[t.data_ptr() for t in ts])       # noqa: E731
    L.call("dflow_bcd_stats_batch", C.byref(s.p), 9, same(s.d_prop), same(s.d_cost), same(s.d_nprop), each(d_labs), each(d_prevs),
           out.data_ptr(), ws.data_ptr(), 9 * s.wsb, L.stream(s.dev))
    raw = out.cpu().numpy().tobytes()
    for k in range(9):
        assert raw[48 * k:48 * (k + 1)] == single[k], "pass %d of the batch differs from the single call" % k
        assert np.array_equal(d_prevs[k].cpu().numpy(), labs[k]), k


def test_captured_into_a_graph(torch_):
    torch = torch_
    L = pkg("_lib")
    s = State(torch, 33, 65, seed=3)
    rng = np.random.default_rng(8)
    prev = s.random_labels(rng)
    direct = s.call(d_prev=s.upload(prev))
    d_prev = s.upload(prev)
    kept = torch.full((33, 65), SENTINEL, dtype=torch.int32, device=s.dev)
    out = torch.full((6,), SENTINEL, dtype=torch.int64, device=s.dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=s.dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        L.call("dflow_bcd_stats", C.byref(s.p), s.d_prop.data_ptr(), s.d_cost.data_ptr(), s.d_nprop.data_ptr(), s.d_labels.data_ptr(),
               d_prev.data_ptr(), kept.data_ptr(), out.data_ptr(), s.ws.data_ptr(), s.wsb, L.stream(s.dev))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and (kept == SENTINEL).all().item(), "a captured call must not run before the replay"
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == direct
        assert np.array_equal(kept.cpu().numpy(), s.labels)
        out.fill_(SENTINEL)
        torch.cuda.synchronize()


def test_argument_gate_launches_nothing(torch_):
    """Every DFLOW_EINVAL / DFLOW_ENOSPC case of include/dflow.h: the code, and the outputs untouched afterwards."""
    torch = torch_
    L = pkg("_lib")
    lib = L.lib()
    s = State(torch, 33, 65, seed=1)
    out = torch.full((8,), SENTINEL, dtype=torch.int64, device=s.dev)
    kept = torch.full((33, 65), SENTINEL, dtype=torch.int32, device=s.dev)
    ok = [C.byref(s.p), s.d_prop.data_ptr(), s.d_cost.data_ptr(), s.d_nprop.data_ptr(), s.d_labels.data_ptr(), None,
          kept.data_ptr(), out.data_ptr(), s.ws.data_ptr(), s.wsb, L.stream(s.dev)]

    def single(code, **change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        assert lib.dflow_bcd_stats(*a) == code, (change, lib.dflow_last_error())

    EINVAL, ENOSPC = -1, -2
    for field, bad in (("pich", 0), ("picw", 8193), ("tpsi", 0), ("tpsi", 9), ("label_pitch", 150), ("label_pitch", 176),
                       ("maxnprop", 0), ("maxnprop", 161), ("tphi", float("nan")), ("tphi", -1.0)):
        q = L.default_params(33, 65, 1, 1)
        setattr(q, field, bad)
        single(EINVAL, a0=C.byref(q))
        assert lib.dflow_bcd_stats_workspace_bytes(C.byref(q)) == 0
    single(EINVAL, a0=None)
    for k in (1, 2, 3, 4, 7):                                        # proposals, lcosts, nprop, bestlabels, stats
        single(EINVAL, **{"a%d" % k: None})
        assert b"NULL" in lib.dflow_last_error()
    single(EINVAL, a7=out.data_ptr() + 4)
    assert b"aligned" in lib.dflow_last_error()
    single(EINVAL, a8=s.ws.data_ptr() + 4, a9=s.wsb)
    assert b"d_ws" in lib.dflow_last_error()
    single(ENOSPC, a8=None)
    single(ENOSPC, a9=s.wsb - 1)
    assert b"workspace" in lib.dflow_last_error()

    arr = lambda v: (C.c_void_p * 2)(v, v)                           # noqa: E731
    okb = [C.byref(s.p), 2, arr(s.d_prop.data_ptr()), arr(s.d_cost.data_ptr()), arr(s.d_nprop.data_ptr()),
           arr(s.d_labels.data_ptr()), arr(kept.data_ptr()), out.data_ptr(), s.ws.data_ptr(), 2 * s.wsb, L.stream(s.dev)]

    def batch(code, **change):
        a = list(okb)
        for k, v in change.items():
            a[int(k[1:])] = v
        assert lib.dflow_bcd_stats_batch(*a) == code, (change, lib.dflow_last_error())

    batch(EINVAL, a0=None)
    for n in (0, -1):
        batch(EINVAL, a1=n)
        assert b"npass" in lib.dflow_last_error()
    for k in (2, 3, 4, 5):
        batch(EINVAL, **{"a%d" % k: None})
        batch(EINVAL, **{"a%d" % k: (C.c_void_p * 2)(s.d_prop.data_ptr(), None)})
        assert b"NULL" in lib.dflow_last_error()
    batch(EINVAL, a7=None)
    batch(EINVAL, a7=out.data_ptr() + 4)
    batch(EINVAL, a1=1025)
    assert b"npass" in lib.dflow_last_error()
    batch(EINVAL, a8=s.ws.data_ptr() + 4)
    batch(ENOSPC, a8=None)
    batch(ENOSPC, a9=2 * s.wsb - 1)                                  # room for one pass, not for two
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and (kept == SENTINEL).all().item(), "a refused call must not launch"


# ---------------------------------------------------------------- the golden fixtures, and ceoBCD's stop rule on them

@pytest.fixture(scope="module")
def passes(torch_, golden):
    """name, backward -> a DiscreteFlow of the fixture after generisi and nasumicni (the state BCD starts from), made once;
    the tests below restore the WTA labels before they sweep."""
    made = {}

    def get(name, backward=0):
        if (name, backward) not in made:
            g = golden(name)
            df = pkg("pipeline").DiscreteFlow(int(g["H"]), int(g["W"]), int(g["cellh"]), int(g["cellw"]), seed=int(g["seed"]))
            a, b = (g["img1"], g["img2"]) if backward == 0 else (g["img2"], g["img1"])
            df.load_pair(a, b)
            df.generisi()
            df.nasumicni()
            st = df.host_state()
            made[(name, backward)] = (df, g, st, df.bestlabels.clone())
        df, g, st, wta = made[(name, backward)]
        df.bestlabels.copy_(wta)
        return df, g, st
    return get


def golden_labels(g, backward, w):
    return g["b%d_labels%02d" % (backward, w)].astype(np.int64)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_geometries_after_0_and_2_sweeps(torch_, passes, name):
    df, g, st = passes(name)
    pl = pkg("pipeline")
    lc = st["lcosts"].astype(np.float32)
    H, W = df.p.pich, df.p.picw
    prev = torch_.empty_like(df.bestlabels)
    for sweeps in (0, 2):
        if sweeps:
            df.ceoBCD(2)
        lab = golden_labels(g, 0, sweeps)
        assert np.array_equal(df.bestlabels.cpu().numpy(), lab)
        ref = bcd_stats_ref(st["proposals"], lc, st["nprop"], lab, df.p.tpsi, df.p.tphi,
                            prev=golden_labels(g, 0, 0) if sweeps else None)
        t = df.bcd_stats(prev=prev if sweeps else None, prev_out=prev)
        got = check(t.cpu().numpy().tobytes(), ref, "%s after %d sweeps:" % (name, sweeps))
        d = pl.bcd_stats_dict(t, df.p.lamda, H * W)
        assert {k: d[k] for k in got} == got
        assert d["energy"] == df.p.lamda * got["data_sum"] + got["smooth_sum"] and d["changed_frac"] == got["n_changed"] / (H * W)
        assert np.array_equal(prev.cpu().numpy(), lab)
    # the statistics left the records of dflow_bcd_prepare alone: the third sweep still gives the golden labels
    df.ceoBCD(1)
    assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, 0, 3))


def test_stop_none_is_todays_run(torch_, passes):
    df, g, _ = passes(GOLDEN_NAMES[0])
    assert df.ceoBCD(2, stop=None) is None
    assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, 0, 2))


def test_stop_after_exactly_one_sweep(torch_, passes):
    df, g, _ = passes(GOLDEN_NAMES[0])
    seen = []
    hist = df.ceoBCD(6, on_sweep=seen.append, stop={"changed_frac": 1.0})
    assert [h["sweep"] for h in hist] == [0, 1] and seen == [1]
    assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, 0, 1))
    assert hist[0]["n_changed"] == 0 and hist[1]["n_changed"] == int((golden_labels(g, 0, 1) != golden_labels(g, 0, 0)).sum())


def test_rule_that_never_fires_runs_every_sweep(torch_, passes):
    df, g, st = passes(GOLDEN_NAMES[0])
    hist = df.ceoBCD(3, stop={"changed_frac": 0.0, "rel_energy": -1e9})
    assert [h["sweep"] for h in hist] == [0, 1, 2, 3]
    assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, 0, 3))
    lc = st["lcosts"].astype(np.float32)
    for w, h in enumerate(hist):
        ref = bcd_stats_ref(st["proposals"], lc, st["nprop"], golden_labels(g, 0, w), df.p.tpsi, df.p.tphi,
                            prev=golden_labels(g, 0, w - 1) if w else None)
        for k in INT_FIELDS:
            assert h[k] == ref[k], (w, k)
        assert h["energy"] == df.p.lamda * h["data_sum"] + h["smooth_sum"]
        assert h["changed_frac"] == ref["n_changed"] / (df.p.pich * df.p.picw)


def test_energy_rule_stops_on_a_small_gain(torch_, passes):
    """rel_energy = 1: (E_prev - E) / E_prev <= 1 holds for every E >= 0, so the first sweep ends the pass."""
    df, g, _ = passes(GOLDEN_NAMES[0])
    hist = df.ceoBCD(3, stop={"rel_energy": 1.0})
    assert [h["sweep"] for h in hist] == [0, 1]
    assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, 0, 1))


def test_batch_a_stopped_pass_leaves_the_later_sweeps(torch_, passes):
    """Forward and backward pass of one fixture, a threshold between their change counts of sweep 2 (known from the golden
    labels): each pass ends where its own counts say, with the golden labels of that sweep."""
    name = GOLDEN_NAMES[0]
    (d0, g, _), (d1, _, _) = passes(name, 0), passes(name, 1)
    npix = d0.p.pich * d0.p.picw
    T = int(g["bcd_times"])
    counts = [[int((golden_labels(g, b, w) != golden_labels(g, b, w - 1)).sum()) for w in range(1, T + 1)] for b in (0, 1)]
    lo, hi = sorted((counts[0][1], counts[1][1]))
    assert lo < hi, counts
    frac = (lo + hi) / 2 / npix
    want = [next((w for w in range(1, T + 1) if c[w - 1] / npix <= frac), T) for c in counts]
    assert sorted(want) == [2, 3], (counts, want)
    seen = []
    hists = pkg("pipeline").ceoBCD_batch([d0, d1], T, on_sweep=seen.append, stop={"changed_frac": frac})
    assert seen == [1, 2, 3]
    for b, (df, h) in enumerate(zip((d0, d1), hists)):
        assert [e["sweep"] for e in h] == list(range(want[b] + 1)), (b, counts)
        assert [e["n_changed"] for e in h[1:]] == counts[b][:want[b]]
        assert np.array_equal(df.bestlabels.cpu().numpy(), golden_labels(g, b, want[b])), b
    # the same passes one by one give the same histories
    for b in (0, 1):
        df, _, _ = passes(name, b)
        assert df.ceoBCD(T, stop={"changed_frac": frac}) == hists[b]
    with pytest.raises(ValueError):
        d0.ceoBCD(1, stop={"changed": 0.5})
