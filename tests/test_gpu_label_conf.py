"""dflow_label_confidence and dflow_flow_gate on the GPU against tests/label_conf_ref.py (the definition in numpy float64).  No step
of the definition depends on an order, so every comparison is bit for bit: margins as uint32 words, alt, the sparse field and the
counts equal.  The states and parameter sets are those of label_conf_ref.SHAPES and COMBOS, whose contents tests/
test_label_conf_ref.py checks on the CPU.  Every output lies in a plane of its exact size between poisoned guard bands
(tests/ws_guard.py).  Run with `pytest -m gpu`."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import GOLDEN_NAMES, pkg
from label_conf_ref import COMBOS, COUNTS, DATA, LOCAL, SHAPES, THRESH, flow_gate_ref, gpu_state, label_conf_ref
from ws_guard import GuardedWs

pytestmark = pytest.mark.gpu

POISON = 0x7F
OUTPUTS = ("margin", "alt", "sparse", "counts")
DTYPES = dict(margin=np.uint32, alt=np.int32, sparse=np.uint32, counts=np.int32)      # float planes are compared as their words


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


class Device:
    """A label_conf_ref.RandomState on the device, as the C-ABI lays it out."""

    def __init__(self, torch, s):
        self.torch, self.s, self.dev = torch, s, torch.device("cuda", 0)
        self.d_prop = torch.from_numpy(s.packed().view(np.int32)).to(self.dev)
        self.d_cost = torch.from_numpy(s.costs).to(self.dev)
        self.d_nprop = torch.from_numpy(s.nprop.astype(np.int32)).to(self.dev)
        self.d_labels = torch.from_numpy(s.labels.astype(np.int32)).to(self.dev)

    def call(self, tpsi, lamda, mode, min_sep, thresh, want=OUTPUTS):
        """One dflow_label_confidence through _lib with the outputs `want`, each in a guarded plane of its exact size; returns
        {name: the plane as a flat numpy array} after checking the guard bands."""
        L = pkg("_lib")
        s = self.s
        p = L.default_params(s.H, s.W, 1, 1, tpsi=tpsi, lamda=lamda, maxnprop=s.maxnprop, label_pitch=s.label_pitch)
        n = s.H * s.W
        nbytes = dict(margin=4 * n, alt=4 * n, sparse=12 * n, counts=4 * len(COUNTS))
        planes = {name: GuardedWs(self.torch, nbytes[name], POISON, self.dev) for name in want}
        L.call("dflow_label_confidence", C.byref(p), self.d_prop.data_ptr(), self.d_cost.data_ptr(), self.d_nprop.data_ptr(),
               self.d_labels.data_ptr(), mode, min_sep, thresh, *[planes[k].ptr if k in planes else None for k in OUTPUTS],
               L.stream(self.dev))
        out = {}
        for name, g in planes.items():
            g.assert_guards("%dx%d %s" % (s.H, s.W, name))
            out[name] = np.frombuffer(g.snapshot(), DTYPES[name])
        return out


def expected(r):
    return dict(margin=r["margin"].view(np.uint32).reshape(-1), alt=r["alt"].reshape(-1), sparse=r["sparse"].view(np.uint32).reshape(-1),
                counts=np.asarray(r["counts"], np.int32))


def compare(got, want, what):
    for name, a in got.items():
        bad = np.flatnonzero(a != want[name])
        assert bad.size == 0, "%s: %s differs at %d of %d entries, first %d: got %r, expected %r" % (
            what, name, bad.size, a.size, bad[0], a[bad[0]], want[name][bad[0]])


@pytest.mark.parametrize("shape", SHAPES)
def test_random_states_match_the_reference_bit_for_bit(torch_, shape):
    devices = {}
    for lp, maxnprop, tpsi, min_sep, mode, lamda, quantised in COMBOS:
        s = gpu_state(shape, lp, maxnprop, quantised)
        d = devices.setdefault(id(s), Device(torch_, s))
        what = "%dx%d pitch %d tpsi %d min_sep %d mode %d lamda %g" % (shape + (lp, tpsi, min_sep, mode, lamda))
        want = expected(s.ref(tpsi, lamda, mode=mode, min_sep=min_sep, thresh=THRESH))
        got = d.call(tpsi, lamda, mode, min_sep, THRESH)
        print(what, dict(zip(COUNTS, got["counts"].tolist())))
        compare(got, want, what)
        again = d.call(tpsi, lamda, mode, min_sep, THRESH)
        assert all(np.array_equal(got[k], again[k]) for k in OUTPUTS), "%s: two calls must give identical bytes" % what


def test_every_subset_of_outputs_gives_the_same_bytes(torch_):
    lp, maxnprop, tpsi, min_sep, mode, lamda, quantised = COMBOS[4]
    d = Device(torch_, gpu_state((33, 65), lp, maxnprop, quantised))
    full = d.call(tpsi, lamda, mode, min_sep, THRESH)
    compare(full, expected(d.s.ref(tpsi, lamda, mode=mode, min_sep=min_sep, thresh=THRESH)), "all outputs")
    for r in range(1, len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, r):
            got = d.call(tpsi, lamda, mode, min_sep, THRESH, want=want)
            assert set(got) == set(want)
            compare(got, full, "outputs %s" % (want,))


@pytest.mark.parametrize("thresh", (-np.inf, np.inf, 1.5, -2.0))
def test_thresholds_and_infinities(torch_, thresh):
    """-Inf keeps every labelled pixel, +Inf those without an alternative; the compare is made in float32."""
    lp, maxnprop, tpsi, min_sep, mode, lamda, quantised = COMBOS[3]
    d = Device(torch_, gpu_state((33, 65), lp, maxnprop, quantised))
    want = d.s.ref(tpsi, lamda, mode=mode, min_sep=min_sep, thresh=thresh)
    got = d.call(tpsi, lamda, mode, min_sep, float(thresh))
    compare(got, expected(want), "thresh %g" % thresh)
    if thresh == -np.inf:
        assert got["counts"][5] == got["counts"][0]
    if thresh == np.inf:
        assert got["counts"][5] == got["counts"][2] > 0


def test_captured_into_a_graph(torch_):
    """Asynchronous, nothing read back: the call can be captured, and a replay gives the bytes of a plain call."""
    L = pkg("_lib")
    lp, maxnprop, tpsi, min_sep, mode, lamda, quantised = COMBOS[0]
    d = Device(torch_, gpu_state((33, 65), lp, maxnprop, quantised))
    s = d.s
    plain = d.call(tpsi, lamda, mode, min_sep, THRESH)
    p = L.default_params(s.H, s.W, 1, 1, tpsi=tpsi, lamda=lamda, maxnprop=s.maxnprop, label_pitch=s.label_pitch)
    margin = torch_.zeros((s.H, s.W), dtype=torch_.float32, device=d.dev)
    counts = torch_.full((6,), -7, dtype=torch_.int32, device=d.dev)
    torch_.cuda.synchronize()
    side = torch_.cuda.Stream(device=d.dev)
    graph = torch_.cuda.CUDAGraph()
    with torch_.cuda.graph(graph, stream=side):
        L.call("dflow_label_confidence", C.byref(p), d.d_prop.data_ptr(), d.d_cost.data_ptr(), d.d_nprop.data_ptr(),
               d.d_labels.data_ptr(), mode, min_sep, THRESH, margin.data_ptr(), None, None, counts.data_ptr(), L.stream(d.dev))
    torch_.cuda.synchronize()
    assert (counts == -7).all().item(), "a captured call must not run before the replay"
    for _ in range(2):
        graph.replay()
    torch_.cuda.synchronize()
    assert np.array_equal(margin.cpu().numpy().view(np.uint32).reshape(-1), plain["margin"])
    assert np.array_equal(counts.cpu().numpy(), plain["counts"])


def test_confidence_of_a_real_pass_equals_the_reference_on_its_host_state(torch_, golden):
    """End to end at a small golden geometry: after DiscreteFlow.run, df.confidence(...) against the reference on df.host_state()."""
    pipeline = pkg("pipeline")
    g = golden(GOLDEN_NAMES[0])
    df = pipeline.DiscreteFlow(int(g["H"]), int(g["W"]), int(g["cellh"]), int(g["cellw"]), seed=int(g["seed"]))
    flow = df.run(g["img1"], g["img2"], 2).cpu().numpy()
    st = df.host_state()
    for mode, name in ((LOCAL, "local"), (DATA, "data")):
        for min_sep in (0, 1):
            want = label_conf_ref(st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"], df.p.tpsi, df.p.lamda, mode=mode,
                                  min_sep=min_sep, thresh=0.25)
            margin, alt, sparse, counts = df.confidence(mode=name, min_sep=min_sep, thresh=0.25, alt=True, sparse=True, counts=True)
            got = dict(margin=margin.cpu().numpy().view(np.uint32).reshape(-1), alt=alt.cpu().numpy().reshape(-1),
                       sparse=sparse.cpu().numpy().view(np.uint32).reshape(-1), counts=counts.cpu().numpy())
            print(name, min_sep, dict(zip(COUNTS, got["counts"].tolist())))
            compare(got, expected(want), "golden %s, mode %s, min_sep %d" % (GOLDEN_NAMES[0], name, min_sep))
            assert want["counts"][0] == df.p.pich * df.p.picw and 0 < want["counts"][5] < want["counts"][0]
            # the kept vectors are the pass's own flow
            keep = sparse.cpu().numpy()[..., 2] == 1
            assert np.array_equal(sparse.cpu().numpy()[keep][:, :2], flow[keep][:, ::-1])
    # the margin alone, and the same plane
    only = df.confidence(mode="data", min_sep=1)
    assert isinstance(only, torch_.Tensor) and np.array_equal(only.cpu().numpy().view(np.uint32).reshape(-1), got["margin"])
    assert pipeline.LABEL_CONF_COUNTS == COUNTS


# ---------------------------------------------------------------- the gate
def gate_case(H, W, seed):
    """A [U,V,valid] field with invalid and non-finite vectors, and scores with NaN, +-Inf and values exactly at lo and hi."""
    rng = np.random.default_rng(seed)
    uvv = np.concatenate([rng.normal(0, 3, (H, W, 2)), (rng.random((H, W, 1)) < 0.8)], axis=2).astype(np.float32)
    flat = uvv.reshape(-1, 3)
    n = flat.shape[0]
    flat[rng.integers(0, n, max(1, n // 20)), 0] = np.nan
    flat[rng.integers(0, n, max(1, n // 20)), 1] = np.inf
    flat[rng.integers(0, n, max(1, n // 20)), 0] = -0.0
    score = rng.normal(0, 1, (H, W)).astype(np.float32)
    sf = score.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, -0.5, 0.75):
        sf[rng.integers(0, n, max(1, n // 10))] = v
    return uvv, score


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (33, 65), (131, 257)])
def test_flow_gate_both_layouts_and_in_place(torch_, shape):
    pipeline, L = pkg("pipeline"), pkg("_lib")
    H, W = shape
    uvv, score = gate_case(H, W, seed=H * W)
    dydx = np.ascontiguousarray(uvv[..., [1, 0]])
    for flow in (uvv, dydx):
        for lo, hi in ((-0.5, 0.75), (-np.inf, np.inf), (0.75, 0.75), (-np.inf, -0.5)):
            want, want_counts = flow_gate_ref(flow, score, lo, hi)
            out, counts = pipeline.flow_gate(flow, score, lo=lo, hi=hi, counts=True)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (shape, flow.shape, lo, hi)
            assert counts.cpu().tolist() == want_counts
            assert np.array_equal(pipeline.flow_gate(flow, score, lo=lo, hi=hi).cpu().numpy().view(np.uint32), want.view(np.uint32))
    # in place under [U,V,valid], in an exact-size plane between guard bands
    dev = torch_.device("cuda", 0)
    g = GuardedWs(torch_, 12 * H * W, POISON, dev)
    g.region.copy_(torch_.from_numpy(uvv.reshape(-1).view(np.uint8)).to(dev))
    d_score = torch_.from_numpy(score).to(dev)
    L.call("dflow_flow_gate", H, W, g.ptr, L.EVAL_UVV, d_score.data_ptr(), -0.5, 0.75, g.ptr, None, L.stream(dev))
    g.assert_guards("flow_gate in place %dx%d" % shape)
    assert np.array_equal(np.frombuffer(g.snapshot(), np.uint32), flow_gate_ref(uvv, score, -0.5, 0.75)[0].view(np.uint32).reshape(-1))


def test_flow_gate_with_the_margin_is_the_sparse_field(torch_):
    """The consumer's path: gating the flow of a labelling by its margin plane gives the sparse field of the confidence call."""
    pipeline = pkg("pipeline")
    lp, maxnprop, tpsi, min_sep, mode, lamda, quantised = COMBOS[4]
    s = gpu_state((33, 65), lp, maxnprop, quantised)
    r = s.ref(tpsi, lamda, mode=mode, min_sep=min_sep, thresh=THRESH)
    ok = (s.labels >= 0) & (s.labels < s.nprop)
    chosen = np.take_along_axis(s.flows, np.clip(s.labels, 0, lp - 1)[:, :, None, None], axis=2)[:, :, 0, :]
    uvv = np.concatenate([chosen[..., ::-1], ok[..., None]], axis=2).astype(np.float32)
    out = pipeline.flow_gate(uvv, r["margin"], lo=THRESH)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), r["sparse"].view(np.uint32))
