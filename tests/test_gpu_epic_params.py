"""dflow_epic_interpolate and stage B of dflow_epic_prefilter across the accepted nn, pref_nn and k range, against
epic_ref.py on the inputs of epic_param_cases.py: lists of up to 256 entries (all four register slots of epic_dijkstra's
frontier and settled list), seed-graph rows of 156 and 196 edges (three and four 64-edge chunks), G ties everywhere, nn = 1, 2, 3, k from
"every weight 1" to "every weight 0", and special values in the edge map and the valid plane.  S, D, lists and list_g are
held byte for byte; every output buffer holds a sentinel and the workspace 0x7F bytes before each call.
Run with `pytest -m gpu`.

Tolerances.  The flow of a case is held to 4 x max(yardstick, half a float32 ulp at the case's largest |flow|): the
yardstick is the reference itself, its float64 models rounded to float32 and filled in float32 in the written order
(m0 + m1 dx) + m2 dy, against its float64 fill (epic_param_cases.interp_case; computed per case from the reference alone).
The margin of 4 pays for one fused or reordered float32 operation in the fill and for an exp that differs in the last
place.  Over all cases the yardstick is at most 5.4836e-6 px (sparse32x48, nn = 3, k = 0.8, LA; measured on the CPU,
tests/test_epic_params_ref.py prints it), so no tolerance here exceeds 2.2e-5 px.  Seeds whose reference lambda_min lies
within 1 % of TAU are left out of the LA flow comparison, at most 1 % of a case's seeds.  The pre-filter's estimates, float32
roundings of a double quotient, are held to 4 x half a float32 ulp at the largest |estimate| on top of what compare() of
test_gpu_epic_prefilter.py asserts."""
import numpy as np
import pytest

import epic_param_cases as E
import epic_prefilter_ref as P
import epic_ref as R
from conftest import pkg
from test_gpu_epic_prefilter import compare

pytestmark = pytest.mark.gpu

I32_SENTINEL, I64_SENTINEL, U8_SENTINEL = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0xEE


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def interpolate(torch, sparse, edges, nn, k, method):
    """dflow_epic_interpolate on sentinel-filled outputs and a workspace of 0x7F bytes -> flow, S, D (uint32), lists, list_g."""
    L, pipeline = pkg("_lib"), pkg("pipeline")
    dev = torch.device("cuda", 0)
    H, W = edges.shape
    sp, ed = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sparse, edges))
    ws, ws_bytes = L.workspace("dflow_epic_workspace_bytes", H, W, dev)
    ws.fill_(0x7F)
    flow = torch.full((H, W, 2), float("nan"), dtype=torch.float32, device=dev)
    S, D = (torch.full((H, W), I32_SENTINEL, dtype=torch.int32, device=dev) for _ in range(2))
    lst = torch.full((H * W, nn), I32_SENTINEL, dtype=torch.int32, device=dev)
    lg = torch.full((H * W, nn), I64_SENTINEL, dtype=torch.int64, device=dev)
    L.call("dflow_epic_interpolate", H, W, sp.data_ptr(), ed.data_ptr(), nn, float(k), pipeline.EPIC_METHODS[method],
           flow.data_ptr(), S.data_ptr(), D.data_ptr(), lst.data_ptr(), lg.data_ptr(), ws.data_ptr(), ws_bytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    return flow.cpu().numpy(), S.cpu().numpy(), D.cpu().numpy().view(np.uint32), lst.cpu().numpy(), lg.cpu().numpy()


def prefilter(torch, sparse, edges, pref_nn, k, pref_th=E.PREF_TH):
    """Stage B of dflow_epic_prefilter alone (no image, saliency_th = 0), on sentinels as above -> out, reason, saliency, estimate."""
    L = pkg("_lib")
    dev = torch.device("cuda", 0)
    H, W = edges.shape
    sp, ed = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sparse, edges))
    ws, ws_bytes = L.workspace("dflow_epic_prefilter_workspace_bytes", H, W, dev)
    ws.fill_(0x7F)
    out = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device=dev)
    reason = torch.full((H, W), U8_SENTINEL, dtype=torch.uint8, device=dev)
    sal = torch.full((H, W), float("nan"), dtype=torch.float32, device=dev)
    est = torch.full((H, W, 2), float("nan"), dtype=torch.float32, device=dev)
    L.call("dflow_epic_prefilter", H, W, None, sp.data_ptr(), ed.data_ptr(), 0.0, pref_nn, float(pref_th), float(k), out.data_ptr(),
           reason.data_ptr(), sal.data_ptr(), est.data_ptr(), ws.data_ptr(), ws_bytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), reason.cpu().numpy(), sal.cpu().numpy(), est.cpu().numpy()


def check_diagram_and_lists(name, nn, got):
    """S, D, lists and list_g byte-equal to the reference's prefix of length nn, -1 pads after it and in every other row."""
    r = E.ref(name)
    _, S, D, lst, lg = got
    assert np.array_equal(S, r.S), "S differs at %s" % np.argwhere(S != r.S)[:5].tolist()
    assert np.array_equal(D.astype(np.int64), r.D), "D differs at %s" % np.argwhere(D != r.D)[:5].tolist()
    ids, G = r.list_planes(nn)
    bad = np.flatnonzero((lst != ids).any(axis=1))
    assert bad.size == 0, "lists differ in %d rows, first %d at position %d" % (
        bad.size, bad[0], np.flatnonzero(lst[bad[0]] != ids[bad[0]])[0])
    bad = np.flatnonzero((lg != G).any(axis=1))
    assert bad.size == 0, "list_g differs in %d rows, first %d" % (bad.size, bad[0])


def check_flow(name, nn, k, method, flow):
    c = E.interp_case(name, nn, k, method)
    assert c["excluded"] <= E.EXCLUSION_CAP * c["seeds"]
    assert np.isfinite(flow).all(), "the flow holds %d non-finite values" % (~np.isfinite(flow)).sum()
    err = float(np.abs(flow - c["flow"])[c["keep"]].max())
    print("%s nn=%d k=%g %s: max |gpu - float64| = %.3e (tolerance %.3e, yardstick %.3e, %d of %d seeds excluded)" % (
        name, nn, k, method, err, c["tol"], c["yard"], c["excluded"], c["seeds"]))
    assert err <= c["tol"], (name, nn, k, method, err, c["tol"])


def own_flow(name):
    """(H,W,2) float32 [dy,dx]: every pixel carries the flow of its Voronoi seed."""
    r = E.ref(name)
    return np.ascontiguousarray(r.sparse.reshape(-1, 3)[r.S.ravel()][:, [1, 0]].reshape(r.H, r.W, 2))


@pytest.fixture(scope="module")
def lists256(torch_):
    """The GPU's own lists at nn = 256, per input: what its lists at a smaller nn must be a prefix of."""
    cache = {}

    def get(name):
        if name not in cache:
            r = E.ref(name)
            cache[name] = interpolate(torch_, r.sparse, r.edges, 256, 0.8, "NW")[3:]
        return cache[name]
    return get


@pytest.mark.parametrize("nn", E.NNS)
@pytest.mark.parametrize("name", E.INTERP_INPUTS)
def test_interpolation_over_nn(torch_, lists256, name, nn):
    r = E.ref(name)
    got = {m: interpolate(torch_, r.sparse, r.edges, nn, 0.8, m) for m in ("LA", "NW")}
    for m in ("LA", "NW"):
        check_diagram_and_lists(name, nn, got[m])
    lst, lg = lists256(name)
    assert np.array_equal(got["LA"][3], lst[:, :nn]) and np.array_equal(got["LA"][4], lg[:, :nn]), "the GPU's own prefix law"
    for m in ("LA", "NW"):
        check_flow(name, nn, 0.8, m, got[m][0])
    if nn < 3:                                             # too short for a covariance: LA is NW, bit for bit
        assert got["LA"][0].tobytes() == got["NW"][0].tobytes()
    if nn == 1:
        assert got["NW"][0].tobytes() == own_flow(name).tobytes()


@pytest.mark.parametrize("k", E.KS)
@pytest.mark.parametrize("nn", E.K_SWEEP_NNS)
@pytest.mark.parametrize("name", E.K_SWEEP_INPUTS)
def test_interpolation_over_k(torch_, name, nn, k):
    r = E.ref(name)
    for m in ("LA", "NW"):
        got = interpolate(torch_, r.sparse, r.edges, nn, k, m)
        check_diagram_and_lists(name, nn, got)
        check_flow(name, nn, k, m, got[0])
        if k == 1e300:                                     # every other weight is 0: the covariance is 0 < TAU, LA falls back
            assert got[0].tobytes() == own_flow(name).tobytes(), m


@pytest.mark.parametrize("nn", E.WIDE_HUB_NNS)
def test_wide_hub_fills_the_fourth_frontier_slot(torch_, nn):
    """The hub of hub72x104 offers 196 entries at once: at nn = 256 the frontier holds them in all four slots; at nn = 193
    it is capped at 192 and the last four replace the largest or are dropped."""
    name = "hub72x104"
    r = E.ref(name)
    for m in ("LA", "NW"):
        got = interpolate(torch_, r.sparse, r.edges, nn, 0.8, m)
        check_diagram_and_lists(name, nn, got)
        check_flow(name, nn, 0.8, m, got[0])
    ref = E.prefilter_case(name, nn - 1, 0.8)
    got = prefilter(torch_, r.sparse, r.edges, nn - 1, 0.8)
    compare(r.sparse, r.edges, None, got, ref, 0.0, E.PREF_TH)
    check_estimate(name, nn - 1, 0.8, got, ref)


def test_edge_and_valid_values(torch_):
    """Special values of the edge map (the clamp, the NaN rule, rintf at .5) and of the valid plane (valid > 0.5) give the
    reference's costs and seeds: S, D and the lists are byte-equal, and nothing the reference's seed_mask rejects is a seed."""
    name = "edgevalues"
    r = E.ref(name)
    seeds = R.seed_mask(r.sparse)
    for nn in (65, 256):
        for m in ("LA", "NW"):
            got = interpolate(torch_, r.sparse, r.edges, nn, 0.8, m)
            check_diagram_and_lists(name, nn, got)
            check_flow(name, nn, 0.8, m, got[0])
            assert seeds.ravel()[got[1].ravel()].all() and (got[3][~seeds.ravel()] == -1).all()
    for pref_nn, k in ((64, 0.8), (255, 10.0)):
        ref = E.prefilter_case(name, pref_nn, k)
        got = prefilter(torch_, r.sparse, r.edges, pref_nn, k)
        compare(r.sparse, r.edges, None, got, ref, 0.0, E.PREF_TH)
        check_estimate(name, pref_nn, k, got, ref)
        assert (got[1][~seeds] == P.NONE).all() and (got[1][seeds] != P.NONE).all()


def check_estimate(name, pref_nn, k, got, ref):
    """The estimates, far tighter than compare()'s 1e-3 px: the GPU rounds a double quotient to float32 once."""
    fin = np.isfinite(ref["estimate"]).all(axis=-1)
    want = ref["estimate"][fin]
    yard = float(np.abs(want.astype(np.float32).astype(np.float64) - want).max())
    tol = E.FACTOR * max(yard, 0.5 * float(np.spacing(np.float32(np.abs(want).max()))))
    err = float(np.abs(got[3][fin] - want).max())
    print("%s pref_nn=%d k=%g: estimate max |gpu - float64| = %.3e (tolerance %.3e)" % (name, pref_nn, k, err, tol))
    assert err <= tol, (name, pref_nn, k, err, tol)


@pytest.mark.parametrize("pref_nn", E.PREF_NNS)
@pytest.mark.parametrize("name", E.PREF_INPUTS)
def test_prefilter_stage_b(torch_, name, pref_nn):
    r = E.ref(name)
    for k in E.PREF_KS:
        ref = E.prefilter_case(name, pref_nn, k)
        assert (ref["reason"] == P.KEPT).any() and (ref["reason"] == P.CONSISTENCY).any()
        assert np.isfinite(ref["estimate"]).all()
        got = prefilter(torch_, r.sparse, r.edges, pref_nn, k)
        compare(r.sparse, r.edges, None, got, ref, 0.0, E.PREF_TH)
        check_estimate(name, pref_nn, k, got, ref)


def test_repeat_is_byte_equal(torch_):
    """The same call twice, and once more through pipeline.epic_interpolate (its own workspace, as torch.empty leaves it):
    nothing depends on what an earlier call left in the workspace or the outputs."""
    r = E.ref("hub64x96")
    a = interpolate(torch_, r.sparse, r.edges, 256, 0.8, "LA")
    interpolate(torch_, r.sparse, np.ones_like(r.edges), 16, 10.0, "NW")      # other contents for the allocator to hand back
    b = interpolate(torch_, r.sparse, r.edges, 256, 0.8, "LA")
    c = pkg("pipeline").epic_interpolate(r.sparse, r.edges, 256, 0.8, "LA", aux=True)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.cpu().numpy().tobytes()
    p = prefilter(torch_, r.sparse, r.edges, 255, 0.8)
    q = prefilter(torch_, r.sparse, r.edges, 255, 0.8)
    for x, y in zip(p, q):
        assert x.tobytes() == y.tobytes()


def test_hub_at_small_nn_replaces_the_largest(torch_):
    """At nn = 16 the hub's row scan offers 156 entries to a frontier capped at 15: about 140 times the new entry replaces
    the largest one or is dropped."""
    r = E.ref("hub64x96")
    hub = E.hub_id("hub64x96")
    got = interpolate(torch_, r.sparse, r.edges, 16, 0.8, "NW")
    want = R.neighbour_list(r.graph, hub, 16)
    assert want == r.lists[hub][:16]
    assert got[3][hub].tolist() == [t for t, _ in want] and got[4][hub].tolist() == [g for _, g in want]
    ids, G = r.list_planes(16)
    assert np.array_equal(got[3], ids) and np.array_equal(got[4], G)
