"""CPU side of the EPIC parameter sweep: the inputs of epic_param_cases.py do to the reference (epic_ref.py) what
test_gpu_epic_params.py relies on, and the float32 yardstick of the flow is measured here.  No GPU needed."""
import numpy as np
import pytest

import epic_param_cases as E
import epic_prefilter_ref as P
import epic_ref as R
from test_gpu_epic_prefilter import CAP, TOL_B


@pytest.mark.parametrize("name", E.FULL_LIST_INPUTS)
def test_every_nearest_256_list_is_full(name):
    r = E.ref(name)
    print("%s: %d seeds, shortest list %d, longest seed-graph row %d" % (name, len(r.seeds), r.length.min(),
                                                                          max(len(v) for v in r.graph.values())))
    assert r.length.min() >= 256
    assert R.verify_fixed_point(r.sparse, r.edges, r.S, r.D) is None
    if name == "ties32x48":                                # every cost 1: D ties and G ties, broken by the seed id
        assert (R.costs(r.edges) == 1).all()
        tied = sum(len(set(g.tolist())) < len(g) for g in r.G)
        print("%s: %d of %d lists hold equal G" % (name, tied, len(r.seeds)))
        assert tied == len(r.seeds)


@pytest.mark.parametrize("name,edges", [("hub64x96", 129), ("hub72x104", 193)])
def test_hub_row_spans_several_chunks(name, edges):
    r = E.ref(name)
    hub, (H, W, half) = E.hub_id(name), E.HUBS[name]
    row = r.graph[hub]
    cell = r.S == hub
    print("%s: %d seeds, hub row %d edges to %d distinct seeds, cell of %d pixels, shortest list %d" % (
        name, len(r.seeds), len(row), len(set(row)), cell.sum(), r.length.min()))
    assert len(row) >= edges and len(set(row)) >= edges
    side = 2 * half - 1
    assert cell.sum() == side * side and cell[H // 2 - half + 1:H // 2 + half, W // 2 - half + 1:W // 2 + half].all()
    assert r.length.min() >= 256
    # the hub settles first in its own list, with nothing else settled or on the frontier: at nn = 256 its whole row is
    # pushed in one scan
    assert r.lists[hub][0] == (hub, 0) and hub not in row


@pytest.mark.parametrize("name", E.INTERP_INPUTS + ("hub72x104", "edgevalues"))
def test_prefix_law(name):
    """neighbour_list(graph, s, n) == neighbour_list(graph, s, 256)[:n]: every nn's reference is a slice of one walk."""
    r = E.ref(name)
    for s in r.seeds[::max(1, len(r.seeds) // 24)].tolist() + ([E.hub_id(name)] if name in E.HUBS else []):
        for n in E.NNS:
            assert R.neighbour_list(r.graph, s, n) == r.lists[s][:n], (name, s, n)


def test_fit_prefixes_is_fit():
    for name, k in (("dense32x48", 0.8), ("dense32x48", 10.0), ("hub64x96", 200.0), ("edgevalues", 0.8)):
        r = E.ref(name)
        f = E.fits(name, k)
        for nn in (1, 2, 3, 65, 256):
            for i in range(0, len(r.seeds), 53):
                s = int(r.seeds[i])
                for method in ("LA", "NW"):
                    model, lmin = R.fit(r.sparse, s, r.lists[s][:nn], k, method)
                    assert np.array_equal(np.array(model), f[nn][method][i]), (name, k, nn, s, method)
                    assert (lmin is None and np.isnan(f[nn]["lmin"][i])) or lmin == f[nn]["lmin"][i]
    r = E.ref("sparse32x48")
    whole = R.interpolate(r.sparse, r.edges, 65, 0.8, "LA")
    assert np.array_equal(whole["flow"], E.interp_case("sparse32x48", 65, 0.8, "LA")["flow"])
    assert np.array_equal(whole["S"], r.S) and np.array_equal(whole["D"], r.D)


def test_edgevalues_covers_every_kind():
    sp, e = E.inputs("edgevalues")
    seeds = R.seed_mask(sp)
    print("edgevalues: %d seeds of %d pixels" % (seeds.sum(), seeds.size))
    assert 0.25 < seeds.mean() < 0.35
    bits = e.view(np.uint32)
    for v in E.EDGE_VALUES:                                # by bit pattern: NaN, and -0.0 apart from 0.0
        at = bits == np.float32(v).view(np.uint32)
        assert (at & seeds).any() and (at & ~seeds).any(), v
    valid = sp[..., 2].view(np.uint32)
    finite = np.isfinite(sp[..., 0]) & np.isfinite(sp[..., 1])
    for v in E.VALID_VALUES:
        at = (valid == np.float32(v).view(np.uint32)) & finite & (sp[..., 0] != 0)
        assert at.any() and (seeds[at] == bool(v > 0.5)).all(), v      # NaN > 0.5 is False
    bad = (sp[..., 2] == 1) & ~finite
    assert bad.sum() == 3 and not seeds[bad].any()
    assert np.isnan(sp[bad]).any() and np.isposinf(sp[bad]).any() and np.isneginf(sp[bad]).any()
    c = R.costs(e)
    want = dict(zip(E.EDGE_VALUES.view(np.uint32).tolist(), (1001, 1, 1, 1, 1, 1, 3, 3, 501, 1001, 1001, 1001, 1001, 1001)))
    assert all((c[bits == b] == w).all() for b, w in want.items())     # 0.5 and 2.5 round to even, 1.5 to 2


def test_extreme_k_weights():
    """k = 1e-300 makes every weight exactly 1, k = 1e300 every weight but the seed's own exactly 0; k = 10 puts seeds on
    both sides of TAU and some close to it."""
    for name in E.K_SWEEP_INPUTS:
        r = E.ref(name)
        G = r.G[:, 1:].astype(np.float64)
        assert (np.exp(-(1e-300 * G) / 2000.0) == 1.0).all()
        with np.errstate(over="ignore"):
            assert (np.exp(-(1e300 * G) / 2000.0) == 0.0).all()
        own = r.sparse.reshape(-1, 3)[r.seeds]
        for nn in E.K_SWEEP_NNS:
            f = E.fits(name, 1e300)[nn]
            assert (f["lmin"] == 0).all()                  # LA falls back everywhere
            for method in ("LA", "NW"):
                assert np.array_equal(f[method][:, [0, 3]], own[:, :2].astype(np.float64)) and not f[method][:, [1, 2, 4, 5]].any()
    f = E.fits("dense32x48", 10.0)[256]
    below, close = (f["lmin"] < R.TAU).sum(), (np.abs(f["lmin"] - R.TAU) <= 0.01 * R.TAU).sum()
    print("dense32x48 k=10 nn=256: %d of %d seeds below TAU, %d within 1 %% of it" % (below, len(f["lmin"]), close))
    assert below > 0 and (f["lmin"] >= R.TAU).sum() > 0 and close > 0


def _interp_cases():
    for name in E.INTERP_INPUTS:
        for nn in E.NNS:
            yield name, nn, 0.8
    for name in E.K_SWEEP_INPUTS:
        for nn in E.K_SWEEP_NNS:
            for k in E.KS:
                yield name, nn, k
    for nn in (65, 256):
        yield "edgevalues", nn, 0.8
    for nn in E.WIDE_HUB_NNS:
        yield "hub72x104", nn, 0.8


def test_exclusion_cap_and_yardstick():
    """Prints the float32 yardstick (the reference's float32 fill of its float32-rounded models against its float64 fill)
    and the seeds excluded for a lambda_min within 1 % of TAU, per case; the cap on the latter is a condition."""
    worst = (0.0, ())
    for name, nn, k in _interp_cases():
        for method in ("LA", "NW"):
            c = E.interp_case(name, nn, k, method)
            if c["excluded"] or c["yard"] > worst[0]:
                print("%s nn=%d k=%g %s: excluded %d of %d seeds, yardstick %.3e px, tolerance %.3e px" % (
                    name, nn, k, method, c["excluded"], c["seeds"], c["yard"], c["tol"]))
            assert c["excluded"] <= E.EXCLUSION_CAP * c["seeds"]
            assert np.isfinite(c["flow"]).all() and c["tol"] < 1e-4
            worst = max(worst, (c["yard"], (name, nn, k, method)))
    print("largest yardstick %.4e px at %s" % worst)


@pytest.mark.parametrize("name", E.PREF_INPUTS)
def test_prefilter_cases(name):
    """prefilter_case() is P.prefilter(); no seed lies within TOL_B of the threshold beyond the pre-filter's CAP, no estimate
    is non-finite, and both decisions occur in every case."""
    r = E.ref(name)
    for pref_nn, k in ((2, 0.05), (64, 10.0)) if name != "hub64x96" else ((129, 0.8),):
        a, b = E.prefilter_case(name, pref_nn, k), P.prefilter(r.sparse, r.edges, None, 0.0, pref_nn, E.PREF_TH, k)
        assert np.array_equal(a["reason"], b["reason"]) and np.array_equal(a["estimate"], b["estimate"])
        assert list(a["dist"]) == list(b["dist"]) and a["out"].tobytes() == b["out"].tobytes()
        assert np.allclose(list(a["dist"].values()), list(b["dist"].values()), rtol=1e-14, atol=0)     # x * x here, x ** 2 there
    worst = 0
    for pref_nn in E.PREF_NNS:
        for k in E.PREF_KS:
            c = E.prefilter_case(name, pref_nn, k)
            close = sum(abs(d - E.PREF_TH) <= TOL_B for d in c["dist"].values())
            worst = max(worst, close)
            assert close <= CAP * len(r.seeds), (pref_nn, k, close)
            assert np.isfinite(c["estimate"]).all(), (pref_nn, k)
            assert (c["reason"] == P.KEPT).any() and (c["reason"] == P.CONSISTENCY).any(), (pref_nn, k)
    print("%s: at most %d seeds within TOL_B of pref_th over %d cases" % (name, worst, len(E.PREF_NNS) * len(E.PREF_KS)))
    c = E.prefilter_case("edgevalues", 64, 0.8)
    assert (c["reason"][~R.seed_mask(E.inputs("edgevalues")[0])] == P.NONE).all()
