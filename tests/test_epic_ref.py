"""The numpy restatement of the edge-aware interpolation (epic_ref.py) on cases that can be computed by hand, and the
host-side validation of dflow_epic_interpolate / dflow_epic_workspace_bytes (CPU only, no launch)."""
import ctypes as C
import os

import numpy as np
import pytest

import epic_ref as R
from conftest import pkg


def field(H, W, seeds):
    """(H,W,3) [U,V,valid] with seeds {(y, x): (U, V)}."""
    sp = np.zeros((H, W, 3), np.float32)
    for (y, x), (u, v) in seeds.items():
        sp[y, x] = (u, v, 1.0)
    return sp


def test_costs_clamp_and_read_nan_as_an_edge():
    e = np.array([[0.0, 1.0, -3.0, 7.0, np.nan, 0.25, 0.0005, 0.0015]], np.float32)
    assert R.costs(e).tolist() == [[1, 1001, 1, 1001, 1001, 251, 1, 3]]   # rint halves to even


def test_step_costs_across_one_edge_pixel():
    sp = field(1, 5, {(0, 0): (1.0, 2.0)})
    e = np.zeros((1, 5), np.float32)
    e[0, 2] = 1.0
    S, D = R.voronoi(sp, e)
    assert S.tolist() == [[0] * 5] and D.tolist() == [[0, 2, 1004, 2006, 2008]]
    assert R.verify_fixed_point(sp, e, S, D) is None
    D2 = D.copy()
    D2[0, 3] -= 1
    assert "off the fixed point" in R.verify_fixed_point(sp, e, S, D2)


def test_strip_of_one_row_and_one_column():
    sp = field(1, 9, {(0, 1): (1.0, 0.0), (0, 6): (2.0, 0.0)})
    e = np.zeros((1, 9), np.float32)
    S, D = R.voronoi(sp, e)
    assert S.tolist() == [[1, 1, 1, 1, 6, 6, 6, 6, 6]] and D.tolist() == [[2, 0, 2, 4, 4, 2, 0, 2, 4]]
    St, Dt = R.voronoi(sp.transpose(1, 0, 2), e.T)
    assert (St.ravel() == S.ravel()).all() and (Dt.ravel() == D.ravel()).all()


def test_tied_distance_goes_to_the_lower_id():
    sp = field(3, 3, {(0, 0): (1.0, 0.0), (2, 2): (5.0, 0.0)})
    e = np.zeros((3, 3), np.float32)
    S, D = R.voronoi(sp, e)
    # the anti-diagonal is 4 from both seeds: seed 0 (id 0) wins over seed 8
    assert S.tolist() == [[0, 0, 0], [0, 0, 8], [0, 8, 8]] and D[1, 1] == 4 and D[0, 2] == 4 and D[2, 0] == 4
    assert R.verify_fixed_point(sp, e, S, D) is None
    S2 = S.copy()
    S2[1, 1] = 8
    assert R.verify_fixed_point(sp, e, S2, D) is not None


def test_nn_one_gives_each_cell_its_own_seed():
    rng = np.random.default_rng(1)
    sp = np.zeros((12, 17, 3), np.float32)
    m = rng.random((12, 17)) < 0.1
    sp[m] = np.c_[rng.normal(size=(m.sum(), 2)), np.ones(m.sum())]
    e = rng.random((12, 17)).astype(np.float32)
    for method in ("LA", "NW"):
        r = R.interpolate(sp, e, nn=1, method=method)
        S = r["S"]
        assert all(len(v) == 1 for v in r["lists"].values())
        assert np.array_equal(r["flow"][..., 1], sp.reshape(-1, 3)[S.ravel(), 0].reshape(S.shape))
        assert np.array_equal(r["flow"][..., 0], sp.reshape(-1, 3)[S.ravel(), 1].reshape(S.shape))


def test_seed_graph_and_lists_by_hand():
    sp = field(1, 7, {(0, 0): (0.0, 0.0), (0, 3): (0.0, 0.0), (0, 6): (0.0, 0.0)})
    e = np.zeros((1, 7), np.float32)
    e[0, 4] = 1.0
    S, D = R.voronoi(sp, e)
    assert S.tolist() == [[0, 0, 3, 3, 3, 6, 6]] and D.tolist() == [[0, 2, 2, 0, 1002, 2, 0]]
    g = R.seed_graph(S, D, e)
    assert g == {0: {3: 2 + 1 + 1 + 2}, 3: {0: 6, 6: 1002 + 1001 + 1 + 2}, 6: {3: 2006}}
    assert R.neighbour_list(g, 0, 3) == [(0, 0), (3, 6), (6, 2012)]
    assert R.neighbour_list(g, 6, 2) == [(6, 0), (3, 2006)]


def test_la_recovers_an_affine_field_under_arbitrary_edges():
    rng = np.random.default_rng(7)
    H, W = 40, 56
    ys, xs = np.mgrid[0:H, 0:W]
    U = 1.5 + 0.02 * xs - 0.03 * ys
    V = -2.0 + 0.01 * xs + 0.05 * ys
    m = rng.random((H, W)) < 0.02
    sp = np.zeros((H, W, 3), np.float32)
    sp[..., 0], sp[..., 1], sp[..., 2] = U, V, m
    sp[~m, :2] = 0
    e = rng.random((H, W)).astype(np.float32)
    r = R.interpolate(sp, e, nn=20, method="LA")
    # the seeds hold float32 flows: the field they sample is affine up to float32 rounding of each sample
    assert all(v is not None and v >= R.TAU for v in r["lmin"].values())
    assert np.abs(r["flow"][..., 1] - U).max() < 1e-5 and np.abs(r["flow"][..., 0] - V).max() < 1e-5
    # an exactly representable affine field is recovered to 1e-9
    U = 1.0 + 0.25 * xs - 0.5 * ys
    V = -2.0 + 0.125 * xs + 0.75 * ys
    sp[..., 0], sp[..., 1] = np.where(m, U, 0), np.where(m, V, 0)
    r = R.interpolate(sp, e, nn=20, method="LA")
    assert np.abs(r["flow"][..., 1] - U).max() < 1e-9 and np.abs(r["flow"][..., 0] - V).max() < 1e-9


def test_collinear_seeds_fall_back_to_nw():
    H, W = 9, 20
    seeds = {(4, x): (float(x), 0.0) for x in range(0, 20, 3)}
    sp = field(H, W, seeds)
    e = np.zeros((H, W), np.float32)
    la = R.interpolate(sp, e, nn=5, method="LA")
    nw = R.interpolate(sp, e, nn=5, method="NW")
    assert all(v < R.TAU for v in la["lmin"].values())
    assert np.array_equal(la["flow"], nw["flow"])


def test_no_seed_gives_zero_flow():
    sp = np.zeros((4, 6, 3), np.float32)
    sp[..., 2] = 1.0
    sp[..., 0] = np.nan                                     # valid but not finite: not a seed
    r = R.interpolate(sp, np.zeros((4, 6), np.float32))
    assert not r["flow"].any() and (r["S"] == -1).all() and R.verify_fixed_point(sp, np.zeros((4, 6)), r["S"], r["D"]) is None


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_epic_symbols_are_exported(L):
    handle = C.CDLL(L.LIB_PATH)
    for name in ("dflow_epic_workspace_bytes", "dflow_epic_interpolate", "dflow_epic_last_stats"):
        assert hasattr(handle, name) and name in L.SYMBOLS


def test_epic_workspace_size(L):
    lib = L.lib()
    assert lib.dflow_epic_workspace_bytes(1, 1) > 0
    a, b = lib.dflow_epic_workspace_bytes(100, 100), lib.dflow_epic_workspace_bytes(200, 200)
    assert 3.5 * a < b < 4.5 * a                            # linear in h*w, no h*w*nn term
    for h, w in ((0, 5), (5, 0), (-1, 5), (8193, 5), (5, 8193)):
        assert lib.dflow_epic_workspace_bytes(h, w) == 0 and b"image size" in lib.dflow_last_error()
    assert lib.dflow_epic_workspace_bytes(8192, 8192) > 0


def test_epic_interpolate_rejects_bad_calls_before_any_launch(L):
    lib = L.lib()
    ws = lib.dflow_epic_workspace_bytes(20, 30)

    def call(h=20, w=30, sparse=1 << 20, edges=1 << 20, nn=100, k=0.8, method=0, flow=1 << 20, d_ws=1, wsb=ws):
        return lib.dflow_epic_interpolate(h, w, sparse, edges, nn, k, method, flow, None, None, None, None, d_ws, wsb, None)
    assert call(h=0) == -1 and b"image size" in lib.dflow_last_error()
    assert call(w=8193) == -1 and b"image size" in lib.dflow_last_error()
    for nn in (0, 257, -5):
        assert call(nn=nn) == -1 and b"nn" in lib.dflow_last_error()
    for k in (0.0, -1.0, float("nan"), float("inf")):
        assert call(k=k) == -1 and b"k=" in lib.dflow_last_error()
    for m in (2, -1):
        assert call(method=m) == -1 and b"method" in lib.dflow_last_error()
    assert call(sparse=None) == -1 and b"d_sparse" in lib.dflow_last_error()
    assert call(edges=None) == -1 and b"d_edges" in lib.dflow_last_error()
    assert call(flow=None) == -1 and b"d_flow" in lib.dflow_last_error()
    assert call(wsb=ws - 1) == -2 and b"workspace" in lib.dflow_last_error()
    assert call(d_ws=None) == -2


def test_python_wrapper_and_cli_reject_bad_input(tmp_path):
    pipeline = pkg("pipeline")
    with pytest.raises(ValueError, match="method"):
        pipeline.epic_interpolate(np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.float32), method="XX")
    ef = pkg("epicflow")
    for argv in (["a", "b", "c", "d"], ["a", "b", "c", "d", "e", "-iter", "5"], ["a", "b", "c", "d", "e", "-nn", "0"],
                 ["a", "b", "c", "d", "e", "-k", "-1"], ["a", "b", "c", "d", "e", "-sintel"], ["a", "b", "c", "d", "e", "-zz"]):
        with pytest.raises(ef.UsageError):
            ef.parse_args(argv)
    assert ef.parse_args(["a", "b", "c", "d", "e", "-nw", "-nn", "7", "-k", "2"]) == (["a", "b", "c", "d", "e"], 7, 2.0, "NW")
    m = tmp_path / "m.txt"
    m.write_text("1 1 3.5 0\n9 9 1 1\n1.4 0.6 2 2\n\n0 0 1 1\n")
    sp = ef.read_matches(str(m), 3, 4)
    assert sp[1, 1].tolist() == [np.float32(2 - 1.4), np.float32(2 - 0.6), 1.0]      # the later line for (1, 1) wins
    assert sp[0, 0].tolist() == [1.0, 1.0, 1.0] and sp[..., 2].sum() == 2
    m.write_text("1 2 3\n")
    with pytest.raises(ef.UsageError):
        ef.read_matches(str(m), 3, 4)
    assert ef.main(["a", "b", "c", "d", "e", "-iter", "5"]) == 2
