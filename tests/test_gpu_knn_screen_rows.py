"""What knn_jacobi_kernel, knn_prep_kernel, knn_cell_post_kernel and knn_screen_kernel WRITE, judged by tests/knn_screen_ref.py
against float64 truth: the basis, the bound factors of every prepared row, the sandwich w <= tau <= v of every (query,
candidate position) pair of every window, and every event list.  The other kNN tests compare the final five proposals; a bound
that is too small changes those only when the violating pair is one of the five nearest.

Every case poisons the workspace and the outputs, runs one screened pass, requires flags == 0 and the predicted number of lists
handed to the exact search, and lets no row, pair or list out of the checks.  Run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

import knn_screen_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "f16")
# (H, W, cellh, cellw): the smallest shapes that reach each path
G_TINY = (11, 17, 2, 3)            # 187 px < 4096 samples; one-chunk cells, mostly sentinel positions, window clipped on all sides
G_SINGULAR = (8, 8, 4, 4)          # 64 px < 68 dimensions: singular second-moment matrix, tied tail eigenvalues
G_RAGGED = (45, 70, 7, 9)          # ragged last row and column; up to 3 query waves per cell
G_CHUNKS = (40, 48, 20, 24)        # cells of 480 points: 3 chunks, 18 tiles, 8 query waves per cell
G_STRIDE = (64, 200, 32, 40)       # 12800 px: sample stride 3; cells of 1280 points
GEOMETRIES = (G_TINY, G_SINGULAR, G_RAGGED, G_CHUNKS, G_STRIDE)

CASES = ([("daisy", g) for g in GEOMETRIES]
         + [(f, G_RAGGED) for f in ("mixed_scale", "tiny", "subnormal", "quantised", "constant", "zero_image2", "zero_block", "near_max")]
         + [(f, G_CHUNKS) for f in ("mixed_scale", "constant", "zero_block")]
         + [("constant", G_SINGULAR), ("zero_image2", G_SINGULAR), ("quantised", G_TINY), ("zero_block", G_TINY)])
BAD_GEOMETRIES = (G_RAGGED, G_CHUNKS, G_STRIDE)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


_daisy = {}


def daisy_pair(O, synth, geom):
    """Real DAISY of a synthetic pair through the oracle, once per geometry (never modified: the families work on copies)."""
    if geom not in _daisy:
        H, W = geom[:2]
        img1, img2, _ = synth.make_pair(H, W, seed=H + W)
        _daisy[geom] = (O.daisy(img1), O.daisy(img2))
    return _daisy[geom]


def family(name, d1, d2, geom):
    """The adversarial families of test_knn_mfma_screen_is_exact_on_hard_descriptors, here judged at the level of the bounds."""
    H, W, ch, cw = geom
    d1, d2 = d1.copy(), d2.copy()
    rng = np.random.default_rng(len(name) + H)
    if name == "mixed_scale":                    # rows scaled by 1e-4 next to rows of full scale
        for d in (d1, d2):
            d[rng.random((H, W)) < 0.5] *= np.float32(1e-4)
    elif name == "tiny":                         # 64 d in and below the f16 subnormal range
        d1, d2 = d1 * np.float32(1e-6), d2 * np.float32(1e-6)
    elif name == "subnormal":
        d1, d2 = d1 * np.float32(1e-9), d2 * np.float32(1e-9)
    elif name == "quantised":                    # a coarse grid: many exactly equal distances
        d1, d2 = np.round(d1 * 64) / 64, np.round(d2 * 64) / 64
    elif name == "constant":                     # every candidate row equal: rank 1, every distance ties
        d2[:] = d2[H // 2, W // 2].copy()
        assert d2.any()
    elif name == "zero_image2":                  # A = 0
        d2[:] = 0
    elif name == "zero_block":                   # all-zero rows in both images: whole cells and more than five in others
        d1[:ch + 3, :cw + 2] = 0
        d2[:ch + 3, :cw + 2] = 0
    elif name == "near_max":                     # rows just under KM_NORM2_MAX (also after the rounding to binary16: 2^-10 of it)
        for d in (d1, d2):
            m = (rng.random((H, W)) < 0.05) & d.any(-1)
            n2 = (d[m].astype(np.float64) ** 2).sum(1) * 4096.0
            d[m] = (d[m] * np.sqrt(29900.0 / n2)[:, None]).astype(np.float32)
    elif name != "daisy":
        raise KeyError(name)
    return d1.astype(np.float32), d2.astype(np.float32)


def new_pass(geom, storage):
    L = pkg("_lib")
    H, W, ch, cw = geom
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=0, flags=L.FLAG_DESCR_F16 if storage == "f16" else 0)


def screened_pass(df, d1, d2):
    """One generisi on (d1, d2) with workspace and outputs poisoned first (as tests/test_gpu_knn_fallbacks.py does) ->
    (workspace bytes, statistics, the planes as stored, widened to float32)."""
    df.set_descriptors(d1, d2)
    df.ws.fill_(1)
    df.proposals.fill_(0x7FFF7FFF)
    df.lcosts.fill_(float("nan"))
    df.nprop.fill_(-1)
    df.bestlabels.fill_(-1)
    df.generisi()
    ws = df.ws.cpu().numpy()
    stats = df.knn_stats()
    return ws, stats, df.descriptors_f32(0).cpu().numpy(), df.descriptors_f32(1).cpu().numpy()


def judge(O, geom, ws, stats, d1s, d2s, case, storage, lists_exact=0):
    """flags, lists_exact, then every checker; prints the measured figures before anything is asserted."""
    H, W, ch, cw = geom
    g = R.Grid(H, W, ch, cw)
    s = R.views(g, ws)
    orth, order, tail = R.basis_quality(s.vt, d2s)
    print(json.dumps(dict(case=case, geom=geom, storage=storage, basis_orth=orth, basis_order=order, basis_tail=tail, stats=stats)))
    assert stats["flags"] == 0, stats
    assert stats["lists_exact"] == lists_exact, stats
    O.set_threads(16)
    try:
        props = O.knn_proposals(O.make_params(H, W, ch, cw), d1s, d2s)[0]
    finally:
        O.set_threads(1)
    out = R.check_all(g, ws, d1s, d2s, stats=stats, oracle_proposals=props)
    print(json.dumps(dict(case=case, geom=geom, storage=storage, **{k: out[k] for k in ("rows1", "rows2", "pairs", "lists")})))
    # nothing was left out: every query against every position of every cell of its window, every written list
    want_pairs = sum(g.npts(qci, qcj) * R.km_pad(g.npts(ci, cj)) for qci, qcj in g.cells() for _, ci, cj in g.window_cells(qci, qcj))
    want_lists = sum(-(-g.npts(qci, qcj) // R.KM_QPW) * len(g.window_cells(qci, qcj)) for qci, qcj in g.cells())
    t = R.Truth(g, d1s, d2s, s.vt)
    if lists_exact:                              # the pairs of a bad row are the only ones not judged: count them
        for qci, qcj in g.cells():
            nbq = int(t.bad[0][g.cell_pixels(qci, qcj)].sum())
            for _, ci, cj in g.window_cells(qci, qcj):
                nbc = int(t.pos_bad[g.cell_base(ci, cj):g.cell_base(ci, cj) + R.km_pad(g.npts(ci, cj))].sum())
                want_pairs -= nbq * R.km_pad(g.npts(ci, cj)) + (g.npts(qci, qcj) - nbq) * nbc
    else:
        assert not t.bad[0].any() and not t.pos_bad.any()
    assert out["lists"]["lists_checked"] == want_lists, (out["lists"], want_lists)
    assert out["pairs"]["pairs"] == want_pairs, (out["pairs"], want_pairs)
    return g, s, t, out


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case,geom", CASES, ids=["%s_%dx%d" % (c, g[0], g[1]) for c, g in CASES])
def test_rows_pairs_and_lists_hold_against_float64(torch_, oracle, synth, case, geom, storage):
    d1, d2 = family(case, *daisy_pair(oracle, synth, geom), geom)
    df = new_pass(geom, storage)
    ws, stats, d1s, d2s = screened_pass(df, d1, d2)
    g, s, t, out = judge(oracle, geom, ws, stats, d1s, d2s, case, storage)
    assert stats["bad_queries"] == 0 and not t.cell_bad.any()
    if case == "zero_block":
        assert stats["zero_candidates_removed"] > 0 and stats["zero_queries"] > 0
        assert any(t.zero[1][g.cell_pixels(ci, cj)].all() for ci, cj in g.cells())          # at least one cell is all zero
    if case == "zero_image2" or (case == "subnormal" and storage == "f16"):
        assert stats["zero_candidates"] == g.N and np.array_equal(s.vt, np.eye(68, dtype=np.float32))
    if case == "near_max":
        assert (t.n2[1] > 29850.0).sum() > 20 and (t.n2[0] > 29850.0).sum() > 20
    if case == "mixed_scale":
        n = np.sqrt(t.n2[1][t.n2[1] > 0])
        assert n.max() / n.min() > 1e3


def bad_pixels(geom):
    """(inf query, NaN candidate, over-range query): the NaN on a pixel the basis samples (index a multiple of the stride)."""
    H, W, ch, cw = geom
    stride = max(1, H * W // R.PCA_SAMPLES)
    p_inf, p_nan, p_over = (ch // 2, cw // 2), (H // 2, W // 2 - (H // 2 * W + W // 2) % stride), (H - 2, W - 3)
    assert (p_nan[0] * W + p_nan[1]) % stride == 0 and (p_nan[0] * W + p_nan[1]) // stride < R.PCA_SAMPLES
    return p_inf, p_nan, p_over


def predicted_bad_lists(g, p_inf, p_nan, p_over):
    """List ids that must report 255: every window slot of the wave of a bad query, and the slot of the bad cell in every wave
    of every query cell that sees it.  Worked out here from the grid alone, not from the checker's truth."""
    lids = set()
    for y, x in (p_inf, p_over):
        qci, qcj = min(x // g.cw, g.ncx - 1), min(y // g.ch, g.ncy - 1)
        qi = (y - qcj * g.ch) * g.cell_w(qci) + (x - qci * g.cw)
        lids |= {g.list_id(qcj * g.ncx + qci, qi // 64, wslot) for wslot, _, _ in g.window_cells(qci, qcj)}
    bci, bcj = min(p_nan[1] // g.cw, g.ncx - 1), min(p_nan[0] // g.ch, g.ncy - 1)
    for qci, qcj in g.cells():
        if abs(qci - bci) <= g.win and abs(qcj - bcj) <= g.win:
            lids |= {g.list_id(qcj * g.ncx + qci, w, g.slot(qci, qcj, bci, bcj)) for w in range(-(-g.npts(qci, qcj) // 64))}
    return lids, (bci, bcj)


def test_predicted_bad_lists_of_the_ragged_geometry():
    """The prediction itself, by hand (no GPU needed, kept next to the case): 45 x 70 in 7 x 9 cells.  inf at (3,4): cell (0,0),
    one wave, a 3 x 3 window = 9 lists.  Over-range at (43,67): the last cell (16 x 10), query 8 * 16 + 13 = 141 = wave 2, 9
    lists.  NaN at (22,35): cell (3,3), seen by the 25 query cells (1..5, 1..5), one wave each except the five of the last cell
    row (9 x 10 = 90 points: two waves): 30 lists."""
    g = R.Grid(*G_RAGGED)
    p_inf, p_nan, p_over = bad_pixels(G_RAGGED)
    assert (p_inf, p_nan, p_over) == ((3, 4), (22, 35), (43, 67))
    lids, cell = predicted_bad_lists(g, p_inf, p_nan, p_over)
    assert cell == (3, 3) and len(lids) == 9 + 9 + 30
    assert g.list_id(41, 2, 0) in lids and g.list_id(41, 1, 0) not in lids


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("geom", BAD_GEOMETRIES, ids=["%dx%d" % g[:2] for g in BAD_GEOMETRIES])
def test_rows_outside_the_screen_flag_exactly_their_lists(torch_, oracle, synth, geom, storage):
    """One inf and one over-range row among the queries, one NaN among the candidates (on a pixel the basis samples: the
    covariance kernel must count it as 0, flags stays 0): exactly those two queries are KM_Q_BAD, exactly that cell is cell_bad,
    exactly the predicted lists report 255 -- all 128 counts of each -- and every other row, pair and list holds as usual."""
    d1, d2 = (d.copy() for d in daisy_pair(oracle, synth, geom))
    p_inf, p_nan, p_over = bad_pixels(geom)
    d1[p_inf][5], d2[p_nan][0], d1[p_over][:] = np.inf, np.nan, 0.4            # 68 * (64 * 0.4)^2 = 44564 >= KM_NORM2_MAX
    g = R.Grid(*geom)
    lids, bad_cell = predicted_bad_lists(g, p_inf, p_nan, p_over)
    df = new_pass(geom, storage)
    ws, stats, d1s, d2s = screened_pass(df, d1, d2)
    g, s, t, out = judge(oracle, geom, ws, stats, d1s, d2s, "bad_rows", storage, lists_exact=len(lids))
    assert stats["bad_queries"] == 2
    assert sorted(np.flatnonzero(s.qs[:, 0] == R.KM_Q_BAD).tolist()) == sorted(y * g.W + x for y, x in (p_inf, p_over))
    assert np.flatnonzero(s.cell_bad).tolist() == [bad_cell[1] * g.ncx + bad_cell[0]]
    for qci, qcj in g.cells():
        for w in range(-(-g.npts(qci, qcj) // 64)):
            for wslot, _, _ in g.window_cells(qci, qcj):
                lid = g.list_id(qcj * g.ncx + qci, w, wslot)
                c = s.ev_cnt[lid]
                assert (c == 255).all() if lid in lids else not (c == 255).any(), (lid, qci, qcj, w, wslot)


@pytest.mark.parametrize("storage", STORAGES)
def test_two_calls_leave_identical_basis_and_rows(torch_, oracle, synth, storage):
    """The comments of knn_pca.hip claim a deterministic basis (fixed summation order): two calls on the same input must leave
    byte-identical vt, h1 and h2, from differently poisoned workspaces."""
    geom = G_STRIDE                               # 16 partial matrices, 50 blocks of rows
    d1, d2 = daisy_pair(oracle, synth, geom)
    g = R.Grid(*geom)
    df = new_pass(geom, storage)
    got = []
    for poison in (1, 0xEE):
        df.set_descriptors(d1, d2)
        df.ws.fill_(poison)
        df.generisi()
        s = R.views(g, df.ws.cpu().numpy())
        got.append((s.vt.copy(), s.h1.copy(), s.h2.copy()))
    for a, b, name in zip(got[0], got[1], ("vt", "h1", "h2")):
        assert a.tobytes() == b.tobytes(), name
