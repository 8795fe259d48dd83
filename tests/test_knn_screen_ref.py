"""tests/knn_screen_ref.py must be able to fail (no GPU).

A numpy restatement of knn_prep_kernel, knn_cell_post_kernel and the event test of knn_screen_kernel writes a workspace in the
kernels' layout (restating the kernels is fine HERE: it only makes fixtures for the checkers, which restate nothing).  The
checkers must pass on it, and each mutation below, one at a time, must draw a NAMED failure from the checker it belongs to.
The fixture is chosen so that every term of the bounds is needed somewhere: a basis whose orthonormality defect is just
inside PCA_DELTA_MAX (so the 3e-6 h of S_c is needed), queries inside the span of the dropped axes (so KM_RHO |x| is what
covers the float32 rotation), tiny and f16-subnormal rows, rows just under KM_NORM2_MAX, more than five all-zero rows in a cell."""
import ctypes as C

import numpy as np
import pytest

import knn_screen_ref as R
from conftest import pkg

GEOMETRIES = {(11, 17, 2, 3): (4800, 625, 7), (8, 8, 4, 4): (768, 100, 7), (45, 70, 7, 9): (8064, 3150, 7),
              (40, 48, 20, 24): (2304, 800, 19), (64, 200, 32, 40): (13440, 5000, 43)}
"""(H, W, cellh, cellw) of tests/test_gpu_knn_screen_rows.py -> (image-2 rows, lists, entries per lane), worked out by hand:
e.g. 45 x 70 in cells of 7 x 9 is 7 x 6 cells, the largest 16 x 10 = 160 points = 3 query waves, every cell padded to one
chunk of 192: 42 * 192 rows, 42 * 3 * 25 lists, 6 tiles + 1 entries."""

KM_RHO, S_DELTA = 2.65e-5, 3e-6
S_SLOPE = 3.5e-5
"""The width of the event test in the fixture's screen, relative to hq - a5 = half the fifth smallest squared distance in y:
what R.EVENT_WIDTH asks for in x, (1 + 3e-5) (1 + delta) / (1 - delta) - 1 = 3.4e-5 with delta = PCA_DELTA_MAX, rounded up."""


def f16_up(v):
    return np.float16(np.float32(np.asarray(v, np.float64) * 1.001 + 1e-7))


def f16_plain(v):
    return np.float16(np.float32(np.asarray(v, np.float64)))


def prep(g, d, vt, which, mut):
    """knn_prep_kernel for the rows d ([n,68] float32) -> ([n,48] f16, bad, zero, 0.5 |x|^2 rounded up)."""
    with np.errstate(all="ignore"):
        x32 = np.float32(64.0) * d
        x = x32.astype(np.float64)
        sxall = (x * x).sum(1)
        bad = ~np.isfinite(x32).all(1) | ~(sxall < R.KM_NORM2_MAX)
        zero = sxall == 0.0
        y = (x32 @ vt[:R.KM_KD].T).astype(np.float32)                  # the float32 rotation (any summation order is allowed)
        hv = y.astype(np.float16)
        f, yd = hv.astype(np.float64), y.astype(np.float64)
        ss, sx, se = (f * f).sum(1), (yd * yd).sum(1), ((f - yd) ** 2).sum(1)
        rx, ry = np.sqrt(sxall), np.sqrt(sx)
        rho = 0.0 if mut == "no_rho" else KM_RHO
        en = np.sqrt(se) + rho * rx
        ypl, ypu = np.maximum(0.0, ry - KM_RHO * rx), ry + KM_RHO * rx
        nd = np.sqrt(np.maximum(0.0, sxall * (1.0 + 1.1 * R.PCA_DELTA_MAX) - ypl * ypl))
        row = np.zeros((len(d), R.KM_K), np.float16)
        row[:, :R.KM_KD] = hv
        if which == 0:
            v41 = np.sqrt(ss) / 64.0
            up41 = f16_up(v41)
            if mut == "plain_rounding_q":                                # plain rounding on the rows where that rounds down
                pl = f16_plain(v41)
                up41 = np.where(pl.astype(np.float64) < v41, pl, up41)
            row[:, 40], row[:, 41], row[:, 42] = -f16_up(nd), -up41, -f16_up(en * 64.0)
            row[:, 43], row[:, 44], row[:, 45] = -1.0, -1.0, -(2.0 ** -12)
            hq = (0.5 * sxall * (1.0 + 1.5 * R.PCA_DELTA_MAX) * 1.0000002).astype(np.float32)
            return row, bad, zero, hq
        hh = 0.5 * sxall
        p1 = f16_plain(hh)
        p2 = f16_plain(hh - p1.astype(np.float64))
        hres = np.abs(hh - p1.astype(np.float64) - p2.astype(np.float64))
        scs = (R.KM_ETA * 1.001 * hh + (0.0 if mut == "no_delta_h" else S_DELTA) * hh + hres) * 1.0004
        v42 = ypu / 64.0
        up42 = f16_up(v42)
        if mut == "plain_rounding_c":
            pl = f16_plain(v42)
            up42 = np.where(pl.astype(np.float64) < v42, pl, up42)
        row[:, 40] = f16_up(nd) * np.float16(0.5 if mut == "half_slot40" else 1.0)
        row[:, 41], row[:, 42] = f16_up((en + R.KM_ETA * np.sqrt(ss)) * 64.0), up42
        row[:, 43], row[:, 44], row[:, 45], row[:, 46], row[:, 47] = p1, p2, f16_up(scs * 4096.0), 1.0, 1.0
    return row, bad, zero, None


def sentinel_row():
    r = np.zeros(R.KM_K, np.float16)
    r[R.SLOT_H] = R.SENTINEL_H
    return r


def write_workspace(g, d1, d2, vt, mut=None):
    """The workspace a pass would leave, and the totals its statistics would report."""
    lay, end = R.layout(g)
    ws = np.ones(end, np.uint8)                                           # regions nobody writes hold garbage
    s = R.views(g, ws)
    s.ctr[:] = 0
    s.cell_bad[:] = 0
    s.vt[:] = vt
    D1, D2 = d1.reshape(-1, 68), d2.reshape(-1, 68)
    s.h1[:], bad1, zero1, hq = prep(g, D1, vt, 0, mut)
    s.qs[:, 0] = np.where(bad1, 2.0, np.where(zero1, 1.0, 0.0))
    s.qs[:, 1] = hq
    for ci, cj in g.cells():
        cell, base, n = cj * g.ncx + ci, g.cell_base(ci, cj), g.npts(ci, cj)
        pix, cand = g.cell_pixels(ci, cj), g.cand_of_pos(ci, cj)
        rows, bad, zero, _ = prep(g, D2[pix], vt, 1, mut)
        zrank = np.cumsum(zero) - 1
        keep_extra = mut == "extra_zero_row" and zero.sum() > 5
        gone = zero & (zrank >= (6 if keep_extra else 5))
        if keep_extra:
            mut = None                                                    # once
        h2 = np.tile(sentinel_row(), (len(cand), 1))
        real = cand < n
        h2[real] = np.where(gone[cand[real], None], sentinel_row()[None, :], rows[cand[real]])
        s.h2[base:base + len(cand)] = h2
        z0 = np.zeros((len(cand), 2), np.float32)
        z0[:, 0] = np.inf
        z0[real, 0], z0[real, 1] = R.canon_sqnorm32(D2[pix])[cand[real]], R.np_l1_32(D2[pix])[cand[real]]
        s.z0[base:base + len(cand)] = z0
        zf = np.zeros(len(cand), np.uint8)
        zf[real] = zero[cand[real]]
        s.zflag[base:base + len(cand)] = zf
        s.cell_bad[cell] = int(bad.any())
        order = np.lexsort((np.arange(n), R.canon_sqnorm32(D2[pix])))[:5]
        s.ztop_idx[cell], s.ztop_cost[cell] = order, R.np_l1_32(D2[pix])[order]
    # the screen, with an exact accumulator: w = P1, v = P2; a5 = the fifth largest w; events v >= th'
    er = g.evrows()
    tot = dict(entries=0, events=0, max_entries_per_lane=0, lists_exact=0)
    h1, h2 = s.h1.astype(np.float64), s.h2.astype(np.float64)
    flip = np.ones(R.KM_K)
    flip[[40, 41, 42, 45]] = -1.0
    for qci, qcj in g.cells():
        qcell, qpix, qn = qcj * g.ncx + qci, g.cell_pixels(qci, qcj), g.npts(qci, qcj)
        for wslot, ci, cj in g.window_cells(qci, qcj):
            cell, base, npad = cj * g.ncx + ci, g.cell_base(ci, cj), R.km_pad(g.npts(ci, cj))
            C = h2[base:base + npad]
            for qwave in range(-(-qn // 64)):
                lid = g.list_id(qcell, qwave, wslot)
                pix = qpix[np.minimum(qwave * 64 + np.arange(64), qn - 1)]
                if bad1[pix].any() or s.cell_bad[cell]:
                    s.ev_cnt[lid] = 255
                    tot["lists_exact"] += 1
                    continue
                Q = h1[pix]
                w, v = Q @ C.T, (Q * flip) @ C.T
                a5 = -np.partition(-w, 4, axis=1)[:, 4]
                hqv = s.qs[pix, 1].astype(np.float64)
                th = np.maximum(a5 - S_SLOPE * np.maximum(hqv - a5, 0.0) - 1e-6 * (np.abs(a5) + S_SLOPE * hqv), -55000.0)
                th = np.where(zero1[pix], 60000.0, th)
                ev = v >= (th - 1e-5 * np.abs(th) - 6e-8)[:, None]           # [query slot, position]
                cnt = np.zeros((2, 64), np.int64)
                E = np.zeros((2, er, 64), np.uint32)
                for ql, pos in zip(*np.nonzero(ev)):
                    tile, row = pos >> 5, pos & 31
                    h, r = (row >> 2) & 1, (row & 3) + 4 * (row >> 3)
                    gq, lane = ql >> 5, h * 32 + (ql & 31)
                    k = cnt[gq, lane]
                    if k and (E[gq, k - 1, lane] >> 16) == tile:
                        E[gq, k - 1, lane] |= np.uint32(1 << r)
                    else:
                        E[gq, k, lane] = np.uint32((tile << 16) | (1 << r))
                        cnt[gq, lane] += 1
                s.ev[lid], s.ev_cnt[lid] = E, cnt
                tot["entries"] += int(cnt.sum()); tot["events"] += int(ev.sum())
                tot["max_entries_per_lane"] = max(tot["max_entries_per_lane"], int(cnt.max()))
    s.ctr[0] = tot["lists_exact"]
    return ws, tot


def make_basis(d2):
    """eigh of the kernel's own sample, rounded to float32; the leading axis stretched by 8e-7 so that |V V^T - I| = 1.6e-6: a
    basis the orthonormality check accepts, on which a row along that axis has 0.5 |y|^2 = h (1 + 1.6e-6)."""
    lam, U = np.linalg.eigh(R.sample_second_moment(d2))
    vt = U[:, ::-1].T.copy()
    vt[0] *= 1.0 + 8e-7
    return vt.astype(np.float32)


@pytest.fixture(scope="module")
def fx():
    g = R.Grid(12, 15, 5, 6)                       # 2 x 2 cells: 30, 45, 42 and 63 points, every cell in every window
    rng = np.random.default_rng(5)
    mix = np.linalg.qr(rng.standard_normal((68, 68)))[0]
    spec = 0.2 * np.exp(-np.arange(68) / 6.0)

    def plane():
        return np.abs((rng.standard_normal((g.N, 68)) * spec) @ mix).astype(np.float32).reshape(g.H, g.W, 68)
    d1, d2 = plane(), plane()
    for d in (d1, d2):
        d[0, 6:9] *= 1e-6                          # tiny rows, f16-subnormal after the scaling by 64
        d[1, 6:9] *= 1e-9
        d[6:8, 0:4] = 0.0                          # eight all-zero rows in cell (0,1), three more than stay candidates
        d[11, 14] *= np.float32(np.sqrt(29990.0 / 4096.0) / np.linalg.norm(d[11, 14].astype(np.float64)))   # just under KM_NORM2_MAX
        d[3, 10] = np.round(d[3, 10] * 64) / 64    # quantised
    vt = make_basis(d2)
    # queries inside the span of the dropped axes: y_P is nothing but the float32 rotation's rounding
    d1[2, 2], d1[4, 12], d1[9, 3] = 2.0 * vt[50], 1.3 * vt[45] - 0.9 * vt[60], 0.7 * vt[67]
    d1[10, 10] = 0.6 * vt[0]                       # and one along the stretched axis
    d2[10, 10] = 0.6 * vt[0]
    vt = make_basis(d2)
    return g, d1, d2, vt


def run_checks(g, ws, d1, d2, tot, oracle_proposals=None):
    out = R.check_all(g, ws, d1, d2, oracle_proposals=oracle_proposals)
    for k in tot:
        assert out["lists"][k] == tot[k], (k, out["lists"], tot)
    return out


def oracle_proposals(O, g, d1, d2):
    return O.knn_proposals(O.make_params(g.H, g.W, g.ch, g.cw), d1, d2)[0]


def test_checkers_pass_on_the_restated_kernels(fx, oracle):
    g, d1, d2, vt = fx
    ws, tot = write_workspace(g, d1, d2, vt)
    out = run_checks(g, ws, d1, d2, tot, oracle_proposals(oracle, g, d1, d2))
    print(out)
    t = R.Truth(g, d1, d2, vt)
    assert t.pos_removed.sum() == 3 and t.zero[0].sum() == 8 and not t.bad[0].any() and not t.bad[1].any()
    assert out["pairs"]["pairs"] == g.N * sum(R.km_pad(g.npts(ci, cj)) for ci, cj in g.cells())     # nothing left out
    assert out["lists"]["lists_checked"] == 4 * 4 and out["lists"]["events"] >= 5 * (g.N - 8) * 4
    assert all(v >= 0 for k in ("rows1", "rows2") for v in out[k].values()), out


def test_checkers_pass_with_bad_rows(fx):
    """inf in a query, NaN and an over-range row in candidates: the flags, cell_bad and the 255 lists are predicted from the
    descriptors, the remaining rows, pairs and lists are judged as usual."""
    g, d1, d2, vt = fx
    d1, d2 = d1.copy(), d2.copy()
    d1[1, 1, 5], d2[8, 12, 0], d2[0, 14] = np.inf, np.nan, 0.5
    ws, tot = write_workspace(g, d1, d2, make_basis(d2))
    out = run_checks(g, ws, d1, d2, tot)
    # query cell (0,0) has one wave: its 4 lists; cells (1,0) and (1,1) are bad: 2 lists of each of the other 3 query cells
    assert out["lists"]["lists_exact"] == 4 + 3 * 2


MUTATIONS = [("half_slot40", "rows2", {"slot40"}), ("no_rho", "rows1", {"slot42"}), ("plain_rounding_q", "rows1", {"slot41"}),
             ("plain_rounding_c", "rows2", {"slot42"}), ("no_delta_h", "rows2", {"slot45"}), ("extra_zero_row", "rows2", {"zero_removed"}),
             ("sentinel_swapped", "rows2", {"sentinel"}), ("vt_rows_exchanged", "basis", {"order"}), ("vt_row_scaled", "basis", {"orthonormal"}),
             ("event_beyond_cell", "lists", {"candidate_range"}), ("neighbour_deleted", "lists", {"missing_neighbour"})]


@pytest.mark.parametrize("mut,checker,names", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught_by_its_checker(fx, oracle, mut, checker, names):
    g, d1, d2, vt = fx
    ws, _ = write_workspace(g, d1, d2, vt, mut)
    s = R.views(g, ws)
    props = oracle_proposals(oracle, g, d1, d2)
    if mut == "sentinel_swapped":                  # cell (1,1): 63 points in 192 positions; position 20 (row 20 of tile 0) is empty, 3 is real
        b = g.cell_base(1, 1)
        assert g.cand_of_pos(1, 1)[20] >= 63 > g.cand_of_pos(1, 1)[3]
        s.h2[[b + 3, b + 20]] = s.h2[[b + 20, b + 3]]
    elif mut == "vt_rows_exchanged":
        s.vt[[3, 44]] = s.vt[[44, 3]]
    elif mut == "vt_row_scaled":
        s.vt[7] *= np.float32(1.0 + 1e-5)
    elif mut == "event_beyond_cell":               # bit 15 of half-lane 1 = row 31 = candidate 31 * 6 + tile >= 63
        lid = g.list_id(3, 0, g.slot(1, 1, 1, 1))
        if s.ev_cnt[lid, 0, 40] == 0:
            s.ev[lid, 0, 0, 40], s.ev_cnt[lid, 0, 40] = 0, 1
        s.ev[lid, 0, 0, 40] |= 1 << 15
    elif mut == "neighbour_deleted":               # the nearest neighbour of pixel (2,8) (cell (1,0), query 20 of wave 0) in cell (0,0)
        y, x, ci, cj = 2, 8, 0, 0
        ql = (y - 0) * g.cell_w(1) + (x - 6)
        wslot = g.slot(1, 0, ci, cj)
        dy, dx = props[y, x, 5 * wslot]
        cand = (y + dy) * g.cell_w(ci) + (x + dx)
        nt = R.km_ntiles(g.npts(ci, cj))
        row, tile = cand // nt, cand % nt
        h, r = (row >> 2) & 1, (row & 3) + 4 * (row >> 3)
        assert R.event_cand(h, r, tile, nt) == cand
        lid, lane = g.list_id(1, 0, wslot), h * 32 + ql
        n = int(s.ev_cnt[lid, 0, lane])
        e = [int(v) for v in s.ev[lid, 0, :n, lane]]
        k = [v >> 16 for v in e].index(tile)
        assert e[k] >> r & 1
        e[k] &= ~(1 << r)
        if e[k] & 0xFFFF == 0:                     # no empty masks: the entry goes
            del e[k]
        s.ev[lid, 0, :len(e), lane] = e
        s.ev_cnt[lid, 0, lane] = len(e)
    with pytest.raises(R.ScreenError) as ei:
        R.check_all(g, ws, d1, d2, oracle_proposals=props)
    assert ei.value.checker == checker and ei.value.name in names, str(ei.value)


def test_stats_mismatch_is_reported(fx):
    g, d1, d2, vt = fx
    ws, tot = write_workspace(g, d1, d2, vt)
    s, t = R.views(g, ws), R.Truth(g, d1, d2, vt)
    lists = R.check_lists(s, t)
    stats = dict(lists, lists=g.num_lists(), list_capacity=g.evrows(), zero_queries=8, bad_queries=0, zero_candidates=8,
                 zero_candidates_removed=3, flags=0)
    R.check_stats(s, t, lists, stats)
    with pytest.raises(R.ScreenError) as ei:
        R.check_stats(s, t, lists, dict(stats, events=stats["events"] + 1))
    assert (ei.value.checker, ei.value.name) == ("stats", "totals")


def test_float32_pair_arithmetic_matches_the_oracle(oracle):
    """canon_sqnorm32 and the (distance, index) order it gives are those of the canonical search for an all-zero query."""
    rng = np.random.default_rng(2)
    pts = (rng.standard_normal((500, 68)) * np.exp(rng.uniform(-12, 1, (500, 1)))).astype(np.float32)
    pts[100], pts[7] = pts[3], 0.0
    idx, dist = oracle.knn_points(np.zeros(68, np.float32), pts, 5)
    l2 = R.canon_sqnorm32(pts)
    order = np.lexsort((np.arange(500), l2))[:5]
    assert np.array_equal(idx, order) and np.array_equal(dist, l2[order])
    assert np.array_equal(R.np_l1_32(pts), np.array([np.sum(np.absolute(r)) for r in pts], np.float32))
    for i in rng.integers(0, 500, 40):             # every row against the oracle's chain, one by one
        assert oracle.knn_points(np.zeros(68, np.float32), pts[i:i + 1], 1)[1][0] == l2[i]


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_mirror_arithmetic(geom):
    H, W, ch, cw = geom
    g = R.Grid(H, W, ch, cw)
    assert (g.total_rows(), g.num_lists(), g.evrows()) == GEOMETRIES[geom]
    # the cells tile the row array without gaps, in cell order
    at = 0
    for ci, cj in g.cells():
        assert g.cell_base(ci, cj) == at
        cand = g.cand_of_pos(ci, cj)
        assert np.array_equal(np.sort(cand[cand < g.npts(ci, cj)]), np.arange(g.npts(ci, cj)))
        at += R.km_pad(g.npts(ci, cj))
    assert at == g.total_rows()
    L = pkg("_lib")
    for flags in (0, L.FLAG_DESCR_F16):
        p = L.default_params(H, W, ch, cw, flags=flags)
        assert int(L.lib().dflow_workspace_bytes(C.byref(p))) >= R.layout(g)[1]


def test_event_decode_and_lane_queries():
    assert R.km_pad(1) == 192 and R.km_pad(192) == 192 and R.km_pad(193) == 384 and R.km_ntiles(480) == 18
    rows = sorted(R.event_cand(h, r, 0, 1) for h in (0, 1) for r in range(16))
    assert rows == list(range(32))
    assert R.event_cand(1, 5, 7, 18) == (4 + 1 + 8) * 18 + 7 and np.array_equal(R.ROW_OF_BIT[1, 5], 13)
    assert R.query_of_lane(3, 1, 45) == 3 * 64 + 32 + 13
    g = R.Grid(45, 70, 7, 9)
    assert g.window(0, 5) == (0, 2, 3, 5) and g.slot(0, 5, 2, 4) == 2 * 3 + 1 and len(g.window_cells(3, 3)) == 25
    assert g.list_id(41, 2, 24) == g.num_lists() - 1
