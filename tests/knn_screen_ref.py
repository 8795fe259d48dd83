"""What the MFMA-screened kNN search (csrc/knn_mfma.hip, csrc/knn_pca.hip) leaves in its workspace, judged against float64
truth computed from the descriptors.  Plain numpy, no GPU.

Two halves:

* the LAYOUT MIRROR: Grid (the cell grid of Geom, the padded tile-position order of the image-2 rows, the list ids) and
  views() (km_ws: the regions of the workspace, each on a 256-byte boundary);
* the CHECKERS: check_basis, check_rows1, check_rows2, check_pairs, check_lists, check_stats.  None of them restates a bound
  formula of the kernels: they read the f16 rows, the records and the event lists as written and compare them with
  y = V x computed in float64 from the descriptor planes and the written basis.  Each returns the smallest slack it found
  per inequality and raises ScreenError(checker, name, detail) at the first row, pair or list that violates one.

Notation as in the header of knn_mfma.hip: x = 64 d (d as the planes store it), V64 = the written basis in float64,
y = V64 x, y_P = y[:40], y_D = y[40:], y~ = the 40 f16 values of a prepared row, eta = 2^-17."""
import numpy as np

NDESC = 68
KM_K, KM_KD, KM_CHUNK, KM_QPW, KM_EVROWS_MAX, KM_HEAVY_CAP = 48, 40, 192, 64, 96, 1 << 20
KM_ALPHA, KM_NORM2_MAX, KM_ETA = 64.0, 30000.0, 2.0 ** -17
KM_Q_ZERO, KM_Q_BAD = 1.0, 2.0
SLOT_N, SLOT_QE, SLOT_EN, SLOT_H, SLOT_S, SLOT_ONE = 40, 41, 42, 43, 45, 46
SENTINEL_H = 60000.0
PCA_SAMPLES, PCA_BLOCKS, PCA_DELTA_MAX = 4096, 16, 2e-6
EVENT_WIDTH = 3e-5
"""A list must hold every candidate whose float64 squared distance is within this relative width of the query's fifth
smallest in the cell (the s of knn_screen_kernel: the rounding of the canonical float32 distance on both sides)."""
SUM64 = 1e-12
"""Allowance for the float64 summation of the checker's own sums, relative to the sum of the absolute products."""

BASIS_ORDER_TOL = 5.2e-14
BASIS_TAIL_TOL = 1.3e-4
"""Tolerances of the two basis-QUALITY checks, both relative to the trace of the sample's second-moment matrix A: the largest
increase between consecutive Rayleigh quotients v_j^T A v_j, and the sample energy in components 40..67 above the sum of the 28
smallest eigenvalues of numpy.linalg.eigh(A).  The iteration is five float32 Jacobi sweeps, so neither is zero, and neither can
be derived: both were MEASURED on the MI355X over the 46 passes of tests/test_gpu_knn_screen_rows.py (five geometries, DAISY,
the adversarial families and the bad-row passes, both storages; table in DESIGN 5.2).
  ordering: negative everywhere (the quotients fall strictly, by 7e-10 .. 9e-6 of the trace at the closest pair) except on
            the rank-1 `constant` passes, where the 67 quotients of the null space are the basis's own non-orthogonality
            squared: worst +2.59e-14 (45 x 70, float32 planes);
  tail:     worst 6.41e-5 (DAISY 11 x 17, binary16 planes), typically 1.4e-5 .. 5e-5; 0 where A = 0.
The constants are twice the worst excess, because the basis depends on a summation order that may legitimately change."""


class ScreenError(AssertionError):
    def __init__(self, checker, name, detail):
        AssertionError.__init__(self, "%s/%s: %s" % (checker, name, detail))
        self.checker, self.name, self.detail = checker, name, detail


def _need(checker, name, ok, where):
    """ok: boolean array; where(i) describes flat index i of the first violation."""
    ok = np.asarray(ok)
    if not ok.all():
        i = int(np.flatnonzero(~ok.ravel())[0])
        raise ScreenError(checker, name, where(i))


def align256(v):
    return (v + 255) & ~255


def km_pad(npts):
    return -(-npts // KM_CHUNK) * KM_CHUNK


def km_ntiles(npts):
    return km_pad(npts) // 32


ROW_OF_BIT = np.array([[4 * h + (r & 3) + 8 * (r >> 2) for r in range(16)] for h in (0, 1)])
"""km_event_cand: bit r of the mask of half-lane h is tile row 4 h + (r & 3) + 8 (r >> 2)."""


def event_cand(h, r, tile, ntiles):
    return (4 * h + (r & 3) + 8 * (r >> 2)) * ntiles + tile


def query_of_lane(qwave, gq, lane):
    return qwave * KM_QPW + gq * 32 + (lane & 31)


class Grid:
    """Geom and KmGeom: cells of cellw x cellh, the last cell of a row or column absorbing the remainder; a query cell's
    candidate cells are those within `window` cells, slot = (ci - imin) * (jmax - jmin + 1) + (cj - jmin)."""

    def __init__(self, H, W, cellh, cellw, window=2):
        self.H, self.W, self.ch, self.cw, self.win = H, W, cellh, cellw, window
        self.ncx, self.ncy = W // cellw, H // cellh
        self.ncells = self.ncx * self.ncy
        self.N = H * W

    def xr(self, ci):
        return ci * self.cw, (self.W if ci == self.ncx - 1 else (ci + 1) * self.cw)

    def yr(self, cj):
        return cj * self.ch, (self.H if cj == self.ncy - 1 else (cj + 1) * self.ch)

    def cell_w(self, ci):
        return self.xr(ci)[1] - self.xr(ci)[0]

    def npts(self, ci, cj):
        return self.cell_w(ci) * (self.yr(cj)[1] - self.yr(cj)[0])

    def max_cell_points(self):
        return self.npts(self.ncx - 1, self.ncy - 1)

    def qwaves(self):
        return -(-self.max_cell_points() // KM_QPW)

    def num_lists(self):
        return self.ncells * self.qwaves() * (2 * self.win + 1) ** 2

    def evrows(self):
        return min(km_ntiles(self.max_cell_points()) + 1, KM_EVROWS_MAX)

    def window(self, qci, qcj):
        return max(0, qci - self.win), min(self.ncx - 1, qci + self.win), max(0, qcj - self.win), min(self.ncy - 1, qcj + self.win)

    def slot(self, qci, qcj, ci, cj):
        imin, imax, jmin, jmax = self.window(qci, qcj)
        return (ci - imin) * (jmax - jmin + 1) + (cj - jmin)

    def window_cells(self, qci, qcj):
        """[(slot, ci, cj)] of the clipped window: the lists the screen writes for a query wave of this cell."""
        imin, imax, jmin, jmax = self.window(qci, qcj)
        return [(self.slot(qci, qcj, ci, cj), ci, cj) for ci in range(imin, imax + 1) for cj in range(jmin, jmax + 1)]

    def list_id(self, qcell, qwave, wslot):
        return (qcell * self.qwaves() + qwave) * (2 * self.win + 1) ** 2 + wslot

    def cell_base(self, ci, cj):
        """km_cell_base: first row of cell (ci, cj) in the image-2 row array."""
        wl, hl = self.cell_w(self.ncx - 1), self.yr(self.ncy - 1)[1] - self.yr(self.ncy - 1)[0]
        rowsum = (self.ncx - 1) * km_pad(self.cw * self.ch) + km_pad(wl * self.ch)
        hj = hl if cj == self.ncy - 1 else self.ch
        return cj * rowsum + ci * km_pad(self.cw * hj)

    def total_rows(self):
        wl, hl = self.cell_w(self.ncx - 1), self.yr(self.ncy - 1)[1] - self.yr(self.ncy - 1)[0]
        return self.cell_base(0, self.ncy - 1) + (self.ncx - 1) * km_pad(self.cw * hl) + km_pad(wl * hl)

    def cell_pixels(self, ci, cj):
        """Flat pixel index of every in-cell index (row-major inside the cell)."""
        (x0, x1), (y0, y1) = self.xr(ci), self.yr(cj)
        return (np.arange(y0, y1)[:, None] * self.W + np.arange(x0, x1)[None, :]).ravel()

    def cand_of_pos(self, ci, cj):
        """The tile-position map: position pos of the padded cell holds candidate (pos & 31) * ntiles + (pos >> 5)."""
        n = self.npts(ci, cj)
        pos = np.arange(km_pad(n))
        return (pos & 31) * km_ntiles(n) + (pos >> 5)

    def cells(self):
        return [(ci, cj) for cj in range(self.ncy) for ci in range(self.ncx)]


def layout(g):
    """km_ws: {region: (byte offset, dtype, shape)} and the end offset; WsCarver puts every region on a 256-byte boundary."""
    N, rows2, nc, nl, er = g.N, g.total_rows(), g.ncells, g.num_lists(), g.evrows()
    regions = [("h1", np.float16, (N, KM_K)), ("h2", np.float16, (rows2, KM_K)), ("qs", np.float32, (N, 2)),
               ("z0", np.float32, (rows2, 2)), ("zflag", np.uint8, (rows2,)), ("ctr", np.int32, ((256 + 4 * nc) // 4,)),
               ("vt", np.float32, (NDESC, NDESC)), ("pca_ws", np.float64, (PCA_BLOCKS, NDESC, NDESC)),
               ("ztop", np.uint32, (nc, 10)), ("ovf", np.int32, (nl, 4)), ("heavy", np.int32, (KM_HEAVY_CAP, 4)),
               ("ev", np.uint32, (nl, 2, er, 64)), ("ev_cnt", np.uint8, (nl, 2, 64))]
    out, off = {}, 0
    for name, dt, shape in regions:
        out[name] = (off, np.dtype(dt), shape)
        off = align256(off + int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize)
    return out, off


class Screen:
    """Views of the workspace bytes: h1, h2, qs, z0, zflag, ctr (the four counters), cell_bad, vt, ztop_idx, ztop_cost, ev,
    ev_cnt."""


def views(g, ws):
    """ws: the workspace as a uint8 array (the first layout(g)[1] bytes are read)."""
    lay, end = layout(g)
    assert ws.dtype == np.uint8 and ws.ndim == 1 and ws.size >= end, (ws.dtype, ws.size, end)
    s = Screen()
    for name, (off, dt, shape) in lay.items():
        n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        setattr(s, name, ws[off:off + n].view(dt).reshape(shape))
    s.cell_bad = s.ctr[64:64 + g.ncells]
    s.ctr = s.ctr[:4]
    s.ztop_idx, s.ztop_cost = s.ztop[:, :5], s.ztop[:, 5:].view(np.float32)
    return s


# ------------------------------------------------------------------------------------------------ float32 pair arithmetic
def canon_sqnorm32(rows):
    """pair_dist(row, 0).l2: the sequential float32 fmaf chain acc = fmaf(r_k, r_k, acc), k = 0..67.  float64 holds the
    product exactly; the sum is rounded to odd in float64 (TwoSum tells which way) so that the rounding to float32 is the
    single rounding of an fmaf."""
    rows = np.asarray(rows, np.float32)
    acc = np.zeros(rows.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for k in range(rows.shape[1]):
            a = rows[:, k].astype(np.float64)
            p, c = a * a, acc.astype(np.float64)
            t = p + c
            bb = t - p
            e = (p - (t - bb)) + (c - bb)
            fix = (e != 0) & np.isfinite(t) & ((t.view(np.int64) & 1) == 0)
            t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
            acc = t.astype(np.float32)
    return acc


def np_l1_32(rows):
    """pair_dist(row, 0).l1(): sum |r_k| in numpy's float32 pairwise order for 68 values (8 running sums, a tree, a tail)."""
    a = np.abs(np.asarray(rows, np.float32))
    with np.errstate(all="ignore"):
        r = a[:, 0:8].copy()
        for i in range(8, 64, 8):
            r = r + a[:, i:i + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
        for i in range(64, NDESC):
            res = res + a[:, i]
    return res


# ------------------------------------------------------------------------------------------------ truth
class Truth:
    """float64 truth of one pass: d1, d2 are the (H,W,68) float32 planes as stored (binary16 storage: already rounded), vt
    the written basis."""

    def __init__(self, g, d1, d2, vt):
        self.g = g
        self.V = np.asarray(vt, np.float64)
        self.d = [np.ascontiguousarray(d, np.float32).reshape(-1, NDESC) for d in (d1, d2)]
        self.x, self.y, self.bad, self.zero, self.n2 = [], [], [], [], []
        with np.errstate(all="ignore"):
            for d in self.d:
                sc = np.float32(KM_ALPHA) * d                                   # exact unless it overflows
                x = sc.astype(np.float64)
                n2 = (x * x).sum(1)
                bad = ~np.isfinite(sc).all(1) | ~(n2 < KM_NORM2_MAX)
                x = np.where(bad[:, None], 0.0, x)
                self.x.append(x); self.y.append(x @ self.V.T); self.bad.append(bad)
                self.zero.append(~bad & (d == 0).all(1)); self.n2.append(np.where(bad, 0.0, n2))
        # image 2 by position: cell, candidate index, pixel (-1: no candidate), removed zero rows
        rows2 = g.total_rows()
        self.pos_pix = np.full(rows2, -1, np.int64)
        self.pos_cell = np.zeros(rows2, np.int64)
        self.pos_cand = np.zeros(rows2, np.int64)
        self.removed_pix = np.zeros(g.N, bool)
        self.cell_bad = np.zeros(g.ncells, bool)
        for ci, cj in g.cells():
            cell, base, n = cj * g.ncx + ci, g.cell_base(ci, cj), g.npts(ci, cj)
            cand, pix = g.cand_of_pos(ci, cj), g.cell_pixels(ci, cj)
            real = cand < n
            self.pos_cell[base:base + len(cand)] = cell
            self.pos_cand[base:base + len(cand)] = cand
            self.pos_pix[base:base + len(cand)][real] = pix[cand[real]]
            self.removed_pix[pix[np.flatnonzero(self.zero[1][pix])[5:]]] = True     # all-zero rows beyond the first five, by index
            self.cell_bad[cell] = self.bad[1][pix].any()
        self.pos_real = self.pos_pix >= 0
        pp = np.maximum(self.pos_pix, 0)
        self.pos_removed = self.pos_real & self.removed_pix[pp]
        self.pos_bad = self.pos_real & self.bad[1][pp]
        self.pos_kept = self.pos_real & ~self.pos_removed & ~self.pos_bad
        self.pos_sentinel = ~self.pos_real | self.pos_removed

    def pos_name(self, i):
        g = self.g
        cell = int(self.pos_cell[i])
        pix = int(self.pos_pix[i])
        return "cell (%d,%d) position %d candidate %d pixel %s" % (cell % g.ncx, cell // g.ncx, i - g.cell_base(cell % g.ncx, cell // g.ncx),
                                                                   self.pos_cand[i], (pix // g.W, pix % g.W) if pix >= 0 else None)

    def pix_name(self, i):
        return "pixel (%d,%d)" % (i // self.g.W, i % self.g.W)


def _norm(a):
    return np.sqrt((a * a).sum(-1))


def _rel_slack(bound, truth):
    """Smallest (bound - truth) / bound over the rows with a positive bound (1.0 if there are none)."""
    m = bound > 0
    return float(((bound[m] - truth[m]) / bound[m]).min()) if m.any() else 1.0


# ------------------------------------------------------------------------------------------------ basis
def sample_second_moment(d2):
    """The float64 second-moment matrix (about the origin) of knn_cov_kernel's sample of the image-2 plane."""
    d = np.asarray(d2, np.float32).reshape(-1, NDESC)
    npix = d.shape[0]
    nsamp = min(npix, PCA_SAMPLES)
    stride = npix // nsamp
    with np.errstate(all="ignore"):
        s = d[np.arange(nsamp) * stride].astype(np.float64)
        s = np.where(np.abs(s) < 1e4, s, 0.0)              # non-finite or absurd values count as 0
    return s.T @ s


def basis_quality(vt, d2):
    """(orthonormality defect, ordering excess, tail excess); the last two relative to trace(A), 0 if A = 0."""
    V = np.asarray(vt, np.float64)
    orth = float(np.linalg.norm(V @ V.T - np.eye(NDESC), 2)) if np.isfinite(V).all() else np.inf
    A = sample_second_moment(d2)
    tr = float(np.trace(A))
    if not tr > 0:
        return orth, 0.0, 0.0
    r = np.einsum("ji,ik,jk->j", V, A, V)
    lam = np.linalg.eigh(A)[0]                             # ascending
    return orth, float(np.max(r[1:] - r[:-1]) / tr), float((r[KM_KD:].sum() - lam[:NDESC - KM_KD].sum()) / tr)


def check_basis(vt, d2):
    orth, order, tail = basis_quality(vt, d2)
    if not orth <= PCA_DELTA_MAX:
        raise ScreenError("basis", "orthonormal", "|V V^T - I|_2 = %.3g > %.3g" % (orth, PCA_DELTA_MAX))
    if not order <= BASIS_ORDER_TOL:
        raise ScreenError("basis", "order", "a Rayleigh quotient rises by %.3g of the trace (tolerance %.3g)" % (order, BASIS_ORDER_TOL))
    if not tail <= BASIS_TAIL_TOL:
        raise ScreenError("basis", "tail", "components 40..67 hold %.3g of the trace more than the 28 smallest eigenvalues (tolerance %.3g)"
                          % (tail, BASIS_TAIL_TOL))
    return dict(orthonormal=PCA_DELTA_MAX - orth, order=order, tail=tail)


# ------------------------------------------------------------------------------------------------ rows of image 1
def check_rows1(s, t):
    ck, name = "rows1", t.pix_name
    flag, hq = s.qs[:, 0], s.qs[:, 1].astype(np.float64)
    want = np.where(t.bad[0], KM_Q_BAD, np.where(t.zero[0], KM_Q_ZERO, 0.0)).astype(np.float32)
    _need(ck, "flag", flag == want, lambda i: "%s: qs.x = %g, want %g" % (name(i), flag[i], want[i]))
    ok = ~t.bad[0]
    y, r = t.y[0], s.h1.astype(np.float64)
    yt = r[:, :KM_KD]
    out = {}
    with np.errstate(all="ignore"):
        for nm, bound, truth in (("hq_y", hq, 0.5 * (y * y).sum(1)), ("hq_x", hq, 0.5 * t.n2[0]),
                                 ("slot40", -r[:, SLOT_N], _norm(y[:, KM_KD:])),
                                 ("slot41", -r[:, SLOT_QE] * 64.0, _norm(yt)),
                                 ("slot42", -r[:, SLOT_EN] / 64.0, _norm(yt - y[:, :KM_KD]))):
            _need(ck, nm, ~ok | (bound >= truth), lambda i: "%s: bound %.9g < truth %.9g" % (name(i), bound[i], truth[i]))
            out[nm] = _rel_slack(bound[ok], truth[ok])
    fixed = np.array([-1.0, -1.0, -(2.0 ** -12), 0.0, 0.0])
    _need(ck, "fixed_slots", ~ok[:, None] | (r[:, SLOT_H:] == fixed[None, :]),
          lambda i: "%s slot %d: %g, want %g" % (name(i // 5), SLOT_H + i % 5, r[i // 5, SLOT_H + i % 5], fixed[i % 5]))
    return out


# ------------------------------------------------------------------------------------------------ rows of image 2
def check_rows2(s, t):
    g, ck, name = t.g, "rows2", t.pos_name
    r = s.h2.astype(np.float64)
    sent = np.zeros(KM_K)
    sent[SLOT_H] = SENTINEL_H
    is_sent = (r == sent[None, :]).all(1)
    _need(ck, "sentinel", t.pos_real | is_sent, lambda i: "%s: a position without a candidate does not hold the sentinel row" % name(i))
    z0 = s.z0
    _need(ck, "sentinel_z0", t.pos_real | ((z0[:, 0] == np.inf) & (z0[:, 1] == 0) & (s.zflag == 0)),
          lambda i: "%s: z0 = %s zflag = %d" % (name(i), z0[i], s.zflag[i]))
    pp = np.maximum(t.pos_pix, 0)
    zero = t.pos_real & t.zero[1][pp]
    _need(ck, "zflag", (s.zflag != 0) == zero, lambda i: "%s: zflag = %d, all-zero row: %s" % (name(i), s.zflag[i], zero[i]))
    _need(ck, "zero_removed", ~t.pos_removed | is_sent, lambda i: "%s: an all-zero row beyond the first five of its cell stayed a candidate" % name(i))
    _need(ck, "zero_kept", ~t.pos_kept | ~is_sent, lambda i: "%s: a real candidate was replaced by the sentinel row" % name(i))
    _need(ck, "cell_bad", (s.cell_bad != 0) == t.cell_bad,
          lambda i: "cell (%d,%d): cell_bad = %d, holds a bad row: %s" % (i % g.ncx, i // g.ncx, s.cell_bad[i], t.cell_bad[i]))
    k = t.pos_kept
    y = t.y[1][pp]
    yt, y_p = r[:, :KM_KD], y[:, :KM_KD]
    h12 = r[:, SLOT_H] + r[:, SLOT_H + 1]
    out = {}
    with np.errstate(all="ignore"):
        for nm, bound, truth in (("slot40", r[:, SLOT_N], _norm(y[:, KM_KD:])),
                                 ("slot41", r[:, SLOT_QE] / 64.0, _norm(yt - y_p) + KM_ETA * _norm(yt)),
                                 ("slot42", r[:, SLOT_EN] * 64.0, _norm(y_p)),
                                 ("slot45", r[:, SLOT_S] / 4096.0, np.abs(0.5 * (y * y).sum(1) - h12)
                                  + KM_ETA * (np.abs(r[:, SLOT_H]) + np.abs(r[:, SLOT_H + 1])))):
            _need(ck, nm, ~k | (bound >= truth), lambda i: "%s: bound %.9g < truth %.9g" % (name(i), bound[i], truth[i]))
            out[nm] = _rel_slack(bound[k], truth[k])
    _need(ck, "slot46_47", ~k[:, None] | (r[:, SLOT_ONE:] == 1.0), lambda i: "%s: slot %d = %g, want 1" % (name(i // 2), SLOT_ONE + i % 2, r[i // 2, SLOT_ONE + i % 2]))
    # z0: what an all-zero query computes for the row (canonical float32 squared norm, numpy-order L1)
    d = t.d[1][pp]
    nb = t.pos_real & ~t.pos_bad
    l2, l1 = canon_sqnorm32(d), np_l1_32(d)
    _need(ck, "z0_l2", ~nb | (z0[:, 0] == l2), lambda i: "%s: z0.x = %.9g, canonical |c|^2 = %.9g" % (name(i), z0[i, 0], l2[i]))
    _need(ck, "z0_l1", ~nb | (z0[:, 1] == l1), lambda i: "%s: z0.y = %.9g, numpy-order |c|_1 = %.9g" % (name(i), z0[i, 1], l1[i]))
    # ztop: the five smallest (z0.x, index) of the cell with their costs
    for ci, cj in g.cells():
        cell = cj * g.ncx + ci
        if t.cell_bad[cell]:
            continue                                        # the lists against a bad cell go to the exact search: ztop is not read
        pix = g.cell_pixels(ci, cj)
        cl2, cl1 = canon_sqnorm32(t.d[1][pix]), np_l1_32(t.d[1][pix])
        order = np.lexsort((np.arange(len(pix)), cl2))[:5]
        if not (np.array_equal(s.ztop_idx[cell], order) and np.array_equal(s.ztop_cost[cell], cl1[order])):
            raise ScreenError(ck, "ztop", "cell (%d,%d): ztop = %s %s, want %s %s" % (ci, cj, s.ztop_idx[cell], s.ztop_cost[cell], order, cl1[order]))
    return out


# ------------------------------------------------------------------------------------------------ pair sandwich
def check_pairs(s, t):
    """Every query against every position of every cell of its window: P1 + eta A <= tau <= P2 - eta A for real candidates,
    both values at -60000 for sentinel positions, every real value above -50000.  Returns the smallest slack of each side
    (in units of the MFMA value) and the number of pairs judged."""
    g, ck = t.g, "pairs"
    out = dict(lower=np.inf, upper=np.inf, floor=np.inf, pairs=0)
    h1, h2 = s.h1.astype(np.float64), s.h2.astype(np.float64)
    flipped = [SLOT_N, SLOT_QE, SLOT_EN, SLOT_S]
    ycc = 0.5 * (t.y[1] * t.y[1]).sum(1)
    for qci, qcj in g.cells():
        qpix = g.cell_pixels(qci, qcj)
        qpix = qpix[~t.bad[0][qpix]]                        # the rows of bad queries are not judged (their lists are 255)
        Q, Yq = h1[qpix], t.y[0][qpix]
        assert not Q[:, SLOT_ONE:].any()                    # check_rows1: slots 46, 47 are 0 as stored, and P2 leaves them there
        Qa, Qf = np.abs(Q), 2.0 * Q[:, flipped]
        for _, ci, cj in g.window_cells(qci, qcj):
            base, npad = g.cell_base(ci, cj), km_pad(g.npts(ci, cj))
            for kind, sel in (("real", t.pos_kept[base:base + npad]), ("sentinel", t.pos_sentinel[base:base + npad])):
                pos = base + np.flatnonzero(sel)
                if not len(pos) or not len(qpix):
                    continue
                C = h2[pos]
                P1, A = Q @ C.T, Qa @ np.abs(C).T
                P2 = P1 - Qf @ C[:, flipped].T               # the query's slots 40, 41, 42 and 45 negated
                out["pairs"] += P1.size
                if kind == "sentinel":
                    ok = (P1 <= -SENTINEL_H) & (P2 <= -SENTINEL_H) & (KM_ETA * A <= 0.5)
                    names = ("sentinel_value",)
                else:
                    cp = t.pos_pix[pos]
                    tau = Yq @ t.y[1][cp].T - ycc[cp][None, :]
                    A *= KM_ETA - SUM64
                    lo, hi, fl = tau - P1, P2 - tau, P1 + 50000.0
                    lo -= A; hi -= A; fl -= A
                    ok = (lo >= 0) & (hi >= 0) & (fl > 0)
                    names = ("lower", "upper", "real_floor")
                    out["lower"], out["upper"], out["floor"] = min(out["lower"], float(lo.min())), min(out["upper"], float(hi.min())), min(out["floor"], float(fl.min()))
                if not ok.all():
                    i = int(np.flatnonzero(~ok.ravel())[0])
                    q, c = i // len(pos), i % len(pos)
                    vals = dict(P1=P1[q, c], P2=P2[q, c])
                    nm = names[0]
                    if kind == "real":
                        vals.update(tau=tau[q, c], eta_A=A[q, c])
                        nm = "lower" if lo[q, c] < 0 else "upper" if hi[q, c] < 0 else "real_floor"
                    raise ScreenError(ck, nm, "query %s, %s: %s" % (t.pix_name(qpix[q]), t.pos_name(pos[c]), vals))
    return out


# ------------------------------------------------------------------------------------------------ event lists
def _fifth(D, counts):
    """Fifth smallest of every row of D, column j counting counts[j] times (counts None: once each)."""
    if D.shape[1] <= 5:
        i5 = np.broadcast_to(np.arange(D.shape[1]), D.shape)
    else:
        i5 = np.argpartition(D, 4, axis=1)[:, :5]           # the fifth smallest is among the five smallest columns
    v5 = np.take_along_axis(D, i5, 1)
    o = np.argsort(v5, axis=1, kind="stable")
    v5 = np.take_along_axis(v5, o, 1)
    if counts is None:
        return v5[:, -1]
    k5 = (np.cumsum(counts[np.take_along_axis(i5, o, 1)], axis=1) >= 5).argmax(1)
    return v5[np.arange(D.shape[0]), k5]


def required(xq, xc):
    """[nq, nc] bool: the candidates whose float64 squared distance to the query is within EVENT_WIDTH (relative) of the
    query's fifth smallest.  Equal candidate rows are folded first (tied cells stay cheap); the distances that decide come
    from the differences themselves, the expansion through the norms only picks which ones to compute."""
    U, inv = np.unique(xc, axis=0, return_inverse=True)
    inv = inv.ravel()
    if len(U) == len(xc):
        U, inv, counts = xc, None, None
    else:
        counts = np.bincount(inv, minlength=len(U))
        assert counts.sum() >= 5
    qq, uu = (xq * xq).sum(1), (U * U).sum(1)
    D = xq @ U.T
    D *= -2.0
    D += qq[:, None]
    D += uu[None, :]
    emax = 1e-13 * (qq + uu.max())                          # error of the expansion, per query, over its candidates
    poss = D <= ((_fifth(D, counts) + emax) * (1.0 + EVENT_WIDTH) + emax)[:, None]
    qi, ui = np.nonzero(poss)
    D.fill(np.inf)
    for c0 in range(0, len(qi), 1 << 18):
        a, b = qi[c0:c0 + (1 << 18)], ui[c0:c0 + (1 << 18)]
        df = xq[a] - U[b]
        D[a, b] = (df * df).sum(1)
    req = D <= (_fifth(D, counts) * (1.0 + EVENT_WIDTH))[:, None]
    return req if inv is None else req[:, inv]


def check_lists(s, t, oracle_proposals=None):
    """Every list the screen writes.  oracle_proposals: (H,W,L,2) [dy,dx] of the canonical search (slot 5 wslot + j), whose
    five per cell must be in the list too.  Returns the totals dflow_knn_screen_stats reports."""
    g, ck = t.g, "lists"
    er = g.evrows()
    tot = dict(entries=0, events=0, max_entries_per_lane=0, lists_exact=0, lists_checked=0)
    lanes = np.arange(64)
    half, col = lanes >> 5, lanes & 31
    for qci, qcj in g.cells():
        qcell, qpix, qn = qcj * g.ncx + qci, g.cell_pixels(qci, qcj), g.npts(qci, qcj)
        xq = t.x[0][qpix]
        for wslot, ci, cj in g.window_cells(qci, qcj):
            cell, cpix, cn, nt = cj * g.ncx + ci, g.cell_pixels(ci, cj), g.npts(ci, cj), km_ntiles(g.npts(ci, cj))
            (cx0, _), (cy0, _), ccw = g.xr(ci), g.yr(cj), g.cell_w(ci)
            req = None
            removed = t.removed_pix[cpix]
            for qwave in range(-(-qn // KM_QPW)):
                lid = g.list_id(qcell, qwave, wslot)
                lname = "list %d (query cell (%d,%d) wave %d, cell (%d,%d))" % (lid, qci, qcj, qwave, ci, cj)
                qi = np.minimum(qwave * KM_QPW + np.arange(KM_QPW), qn - 1)      # lanes past the cell shadow its last query
                pix = qpix[qi]
                cnt = s.ev_cnt[lid].astype(np.int64)                             # [gq, lane]
                tot["lists_checked"] += 1
                if t.bad[0][pix].any() or t.cell_bad[cell]:
                    _need(ck, "bad_list_count", cnt == 255, lambda i: "%s holds a bad query or cell: count %d of group %d lane %d" % (lname, cnt.ravel()[i], i // 64, i % 64))
                    tot["lists_exact"] += 1
                    continue
                _need(ck, "unexpected_255", cnt != 255, lambda i: "%s: group %d lane %d reports 255" % (lname, i // 64, i % 64))
                _need(ck, "count", cnt <= er - 1, lambda i: "%s: count %d > %d" % (lname, cnt.ravel()[i], er - 1))
                E = s.ev[lid]                                                    # [gq, entry, lane]
                valid = np.arange(er)[None, :, None] < cnt[:, None, :]
                tile, mask = (E >> 16).astype(np.int64), (E & 0xFFFF).astype(np.int64)
                ename = lambda i: "%s: group %d entry %d lane %d = 0x%08x" % (lname, i // (64 * er), i // 64 % er, i % 64, E.ravel()[i])
                _need(ck, "empty_mask", ~valid | (mask != 0), ename)
                inc = np.ones_like(valid)
                inc[:, 1:] = ~valid[:, 1:] | (tile[:, 1:] > tile[:, :-1])
                _need(ck, "tile_order", inc, ename)
                M = np.zeros((KM_QPW, km_pad(cn)), bool)
                gqs, es, ls = np.nonzero(valid)
                ev_mask, ev_tile = mask[gqs, es, ls], tile[gqs, es, ls]
                nev = 0
                for r in range(16):
                    b = (ev_mask >> r & 1) != 0
                    cand = ROW_OF_BIT[half[ls[b]], r] * nt + ev_tile[b]
                    qslot = gqs[b] * 32 + col[ls[b]]
                    nev += int(b.sum())
                    if (cand >= cn).any():
                        i = int(np.flatnonzero(cand >= cn)[0])
                        raise ScreenError(ck, "candidate_range", "%s: group %d lane %d tile %d bit %d names candidate %d of %d"
                                          % (lname, gqs[b][i], ls[b][i], ev_tile[b][i], r, cand[i], cn))
                    if removed[cand].any():
                        i = int(np.flatnonzero(removed[cand])[0])
                        raise ScreenError(ck, "removed_candidate", "%s: group %d lane %d names the removed all-zero row %d" % (lname, gqs[b][i], ls[b][i], cand[i]))
                    M[qslot, cand] = True
                M = M[:, :cn]
                qz = t.zero[0][pix]
                zl = qz[(np.arange(2)[:, None] * 32 + col[None, :])]               # [gq, lane]: the lane's query is all zero
                _need(ck, "zero_query_events", ~zl | (cnt == 0), lambda i: "%s: group %d lane %d (all-zero query) has %d entries" % (lname, i // 64, i % 64, cnt.ravel()[i]))
                if req is None:
                    req = required(xq, t.x[1][cpix]) & ~removed[None, :]
                miss = req[qi] & ~M & ~qz[:, None]
                if miss.any():
                    q, c = np.argwhere(miss)[0]
                    raise ScreenError(ck, "missing_neighbour", "%s: query %s: candidate %d within %g of the fifth smallest distance is not in the list"
                                      % (lname, t.pix_name(pix[q]), c, EVENT_WIDTH))
                if oracle_proposals is not None:
                    py, px = pix // g.W, pix % g.W
                    fl = oracle_proposals[py, px, 5 * wslot:5 * wslot + 5]           # [64, 5, 2]
                    oc = (py[:, None] + fl[..., 0] - cy0) * ccw + (px[:, None] + fl[..., 1] - cx0)
                    got = M[np.arange(KM_QPW)[:, None], oc] | qz[:, None]
                    if not got.all():
                        q, j = np.argwhere(~got)[0]
                        raise ScreenError(ck, "missing_neighbour", "%s: query %s: candidate %d, number %d of the canonical search, is not in the list"
                                          % (lname, t.pix_name(pix[q]), oc[q, j], j))
                tot["entries"] += int(cnt.sum())
                tot["events"] += nev
                tot["max_entries_per_lane"] = max(tot["max_entries_per_lane"], int(cnt.max()))
    return tot


def check_stats(s, t, tot, stats):
    """The totals of check_lists and the row counts against dflow_knn_screen_stats (which also proves that the mirror reads the
    bytes the kernels wrote) and against the counters in the control block."""
    g = t.g
    pp = np.maximum(t.pos_pix, 0)
    want = dict(entries=tot["entries"], events=tot["events"], max_entries_per_lane=tot["max_entries_per_lane"],
                lists_exact=tot["lists_exact"], lists=g.num_lists(), list_capacity=g.evrows(),
                zero_queries=int(t.zero[0].sum()), bad_queries=int(t.bad[0].sum()),
                zero_candidates=int((t.pos_real & t.zero[1][pp]).sum()), zero_candidates_removed=int(t.pos_removed.sum()))
    got = {k: stats[k] for k in want}
    if got != want:
        raise ScreenError("stats", "totals", "dflow_knn_screen_stats %s, the mirror %s" % (got, want))
    if int(s.ctr[0]) != want["lists_exact"] or int(s.ctr[1]) != stats["flags"]:
        raise ScreenError("stats", "counters", "ctr = %s, stats %s" % (s.ctr.tolist(), stats))
    return want


def check_all(g, ws, d1, d2, stats=None, oracle_proposals=None):
    """All checkers on one pass; returns {checker: result}."""
    s = views(g, ws)
    out = dict(basis=check_basis(s.vt, d2))
    t = Truth(g, d1, d2, s.vt)
    out["rows1"] = check_rows1(s, t)
    out["rows2"] = check_rows2(s, t)
    out["pairs"] = check_pairs(s, t)
    out["lists"] = check_lists(s, t, oracle_proposals)
    if stats is not None:
        out["stats"] = check_stats(s, t, out["lists"], stats)
    return out
