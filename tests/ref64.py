"""Independent float64 restatements of the hot path's stages, written from their definitions (DESIGN.md §2 "Parity
unpinned", SURVEY App. A and C, the reference's own lines), not from the oracle or the kernels.

Plain numpy, float64 throughout; nothing here imports the oracle, the package or torch.  The oracle and the HIP kernels
repeat each other operation for operation, so a mistake they share passes every bit-exact test; these functions judge
both from outside, within tolerances derived from float32 error bounds (see each docstring).

Conventions: descriptors (H,W,68); proposals (H,W,L,2) int [dy,dx]; lcosts (H,W,L); nprop, labels (H,W) -- the reference's
own dtypes, as `DiscreteFlow.host_state()` and the oracle hand them out.
"""
import math

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of binary32
U64 = 2.0 ** -53          # unit roundoff of binary64
NDESC = 68

# ------------------------------------------------------------------------------------------------------------------ DAISY


def filter_size(sigma):
    """`size = odd(int(5 sigma)) >= 3` taps."""
    n = int(5.0 * sigma)
    if n % 2 == 0:
        n += 1
    return max(n, 3)


def gaussian_taps(sigma, n=None):
    """n normalised Gaussian taps exp(-x^2 / 2 sigma^2), x = i - (n-1)/2, in float64 (the build rounds them
    to float32 first, the tolerance absorbs that).  n defaults to filter_size(sigma)."""
    n = filter_size(sigma) if n is None else n
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    k = np.exp(-0.5 * x * x / (sigma * sigma))
    return k / k.sum()


def _blur(a, k):
    """Separable blur with replicated borders ("exact border mode of each filter" settled as replicate), rows
    then columns; a is (H,W) or (H,W,C)."""
    r = len(k) // 2
    H, W = a.shape[:2]
    ix = np.clip(np.arange(-r, W + r), 0, W - 1)
    iy = np.clip(np.arange(-r, H + r), 0, H - 1)
    t = sum(k[j] * a[:, ix[j:j + W]] for j in range(len(k)))
    return sum(k[j] * t[iy[j:j + H]] for j in range(len(k)))


def gray(bgr):
    """cv::cvtColor BGR2GRAY on uint8: the 14-bit fixed-point weights (1868, 9617, 4899) with rounding, exact in integers;
    then /255 (SURVEY App. C "BGR->gray, scale to [0,1]")."""
    b = bgr.astype(np.int64)
    g = (1868 * b[..., 0] + 9617 * b[..., 1] + 4899 * b[..., 2] + 8192) >> 14
    return g.astype(np.float64) / 255.0


def daisy_cubes64(bgr):
    """(4,H,W,4) smoothed orientation layers, SURVEY App. C: a 5-tap sigma 0.5 blur (fixed size, not filter_size); central differences x0.5 with replicated
    borders; layers max(0, cos(l 90deg) dx + sin(l 90deg) dy) with exact cos/sin; a blur of sigma sqrt(1.6^2 - 0.5^2);
    then cubes r = 0..3 at sigma 0.625 (r+1), each blurred from the previous one by the incremental sigma."""
    img = _blur(gray(bgr), gaussian_taps(0.5, 5))
    H, W = img.shape
    xp = np.clip(np.arange(W) + 1, 0, W - 1); xm = np.clip(np.arange(W) - 1, 0, W - 1)
    yp = np.clip(np.arange(H) + 1, 0, H - 1); ym = np.clip(np.arange(H) - 1, 0, H - 1)
    dx = (img[:, xp] - img[:, xm]) * 0.5
    dy = (img[yp] - img[ym]) * 0.5
    lay = np.stack([np.maximum(dx, 0), np.maximum(dy, 0), np.maximum(-dx, 0), np.maximum(-dy, 0)], axis=-1)
    lay = _blur(lay, gaussian_taps(math.sqrt(1.6 * 1.6 - 0.25)))
    sig = [0.625 * (r + 1) for r in range(4)]
    cubes, prev = [], lay
    for r in range(4):
        s = sig[0] if r == 0 else math.sqrt(sig[r] ** 2 - sig[r - 1] ** 2)
        prev = _blur(prev, gaussian_taps(s))
        cubes.append(prev)
    return np.stack(cubes)


def daisy_grid(exact=False):
    """17 grid offsets (gy, gx): the centre, then ring r = 0..3 (radius 1.25 (r+1)) at angles a = 0..3 (a 90deg), as
    `(r+1) * 1.25 * (sin, cos)(a * 2pi/4)` in double.  With exact=True the offsets are the
    mathematically exact ones (sin and cos in {0, +-1}) instead of the libm values, whose residues (cos(3pi/2) = -1.8e-16)
    decide the inside test in column 0."""
    gy, gx = [0.0], [0.0]
    for r in range(4):
        for a in range(4):
            s, c = math.sin(a * (2 * math.pi / 4)), math.cos(a * (2 * math.pi / 4))
            if exact:
                s, c = float(round(s)), float(round(c))
            gy.append((r + 1) * 1.25 * s)
            gx.append((r + 1) * 1.25 * c)
    return np.array(gy), np.array(gx)


def daisy64(bgr, exact_grid=False):
    """(H,W,68) float64 DAISY of a uint8 BGR image (DESIGN.md §2 "Parity unpinned"): the histogram of grid
    point k at (y + gy_k, x + gx_k) is the bilinear interpolation of a cube -- the centre reads cube 0, ring r reads cube r.
    A ring point is skipped (zero) unless its float32-cast coordinates lie in [0, W-1) x [0, H-1); any point whose
    truncated coordinates satisfy mnx >= W-2 or mny >= H-2 is zero.  Bilinear weights are the exact products of
    alpha = mnx + 1 - x and beta = mny + 1 - y.  No normalisation."""
    bgr = np.asarray(bgr, np.uint8)
    H, W = bgr.shape[:2]
    cubes = daisy_cubes64(bgr)
    gy, gx = daisy_grid(exact_grid)
    yy0, xx0 = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((H, W, NDESC))
    for k in range(17):
        cube = cubes[0 if k == 0 else (k - 1) // 4]
        yy, xx = yy0 + gy[k], xx0 + gx[k]
        ok = np.ones((H, W), bool)
        if k > 0:
            xf, yf = xx.astype(np.float32), yy.astype(np.float32)
            ok = (xf >= 0) & (xf < np.float32(W - 1)) & (yf >= 0) & (yf < np.float32(H - 1))
        mnx, mny = np.trunc(xx).astype(np.int64), np.trunc(yy).astype(np.int64)
        ok &= (mnx < W - 2) & (mny < H - 2)
        mnx, mny = np.clip(mnx, 0, W - 2), np.clip(mny, 0, H - 2)
        al, be = (mnx + 1 - xx)[..., None], (mny + 1 - yy)[..., None]
        h = (al * be * cube[mny, mnx] + (1 - al) * be * cube[mny, mnx + 1]
             + al * (1 - be) * cube[mny + 1, mnx] + (1 - al) * (1 - be) * cube[mny + 1, mnx + 1])
        out[..., 4 * k:4 * k + 4] = np.where(ok[..., None], h, 0.0)
    return out


DAISY_ATOL = 1.5e-7
"""Absolute bound on |DAISY_f32 - daisy64|, set in tests/test_ref64.py::test_oracle_daisy_within_tolerance from the measured
error of the float32 oracle (3.7e-8 at most over the test images, see there): 4x that.  The error does not scale with the
value: it comes from float32 rounding of the blurred gray image (values <= 1) before the central differences cancel."""


def f16_bound(ref):
    """The DAISY bound for binary16 planes: half an ulp of binary16 at the reference value, plus DAISY_ATOL."""
    a = np.abs(ref) + DAISY_ATOL
    return np.spacing(a.astype(np.float16)).astype(np.float64) / 2 + DAISY_ATOL


# -------------------------------------------------------------------------------------------------------------------- kNN


class Geom:
    """The cell grid of SURVEY Q12: ncellx = W // cellw cells per row, the last cell absorbing the remainder,
    and a query's candidate cells are those within `window` cells of its own (daisy i flann.py:162-168)."""

    def __init__(self, H, W, cellh, cellw, window=2, knn=5, tphi=2.5):
        self.H, self.W, self.ch, self.cw, self.window, self.K, self.tphi = H, W, cellh, cellw, window, knn, tphi
        self.ncx, self.ncy = W // cellw, H // cellh

    def cell_x(self, x):
        return np.minimum(np.asarray(x) // self.cw, self.ncx - 1)

    def cell_y(self, y):
        return np.minimum(np.asarray(y) // self.ch, self.ncy - 1)

    def x_range(self, ci):
        return ci * self.cw, (self.W if ci == self.ncx - 1 else (ci + 1) * self.cw)

    def y_range(self, cj):
        return cj * self.ch, (self.H if cj == self.ncy - 1 else (cj + 1) * self.ch)

    def window_cells(self, y, x):
        """[(ci, cj)] of pixel (y, x) in slot order: ci outer, cj inner (daisy i flann.py:162-163)."""
        cx, cy = int(self.cell_x(x)), int(self.cell_y(y))
        return [(ci, cj) for ci in range(max(0, cx - self.window), min(self.ncx, cx + self.window + 1))
                for cj in range(max(0, cy - self.window), min(self.ncy, cy + self.window + 1))]

    def nknn(self, y, x):
        """Number of kNN labels: K per window cell (daisy i flann.py:189)."""
        cx, cy = self.cell_x(x), self.cell_y(y)
        nx = np.minimum(self.ncx - 1, cx + self.window) - np.maximum(0, cx - self.window) + 1
        ny = np.minimum(self.ncy - 1, cy + self.window) - np.maximum(0, cy - self.window) + 1
        return self.K * nx * ny


L2_C = 72
"""Error constant of the squared-L2 comparisons.  The kernels (and the oracle) compute d_k = fl(a_k - b_k) and the 68-term
chain acc = fmaf(d_k, d_k, acc), every operation rounding once with unit roundoff u = 2^-24.  fl(a - b) = (a - b)(1 + e1)
squares to (a - b)^2 (1 + 2e1 + e1^2), and each fmaf adds at most u of the running sum, so by the standard recursive-sum
bound |fl(D) - D| <= (n + 2) u D + O(u^2) with n = 68 terms: 70 u D, rounded up to 72 u D.  If r was returned and s was not,
fl(D_r) <= fl(D_s), hence D_r - D_s <= 72 u (D_r + D_s); a near-tie inside that margin may go either way."""

L1_C = 72
"""Error constant of the L1 costs: |fl(a-b)| per term (one rounding) summed in float32 in any order of 68 terms (numpy's
pairwise order here): |fl(S) - S| <= (68 + 1) u S, rounded up to 72 u S."""


def _check_groups(d1, d2, geom, proposals, lcosts, ys, xs, g, ci, cj, pixels_ok):
    """Check group g (cell (ci, cj)) of the pixels (ys, xs); returns a list of failure strings."""
    K = geom.K
    x0, x1 = geom.x_range(ci)
    y0, y1 = geom.y_range(cj)
    cw = x1 - x0
    pts = d2[y0:y1, x0:x1].reshape(-1, NDESC).astype(np.float64)
    q = d1[ys, xs].astype(np.float64)
    fl = proposals[ys, xs, K * g:K * g + K]                      # (n, K, 2)
    ty, tx = ys[:, None] + fl[..., 0], xs[:, None] + fl[..., 1]
    bad = []
    inside = (ty >= y0) & (ty < y1) & (tx >= x0) & (tx < x1)
    if not inside.all():
        i = np.argwhere(~inside)[0][0]
        return ["pixel (%d,%d) group %d cell (%d,%d): target outside the cell: %s" % (ys[i], xs[i], g, ci, cj, fl[i].tolist())]
    idx = (ty - y0) * cw + (tx - x0)
    srt = np.sort(idx, axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        i = np.argwhere((srt[:, 1:] == srt[:, :-1]).any(1))[0][0]
        return ["pixel (%d,%d) group %d: repeated candidate %s" % (ys[i], xs[i], g, idx[i].tolist())]
    qq = (q * q).sum(1)
    pp = (pts * pts).sum(1)
    D = np.maximum(qq[:, None] + pp[None, :] - 2.0 * (q @ pts.T), 0.0)
    # float64 evaluation error of D through the norms: 80 * 2^-53 (|q|^2 + |p|^2), far below the float32 margin
    D64err = 80 * U64 * (qq[:, None] + pp[None, :])
    rows = np.arange(len(ys))[:, None]
    Dr = D[rows, idx]
    Er = D64err[rows, idx]
    Dn = D.copy()
    Dn[rows, idx] = np.inf
    if Dn.shape[1] > K:
        s = Dn.argmin(1)
        Ds, Es = Dn[rows[:, 0], s], D64err[rows[:, 0], s]
        worst = Dr.max(1)
        j = Dr.argmax(1)
        slack = L2_C * U32 * (worst + Ds) + Er[rows[:, 0], j] + Es
        viol = worst - Ds > slack
        if viol.any():
            i = np.flatnonzero(viol)[0]
            bad.append("pixel (%d,%d) group %d cell (%d,%d): returned distance %.9g > non-returned %.9g (slack %.3g)"
                       % (ys[i], xs[i], g, ci, cj, worst[i], Ds[i], slack[i]))
    asc = Dr[:, 1:] - Dr[:, :-1]
    sl = L2_C * U32 * (Dr[:, 1:] + Dr[:, :-1]) + Er[:, 1:] + Er[:, :-1]
    if (asc < -sl).any():
        i = np.argwhere((asc < -sl).any(1))[0][0]
        bad.append("pixel (%d,%d) group %d: distances not ascending: %s" % (ys[i], xs[i], g, Dr[i].tolist()))
    L1 = np.abs(q[:, None, :] - d2[ty, tx].astype(np.float64)).sum(-1)
    want = np.minimum(geom.tphi, L1)
    got = lcosts[ys, xs, K * g:K * g + K]
    tol = L1_C * U32 * L1 + 1e-300
    if (np.abs(got - want) > tol).any():
        i, k = np.argwhere(np.abs(got - want) > tol)[0]
        bad.append("pixel (%d,%d) slot %d: lcost %.9g, min(tphi, L1_64) %.9g" % (ys[i], xs[i], K * g + k, got[i, k], want[i, k]))
    return bad


def knn_check(d1, d2, geom, proposals, lcosts, nprop, labels, pixels=None, cells=None, max_fail=5):
    """Check the kNN stage (generisi, daisy i flann.py:157-189) at `pixels` ((ys, xs) arrays, default
    every pixel) against float64 arithmetic on the descriptor planes d1, d2 the stage read:
      * nprop = K x (number of window cells), the window taken on the Q12 grid (last cell absorbs the remainder);
      * group g (slot 5g..5g+4) belongs to the g-th window cell in ci-major order; its K targets p + [dy,dx] lie inside that
        cell and are distinct;
      * under float64 squared L2 the largest returned distance is at most the smallest non-returned one plus the float32
        margin L2_C u (D_r + D_s) (see L2_C), and the K come ascending within that margin;
      * lcost = min(tphi, L1_64) within L1_C u L1_64 (see L1_C);
      * the WTA label is a kNN slot whose cost is the minimum of the kNN costs within the L1 margin (strict '<', Q4: the
        first minimum of the float32 costs, which float64 cannot tell apart from a near-tie).
    `cells` restricts the group checks to candidate cells in that set of (ci, cj).  Returns a list of failure strings."""
    H, W = geom.H, geom.W
    if pixels is None:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pixels = (yy.ravel(), xx.ravel())
    ys, xs = (np.asarray(a, np.int64) for a in pixels)
    bad = []
    nk = geom.nknn(ys, xs)
    if not np.array_equal(nprop[ys, xs], nk):
        i = np.flatnonzero(nprop[ys, xs] != nk)[0]
        bad.append("pixel (%d,%d): nprop %d, want %d" % (ys[i], xs[i], nprop[ys[i], xs[i]], nk[i]))
        return bad
    # pixels in one query cell share their window: check a (query cell, group) pair at a time
    qcx, qcy = geom.cell_x(xs), geom.cell_y(ys)
    for key in sorted(set(zip(qcx.tolist(), qcy.tolist()))):
        sel = np.flatnonzero((qcx == key[0]) & (qcy == key[1]))
        wc = geom.window_cells(geom.y_range(key[1])[0], geom.x_range(key[0])[0])
        for g, (ci, cj) in enumerate(wc):
            if cells is not None and (ci, cj) not in cells:
                continue
            for c0 in range(0, len(sel), 4096):
                s = sel[c0:c0 + 4096]
                bad += _check_groups(d1, d2, geom, proposals, lcosts, ys[s], xs[s], g, ci, cj, None)
                if len(bad) >= max_fail:
                    return bad
    # WTA: the chosen slot's cost is the minimum of the kNN costs (float64 recomputation of every kNN cost)
    if labels is not None:
        lab = labels[ys, xs]
        if (lab < 0).any() or (lab >= nk).any():
            i = np.flatnonzero((lab < 0) | (lab >= nk))[0]
            return bad + ["pixel (%d,%d): WTA label %d outside the kNN slots" % (ys[i], xs[i], lab[i])]
        for i in range(len(ys)) if len(ys) <= 20000 else np.random.default_rng(0).choice(len(ys), 20000, replace=False):
            y, x = ys[i], xs[i]
            n = nk[i]
            t = proposals[y, x, :n]
            L1 = np.abs(d1[y, x].astype(np.float64)[None] - d2[y + t[:, 0], x + t[:, 1]].astype(np.float64)).sum(1)
            c = np.minimum(geom.tphi, L1)
            if c[lab[i]] > c.min() + 2 * L1_C * U32 * L1[lab[i]]:
                bad.append("pixel (%d,%d): WTA label %d cost %.9g, minimum %.9g" % (y, x, lab[i], c[lab[i]], c.min()))
                if len(bad) >= max_fail:
                    break
    return bad


NEIGHBOUR_REACH = 64
"""The sampler's offsets floor(sigma z) come from a 127-entry table, -64..62 (DESIGN.md §2 "RNG"), truncated toward zero
(SURVEY Q7): a sampled neighbour lies within 64 px of the pixel in each coordinate."""


def neighbour_check(d1, d2, geom, proposals, lcosts, nprop, wta, ngauss, pixels, max_fail=5):
    """Check the labels the neighbour stage (nasumicni, daisy i flann.py:205-233) appended after the kNN slots, at `pixels`
    ((ys, xs)); `wta` is the (H,W) WTA label field the stage read.  Per SURVEY Q5-Q7:
      * at most ngauss labels were appended;
      * each appended label v is the WTA flow of some pixel t within NEIGHBOUR_REACH of p, and its cost is
        min(tphi, |sum_k (d1(p)_k - d2(t)_k)|) for such a t -- the absolute value of the SIGNED sum, with image 2 read at the
        sampled neighbour t, not at p + v (Q6) -- within L1_C u sum_k |d1(p)_k - d2(t)_k| (see L1_C);
      * no two appended labels share a component (Q5: the dedupe is component-wise, `tv in proposals[...]`)."""
    H, W = geom.H, geom.W
    F = np.take_along_axis(proposals, wta[..., None, None].astype(np.int64), axis=2)[:, :, 0]      # (H,W,2)
    dd1, dd2 = d1.astype(np.float64), d2.astype(np.float64)
    S1, S2 = dd1.sum(-1), dd2.sum(-1)
    A1, A2 = np.abs(dd1).sum(-1), np.abs(dd2).sum(-1)
    bad = []
    R = NEIGHBOUR_REACH
    for y, x in zip(*pixels):
        nk, n = int(geom.nknn(y, x)), int(nprop[y, x])
        if not 0 <= n - nk <= ngauss:
            bad.append("pixel (%d,%d): %d labels appended, ngauss %d" % (y, x, n - nk, ngauss))
            continue
        app = proposals[y, x, nk:n]
        if n - nk > 1:
            for c in range(2):
                if len(np.unique(app[:, c])) != n - nk:
                    bad.append("pixel (%d,%d): appended labels share a component: %s" % (y, x, app.tolist()))
        y0, y1, x0, x1 = max(0, y - R), min(H, y + R + 1), max(0, x - R), min(W, x + R + 1)
        Fw = F[y0:y1, x0:x1]
        for j, v in enumerate(app):
            ty, tx = np.nonzero((Fw[..., 0] == v[0]) & (Fw[..., 1] == v[1]))
            if len(ty) == 0:
                bad.append("pixel (%d,%d) slot %d: %s is no WTA flow within %d px" % (y, x, nk + j, v.tolist(), R))
                continue
            ty, tx = ty + y0, tx + x0
            want = np.minimum(geom.tphi, np.abs(S1[y, x] - S2[ty, tx]))
            tol = L1_C * U32 * (A1[y, x] + A2[ty, tx]) + 1e-300
            if not (np.abs(lcosts[y, x, nk + j] - want) <= tol).any():
                bad.append("pixel (%d,%d) slot %d: cost %.9g matches no sampled neighbour with flow %s (nearest %.9g)"
                           % (y, x, nk + j, lcosts[y, x, nk + j], v.tolist(), want[np.abs(lcosts[y, x, nk + j] - want).argmin()]))
        if len(bad) >= max_fail:
            break
    return bad


# -------------------------------------------------------------------------------------------------------------------- BCD


def phase_chains(H, W, phase):
    """(ys, xs): (nchains, length) pixel coordinates of the chains of one phase of ceoBCD (python bcd.py:261-284, SURVEY
    Q11), each in the order the chain runs: 0 even columns downwards, 1 even rows leftwards, 2 odd columns (from
    (W//2)*2-1 down) upwards, 3 odd rows (from (H//2)*2-1 down) rightwards."""
    if phase == 0:
        cols = np.arange(0, W, 2)
        return np.broadcast_to(np.arange(H)[None], (len(cols), H)), np.broadcast_to(cols[:, None], (len(cols), H))
    if phase == 1:
        rows = np.arange(0, H, 2)
        return np.broadcast_to(rows[:, None], (len(rows), W)), np.broadcast_to(np.arange(W - 1, -1, -1)[None], (len(rows), W))
    if phase == 2:
        cols = np.arange((W // 2) * 2 - 1, -1, -2)
        return np.broadcast_to(np.arange(H - 1, -1, -1)[None], (len(cols), H)), np.broadcast_to(cols[:, None], (len(cols), H))
    rows = np.arange((H // 2) * 2 - 1, -1, -2)
    return np.broadcast_to(rows[:, None], (len(rows), W)), np.broadcast_to(np.arange(W)[None], (len(rows), W))


def _unary(proposals, lcosts, nprop, labels, ys, xs, vertical, lamda, tpsi):
    """(nc, L) data term of the chain pixels (ys, xs) (nc,) for every label, python bcd.py:107-112, :118-120, :161-162:
    lamda lcost + sidepsi(y+yside, x+xside) + sidepsi(y-yside, x-xside), with (yside, xside) = (1, 0) for a column chain
    and (0, 1) for a row chain -- the side pixels lie ON the chain, before and after the pixel, and sidepsi reads their
    labels from before the phase (bestlabels is written only by the traceback).  sidepsi = min(tpsi, |f_l - f_nb|_1), 0
    outside the image (:84-88).  inf beyond nprop."""
    H, W, L = lcosts.shape
    f = proposals[ys, xs]                                                   # (nc, L, 2)
    u = lamda * lcosts[ys, xs].astype(np.float64)
    for s in (-1, 1):
        ny, nx = (ys + s, xs) if vertical else (ys, xs + s)
        ok = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        nyc, nxc = np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)
        fn = proposals[nyc, nxc, labels[nyc, nxc]]                          # (nc, 2)
        u = u + np.where(ok[:, None], np.minimum(tpsi, np.abs(f - fn[:, None]).sum(-1)), 0)
    return np.where(np.arange(L)[None] < nprop[ys, xs][:, None], u, np.inf)


def chain_psi(proposals, nprop, pys, pxs, ys, xs, tpsi):
    """(nc, L, L) cost psi[k, l] of predecessor label k at (pys, pxs) followed by label l at (ys, xs), as the DP of python
    bcd.py:152-176 charges it: |f_k - f_l|_1 if compatible (tpsi > |f_k - f_l|_1, Q8); if l has no compatible
    predecessor label at all, tpsi (permmincost); otherwise -- l has a compatible predecessor but k is not one -- inf, because
    mincost is overwritten by the minimum over compatible k even when tpsi + min dp is smaller.  So along a chain the DP
    minimises the energy with this psi, which equals min(tpsi, |f_k - f_l|_1) on every pair it can choose, but forbids
    incompatible pairs wherever a compatible one exists."""
    L = proposals.shape[2]
    fk, fl = proposals[pys, pxs].astype(np.int32), proposals[ys, xs].astype(np.int32)
    raz = np.abs(fk[:, :, None, 0] - fl[:, None, :, 0])
    raz += np.abs(fk[:, :, None, 1] - fl[:, None, :, 1])
    comp = (raz < tpsi) & (np.arange(L)[None, :, None] < nprop[pys, pxs][:, None, None])
    psi = np.where(comp, raz.astype(np.float64), np.inf)
    psi[~comp.any(1)[:, None, :].repeat(L, 1)] = float(tpsi)
    return psi


def chain_energies(proposals, lcosts, nprop, labels, chain_labels, phase, lamda=0.05, tpsi=8, chains=None,
                   max_chain_cells=1 << 22):
    """The energy a chain of python bcd.py:101-257 minimises, given the labels `labels` from before the phase:
    sum_i unary_i(l_i) + sum_i psi(l_{i-1}, l_i) (_unary, chain_psi), i running in the chain's direction.  Returns (vmin, e),
    float64 (nchains,) arrays: vmin its minimum over all labellings of each chain of `phase` (a Viterbi vectorised across
    the chains), e its value at the labels of `chain_labels`.

    This is not the image energy sum lamda lcost + sum_{4-adjacent} min(tpsi, |f_p - f_q|_1): the side terms look along the
    chain at its own old labels, not across it at the other parity, and psi forbids incompatible pairs where a compatible
    one exists.  That energy can rise in a phase of the reference algorithm (96x128 synthetic pair, first phase: 25 754 ->
    27 147), so no test asserts its descent."""
    H, W, L = lcosts.shape
    if (nprop < 1).any():
        raise ValueError("every pixel needs a label")
    ys, xs = phase_chains(H, W, phase)
    if chains is not None:
        ys, xs = ys[chains], xs[chains]
    vertical = phase in (0, 2)
    nc, n = ys.shape
    vmin, e = np.empty(nc), np.empty(nc)
    step = max(1, max_chain_cells // (L * L))
    for c0 in range(0, nc, step):
        cy, cx = ys[c0:c0 + step], xs[c0:c0 + step]
        r = np.arange(len(cy))
        u = _unary(proposals, lcosts, nprop, labels, cy[:, 0], cx[:, 0], vertical, lamda, tpsi)
        dp = u
        lab = chain_labels[cy[:, 0], cx[:, 0]]
        ee = u[r, lab]
        for i in range(1, n):
            psi = chain_psi(proposals, nprop, cy[:, i - 1], cx[:, i - 1], cy[:, i], cx[:, i], tpsi)
            u = _unary(proposals, lcosts, nprop, labels, cy[:, i], cx[:, i], vertical, lamda, tpsi)
            dp = (dp[:, :, None] + psi).min(1) + u
            nl = chain_labels[cy[:, i], cx[:, i]]
            ee = ee + psi[r, lab, nl] + u[r, nl]
            lab = nl
        vmin[c0:c0 + step], e[c0:c0 + step] = dp.min(1), ee
    return vmin, e


def bcd_phase_check(proposals, lcosts, nprop, before, after, phase, lamda=0.05, tpsi=8, chains=None, max_fail=5):
    """One phase of ceoBCD (python bcd.py:265-277) took labels `before` to `after`.  Checks: pixels off the phase's chains
    are unchanged; each chain reads only its own line (the side terms lie on the chain, see _unary), so the chains are
    independent and each one's new labels must reach the minimum of its own energy (chain_energies) given `before`,
    within 1e-9 (1 + |E|).  Ties may be broken differently
    from the reference; the energies may not differ.  `chains` (indices) restricts the Viterbi to some chains of the phase.
    Returns failure strings."""
    H, W = before.shape
    ys, xs = phase_chains(H, W, phase)
    on = np.zeros((H, W), bool)
    on[ys, xs] = True
    bad = []
    if not np.array_equal(before[~on], after[~on]):
        bad.append("phase %d changed %d labels off its chains" % (phase, int((before[~on] != after[~on]).sum())))
    if ((after < 0) | (after >= nprop)).any():
        return bad + ["phase %d left labels outside 0..nprop-1" % phase]
    ids = np.arange(len(ys)) if chains is None else np.asarray(chains)
    vmin, e = chain_energies(proposals, lcosts, nprop, before, after, phase, lamda, tpsi, chains=ids)
    viol = ~(np.abs(e - vmin) <= 1e-9 * (1 + np.abs(vmin)))
    for c in np.flatnonzero(viol)[:max_fail]:
        bad.append("phase %d chain %d (starting at (%d,%d)): energy %.12g, Viterbi minimum %.12g"
                   % (phase, ids[c], ys[ids[c], 0], xs[ids[c], 0], e[c], vmin[c]))
    return bad


# ------------------------------------------------------------------------------------------------------ neighbour sampler


def _normal_mass(a, b, sigma):
    """P(a < sigma Z < b), Z standard normal, from tail differences with math.erfc (accurate far out in either tail)."""
    s = sigma * math.sqrt(2.0)
    if a + b >= 0:
        return 0.5 * (math.erfc(a / s) - math.erfc(b / s))           # upper tails
    return 0.5 * (math.erfc(-b / s) - math.erfc(-a / s))             # lower tails


def gauss_offset_law(c, n, sigma):
    """The law of int(c + sigma Z) (daisy i flann.py:219,221: np.random.normal, then int()) for an integer centre c, given
    0 <= value < n, as a float64 (n,) array; returns (law, clip).  int() truncates toward zero, so value 0 takes
    P(-1 < c + sigma Z < 1) and value v >= 1 takes P(v <= c + sigma Z < v + 1).

    The sampler draws floor(sigma Z) from a 127-entry table of offsets -64..62 plus the catch-all 63 (DESIGN.md §2 "RNG"):
    draws with |sigma Z| >= 64 land on -64 or 63 instead.  `clip` = P(|sigma Z| >= 64) = erfc(64 / (sigma sqrt 2)) is the most
    mass that moves: 1.2e-15 at sigma = 8 and smaller below, far under what any sample size here resolves.  The table's
    thresholds are floor(Phi * 2^32), which moves each bin by at most 2^-32 more."""
    p = np.array([_normal_mass(-1 - c, 1 - c, sigma) if v == 0 else _normal_mass(v - c, v + 1 - c, sigma)
                  for v in range(n)])
    return p / p.sum(), math.erfc(64.0 / (sigma * math.sqrt(2.0)))


def normal_upper_quantile(alpha):
    """z with P(Z > z) = alpha, by bisection on math.erfc (no scipy)."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def chi2_upper_quantile(df, alpha):
    """The chi-square quantile with upper tail alpha on df degrees of freedom, by the Wilson-Hilferty approximation
    df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3, z the normal quantile."""
    z = normal_upper_quantile(alpha)
    h = 2.0 / (9.0 * df)
    return df * (1.0 - h + z * math.sqrt(h)) ** 3


def g_test(counts, probs, min_expected=5.0):
    """G statistic 2 sum O ln(O/E) of observed counts against a law (arrays of one shape), after merging: the bins whose
    expected count N p is below min_expected are pooled into one bin, and that bin, if still below, into the smallest of the
    others.  The merge depends on the law alone, never on the counts.  Bins of probability 0 take no part; a count in one
    makes G inf.  Returns (G, degrees of freedom)."""
    O = np.asarray(counts, np.float64).ravel()
    E = O.sum() * np.asarray(probs, np.float64).ravel()
    if (O[E == 0] > 0).any():
        return math.inf, int((E > 0).sum()) - 1
    O, E = O[E > 0], E[E > 0]
    small = E < min_expected
    Ob, Eb = list(O[~small]), list(E[~small])
    if small.any():
        o, e = O[small].sum(), E[small].sum()
        if e < min_expected and Eb:
            j = int(np.argmin(Eb))
            o, e = o + Ob.pop(j), e + Eb.pop(j)
        Ob.append(o)
        Eb.append(e)
    Ob, Eb = np.array(Ob), np.array(Eb)
    k = Ob > 0
    return 2.0 * float((Ob[k] * np.log(Ob[k] / Eb[k])).sum()), len(Ob) - 1


SAMPLER_ALPHA = 1e-6
"""Rejection level of the sampler-law G-tests.  The draws are a fixed function of (seed, pixel, attempt), so a test either
always passes or always fails; the level only sets how far from the law a stream must be before it fails."""


def sampler_state(H, W, maxknn, L):
    """Reference-dtype state (proposals, lcosts, nprop, bestlabels) in which the neighbour stage with ngauss = 1 appends exactly
    the position of its first draw that lands inside the image: every kNN slot 0..maxknn-1 holds (-30000, -30000), whose
    components no position in [0, 8191] shares, so the component-wise duplicate test (`tv in`, daisy i flann.py:226, SURVEY
    Q5) never fires; slot maxknn holds the pixel's own position (y, x) and is its WTA label.  The appended label then lands
    in slot maxknn + 1.  Costs are 0.
    That slot maxknn stays out of the duplicate test's first slice, proposals[broj:broj+K] (:223-226), needs cells of at
    least NEIGHBOUR_REACH px, so that a draw lands at most one cell away, and window >= 1: broj + K then stays at or below
    K (3 + 3 ncellyl) <= 35 < maxknn = 45 at window 1.  (At window 0 the draw one cell down gives broj = K = maxknn.)"""
    proposals = np.full((H, W, L, 2), -1, np.int64)
    proposals[:, :, :maxknn] = -30000
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    proposals[:, :, maxknn, 0] = yy
    proposals[:, :, maxknn, 1] = xx
    lcosts = np.full((H, W, L), 1000.0)
    lcosts[:, :, :maxknn + 1] = 0.0
    nprop = np.full((H, W), maxknn + 1, np.int64)
    return proposals, lcosts, nprop, np.full((H, W), maxknn, np.int64)


def sampler_law_check(draws, sigma, border=16, alpha=SAMPLER_ALPHA):
    """G-tests of the sampled positions `draws` ((H,W,2) [ty, tx], one per pixel) against gauss_offset_law:
      * interior (pixels at least 64 px from every border, where no draw leaves the image): the joint histogram of the
        offsets (ty - y, tx - x) against the product of the offset laws -- which also tests that the two are independent;
      * for each distance d = 0..border-1 from the top and left borders: the rows drawn by the pixels of row d and the columns
        drawn by the pixels of column d, pooled, against gauss_offset_law(d, n, sigma) (with the other coordinate independent,
        its conditioning on landing inside the image does not change this law).  There int() truncation shows: value 0
        takes both sides of the centre line.
    Each test rejects at G > chi2_upper_quantile(df, alpha).  H = W = n is required.  Returns (failures, results), results
    a list of (name, G, df, threshold)."""
    H, W = draws.shape[:2]
    assert H == W, "the border classes pool rows and columns of one length"
    n, R = H, NEIGHBOUR_REACH
    res = []
    off = draws[R:H - R, R:W - R] - np.stack(np.meshgrid(np.arange(R, H - R), np.arange(R, W - R), indexing="ij"), -1)
    q = gauss_offset_law(R, 2 * R, sigma)[0]                         # value R + k  <->  offset k in -64..63
    inside = (off >= -R).all(-1) & (off < R).all(-1)
    hist = np.zeros((2 * R, 2 * R))
    np.add.at(hist, (off[inside][:, 0] + R, off[inside][:, 1] + R), 1)
    G, df = g_test(np.append(hist.ravel(), (~inside).sum()), np.append(np.outer(q, q).ravel(), 0.0))
    res.append(("interior (dy, dx)", G, df))
    for d in range(border):
        vals = np.concatenate([draws[d, :, 0], draws[:, d, 1]])
        cnt = np.bincount(np.clip(vals, -1, n) + 1, minlength=n + 2)                 # bin 0: value -1, bin n + 1: value n
        law = np.concatenate([[0.0], gauss_offset_law(d, n, sigma)[0], [0.0]])      # -1 and n collect impossible values
        G, df = g_test(cnt, law)
        res.append(("distance %d from the top/left border" % d, G, df))
    res = [(name, G, df, chi2_upper_quantile(max(df, 1), alpha)) for name, G, df in res]
    bad = ["sigma %g, %s: G = %.1f on %d df > %.1f" % (sigma, name, G, df, t) for name, G, df, t in res if not G <= t]
    return bad, res
