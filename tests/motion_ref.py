"""dflow_motion_fit restated (include/dflow.h, "Robust global-motion fit"): Philox, the draws, the float64 minimal solves and the
polish solve in plain Python floats and ints (IEEE doubles, exact integers), the float32 score, the keys and the apply step in
np.float32 arithmetic in the written order.  And the fields the tests fit: planted affine maps and homographies with outliers,
holes, NaN / inf / huge vectors and an exclude mask, an all-bad field, a collinear one, two planted motions."""
import numpy as np

F = np.float32
AFFINE, HOMOGRAPHY = 0, 1
UVV, DYDX = 0, 1
CHUNK = 2048                      # FIT_CHUNK of csrc/fit_common.h: the scored pixels a block stages
ATTEMPTS = 16
PIVOT_MIN = 2.0 ** -40
POLISH_RANGE = F(32768.0)
M32 = 0xFFFFFFFF
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
COUNTS = ("scored", "inliers", "degenerate", "best_round", "best_j", "best_count", "accepted", "skipped")


def philox(c0, c1, k0, k1):
    """Word 0 of Philox4x32-10 with counter (c0, c1, 0, 0) and key (k0, k1)."""
    c2 = c3 = 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0


def as_layout(flow, layout):
    """A (h,w,3) [U,V,valid] field in the given layout: DYDX is (h,w,2) [dy,dx], every pixel valid."""
    return flow if layout == UVV else np.ascontiguousarray(flow[..., [1, 0]])


class Field:
    """The planes of a flow field that the fit looks at, flat, in float32."""

    def __init__(self, flow, exclude=None, step=1):
        h, w = flow.shape[:2]
        self.h, self.w, self.n = h, w, h * w
        if flow.shape[2] == 3:
            U, V, valid = flow[..., 0], flow[..., 1], flow[..., 2] > 0.5
        else:
            U, V, valid = flow[..., 1], flow[..., 0], np.ones((h, w), bool)
        ys, xs = np.mgrid[0:h, 0:w]
        self.U, self.V = U.reshape(-1).astype(F), V.reshape(-1).astype(F)
        self.good = (valid & np.isfinite(U) & np.isfinite(V)).reshape(-1)
        self.excluded = np.zeros(self.n, bool) if exclude is None else (np.asarray(exclude).reshape(-1) != 0)
        self.part = self.good & ~self.excluded
        self.xf, self.yf = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
        with np.errstate(all="ignore"):
            self.tx, self.ty = self.xf + self.U, self.yf + self.V
        self.on_grid = ((ys % step == 0) & (xs % step == 0)).reshape(-1)
        self.scored = np.flatnonzero(self.part & self.on_grid)


def project(m, xf, yf):
    with np.errstate(all="ignore"):
        return (m[0] * xf + m[1] * yf) + m[2], (m[3] * xf + m[4] * yf) + m[5], (m[6] * xf + m[7] * yf) + m[8]


def inlier(m, xf, yf, tx, ty, thresh):
    """INLIER of the float32 model m, on float32 scalars or arrays."""
    X, Y, W = project(m, xf, yf)
    with np.errstate(all="ignore"):
        ex, ey, t = X - W * tx, Y - W * ty, thresh * W
        return (W > 0) & (ex * ex + ey * ey <= t * t)


def scored_inliers(fd, m, thresh, at=None):
    at = fd.scored if at is None else at
    return at[inlier(m, fd.xf[at], fd.yf[at], fd.tx[at], fd.ty[at], thresh)]


def gauss(A, n, nrhs):
    """ELIMINATION: A is a list of n rows of n + nrhs Python floats -> nrhs solutions, or None for a small pivot."""
    for c in range(n):
        piv, best = c, abs(A[c][c])
        for r in range(c + 1, n):
            if abs(A[r][c]) > best:
                piv, best = r, abs(A[r][c])
        if not best >= PIVOT_MIN:
            return None
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, n):
            f = A[r][c] / A[c][c]
            for k in range(c + 1, n + nrhs):
                A[r][k] = A[r][k] - f * A[c][k]
    xs = []
    for q in range(nrhs):
        x = [0.0] * n
        for r in range(n - 1, -1, -1):
            t = A[r][n + q]
            for k in range(r + 1, n):
                t = t - A[r][k] * x[k]
            x[r] = t / A[r][r]
        xs.append(x)
    return xs


def normalisation(h, w):
    P = 1.0
    while P < max(h, w):
        P *= 2.0
    return (w - 1) * 0.5, (h - 1) * 0.5, 1.0 / P, P


def minimal_model(h, w, model, pts):
    """The float32 model through the points [(xf, yf, tx, ty)] (np.float32 each), or None when it is degenerate."""
    cx, cy, s, P = normalisation(h, w)
    c = [((float(x) - cx) * s, (float(y) - cy) * s, (float(tx) - cx) * s, (float(ty) - cy) * s) for x, y, tx, ty in pts]
    if model == AFFINE:
        sol = gauss([[a, b, 1.0, p, q] for a, b, p, q in c], 3, 2)
        if sol is None:
            return None
        N = [sol[0], sol[1], [0.0, 0.0, 1.0]]
    else:
        A = []
        for a, b, p, q in c:
            A.append([a, b, 1.0, 0.0, 0.0, 0.0, -(a * p), -(b * p), p])
            A.append([0.0, 0.0, 0.0, a, b, 1.0, -(a * q), -(b * q), q])
        sol = gauss(A, 8, 1)
        if sol is None:
            return None
        v = sol[0] + [1.0]
        N = [v[0:3], v[3:6], v[6:9]]
    R = []
    for i in range(3):
        r0, r1 = N[i][0] * s, N[i][1] * s
        R.append([r0, r1, (N[i][2] - r0 * cx) - r1 * cy])
    with np.errstate(all="ignore"):
        m = np.array([P * R[0][k] + cx * R[2][k] for k in range(3)] + [P * R[1][k] + cy * R[2][k] for k in range(3)] + R[2]).astype(F)
    if not np.isfinite(m).all():
        return None
    if model == HOMOGRAPHY:
        for x, y, _, _ in pts:
            if not (m[6] * x + m[7] * y) + m[8] > 0:
                return None
    return m


def draw_points(fd, model, thresh, seed, r, j, cur):
    """The sample of hypothesis j of round r: [(xf, yf, tx, ty)], or None when a point finds no pixel in 16 attempts."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    idx, pts = [], []
    for k in range(4 if model == HOMOGRAPHY else 3):
        for a in range(ATTEMPTS):
            i = (philox(j, (r * 4 + k) * ATTEMPTS + a, k0, k1) * fd.n) >> 32
            if not fd.part[i] or i in idx:
                continue
            if r > 0 and not inlier(cur, fd.xf[i], fd.yf[i], fd.tx[i], fd.ty[i], thresh):
                continue
            idx.append(i)
            pts.append((fd.xf[i], fd.yf[i], fd.tx[i], fd.ty[i]))
            break
        else:
            return None
    return pts


def hypothesis(fd, model, thresh, seed, r, j, cur=IDENTITY):
    pts = draw_points(fd, model, thresh, seed, r, j, cur)
    return None if pts is None else minimal_model(fd.h, fd.w, model, pts)


def polish_sums(w, h, x, y, tx, ty):
    """The twelve sums over pixels (x, y) (ints) with targets (tx, ty) (np.float32): Python ints, exact."""
    S = [0] * 12
    for xi, yi, txi, tyi in zip(x, y, tx, ty):
        a, b = 2 * int(xi) - (w - 1), 2 * int(yi) - (h - 1)
        p, q = int(np.rint(F(txi) * F(64.0))), int(np.rint(F(tyi) * F(64.0)))
        for k, v in enumerate((1, a, b, a * a, a * b, b * b, p, a * p, b * p, q, a * q, b * q)):
            S[k] += v
    return S


def polish_solve(w, h, S):
    """The candidate of a polish step from the twelve integer sums, or None: the current model stays."""
    if S[0] < 3:
        return None
    n, sa, sb, saa, sab, sbb = (float(v) for v in S[:6])
    c00, c01, c02 = sbb * n - sb * sb, sb * sa - sab * n, sab * sb - sbb * sa
    c11, c12, c22 = saa * n - sa * sa, sa * sab - saa * sb, saa * sbb - sab * sab
    det = (saa * c00 + sab * c01) + sa * c02
    if det == 0.0 or not np.isfinite(det):
        return None
    m = []
    for row in range(2):
        r2, r0, r1 = (float(v) for v in S[6 + 3 * row:9 + 3 * row])
        x0, x1 = ((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det
        x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
        m += [x0 * 0.03125, x1 * 0.03125, ((x2 - x0 * float(w - 1)) - x1 * float(h - 1)) * 0.015625]
    with np.errstate(all="ignore"):
        m = np.array(m + [0.0, 0.0, 1.0]).astype(F)
    return m if np.isfinite(m).all() else None


def fit(flow, model=AFFINE, thresh=1.0, n_hyp=64, lo_rounds=1, polish=2, step=1, seed=0, exclude=None):
    """dflow_motion_fit -> dict: model (9,), models (n_hyp,9), hyp_counts (n_hyp,), key, counts [8], cls (h,w) uint8, model_flow
    and residual (h,w,3) float32, steps: the scored inlier count after the search and after every polish step."""
    fd = Field(flow, exclude, step)
    h, w, thresh = fd.h, fd.w, F(thresh)
    cur, key, cur_count, ndeg = IDENTITY.copy(), 0, 0, 0
    for r in range(lo_rounds + 1):
        models, counts = np.tile(IDENTITY, (n_hyp, 1)), np.zeros(n_hyp, np.int32)
        for j in range(n_hyp):
            m = hypothesis(fd, model, thresh, seed, r, j, cur)
            if m is None:
                ndeg += 1
                continue
            models[j], counts[j] = m, scored_inliers(fd, m, thresh).size
            key = max(key, (int(counts[j]) << 32) | (M32 - (r * 65536 + j)))
        if key and (M32 - (key & M32)) >> 16 == r:
            cur, cur_count = models[(M32 - (key & M32)) & 0xFFFF].copy(), key >> 32
    steps, accepted, skipped = [cur_count], 0, 0
    for _ in range(polish if model == AFFINE and key else 0):
        at = scored_inliers(fd, cur, thresh)
        with np.errstate(all="ignore"):
            near = (np.abs(fd.tx[at]) <= POLISH_RANGE) & (np.abs(fd.ty[at]) <= POLISH_RANGE)
        skipped += int((~near).sum())
        at = at[near]
        cand = polish_solve(w, h, polish_sums(w, h, at % w, at // w, fd.tx[at], fd.ty[at]))
        if cand is not None:
            c = scored_inliers(fd, cand, thresh).size
            if c >= cur_count:
                cur, cur_count, accepted = cand, c, accepted + 1
        steps.append(cur_count)
    # apply
    every = np.arange(fd.n)
    inl = np.zeros(fd.n, bool)
    inl[scored_inliers(fd, cur, thresh, every)] = True
    inl &= fd.good
    cls = np.where(~fd.good, 0, np.where(fd.excluded, 3, np.where(inl, 1, 2))).astype(np.uint8)
    X, Y, W = project(cur, fd.xf, fd.yf)
    ok = W > 0
    mflow, res = np.zeros((fd.n, 3), F), np.zeros((fd.n, 3), F)
    with np.errstate(all="ignore"):
        mflow[ok, 0], mflow[ok, 1], mflow[ok, 2] = (X / W - fd.xf)[ok], (Y / W - fd.yf)[ok], 1
        g = ok & fd.good
        res[g, 0], res[g, 1], res[g, 2] = (fd.U - mflow[:, 0])[g], (fd.V - mflow[:, 1])[g], 1
    best = M32 - (key & M32)
    out_counts = [int(fd.scored.size), int(inl[fd.scored].sum()), ndeg, best >> 16 if key else -1, best & 0xFFFF if key else -1,
                  key >> 32, accepted, skipped]
    return dict(model=cur, models=models, hyp_counts=counts, key=key, counts=out_counts, cls=cls.reshape(h, w),
                model_flow=mflow.reshape(h, w, 3), residual=res.reshape(h, w, 3), steps=steps)


def hyp_counts_of(flow, js, model=AFFINE, thresh=1.0, step=1, seed=0, exclude=None):
    """d_hyp_counts[j] of round 0 for the hypotheses js only."""
    fd = Field(flow, exclude, step)
    out = []
    for j in js:
        m = hypothesis(fd, model, F(thresh), seed, 0, j)
        out.append(0 if m is None else int(scored_inliers(fd, m, F(thresh)).size))
    return out


def layers(flow, k, exclude=None, **fit_args):
    """pipeline.motion_layers: k successive fits, the inliers of each excluded from the next -> (models, (h,w) uint8 layer map)."""
    h, w = flow.shape[:2]
    ex = np.zeros((h, w), np.uint8) if exclude is None else (np.asarray(exclude) != 0).astype(np.uint8)
    layer, models = np.zeros((h, w), np.uint8), []
    for i in range(1, k + 1):
        got = fit(flow, exclude=ex, **fit_args)
        models.append(got["model"])
        layer[got["cls"] == 1] = i
        ex = ex | (got["cls"] == 1).astype(np.uint8)
    return models, layer


# ---- fields
PLANTED = {  # dyadic coefficients: the affine targets are exact in float32
    "affine": np.array([1 + 1 / 64, 1 / 128, 1.5, -1 / 128, 1 - 1 / 64, -0.75, 0, 0, 1], F),
    "affine2": np.array([1 - 1 / 32, -1 / 64, -6.25, 1 / 64, 1 - 1 / 32, 7.5, 0, 0, 1], F),
    "homography": np.array([1.01, 0.02, 1.5, -0.015, 0.99, -0.75, 1e-4, -5e-5, 1], F),
}
KINDS = ("affine", "homography", "allbad", "collinear")


def planted_flow(m, h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    xf, yf = xs.astype(F), ys.astype(F)
    X, Y, W = project(m, xf, yf)
    return np.stack([X / W - xf, Y / W - yf, np.ones((h, w), F)], axis=-1).astype(F)


def field(h, w, seed, kind="affine", outliers=0.4, dirty=True):
    """(flow (h,w,3) [U,V,valid], planted (h,w) bool: the pixels that carry the planted motion untouched, exclude (h,w) uint8)."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "allbad":
        f = rng.uniform(-3, 3, (h, w, 3)).astype(F)
        f[..., 2] = 0
        f[::2, :, 2], f[::2, :, 0] = 1, np.nan
        return f, np.zeros((h, w), bool), np.zeros((h, w), np.uint8)
    if kind == "collinear":
        f = planted_flow(PLANTED["affine"], h, w)
        f[..., 2] = 1 if h == 1 or w == 1 else (ys == xs)         # a row, a column, or the diagonal
        return f, f[..., 2] > 0.5, np.zeros((h, w), np.uint8)
    f = planted_flow(PLANTED[kind], h, w)
    planted = np.ones((h, w), bool)
    out = rng.rand(h, w) < outliers
    f[out, :2] = rng.uniform(-20, 20, (int(out.sum()), 2)).astype(F)
    planted &= ~out
    if dirty:
        u = rng.rand(h, w)
        f[u < 0.05, 2] = 0
        f[(u >= 0.05) & (u < 0.07), 0] = np.nan
        f[(u >= 0.07) & (u < 0.08), 1] = np.inf
        f[(u >= 0.08) & (u < 0.09), 0] = -np.inf
        f[(u >= 0.09) & (u < 0.11), 0] = F(1e30)
        f[(u >= 0.11) & (u < 0.12), 1] = F(-1e30)
        planted &= u >= 0.12
    exclude = (rng.rand(h, w) < 0.1).astype(np.uint8)
    return f, planted, exclude


def two_motions(h, w, seed=0):
    """The left 60 % of the frame moves by PLANTED["affine"], the rest by PLANTED["affine2"] -> (flow, (h,w) uint8 1 | 2)."""
    a, b = planted_flow(PLANTED["affine"], h, w), planted_flow(PLANTED["affine2"], h, w)
    which = np.where(np.mgrid[0:h, 0:w][1] < (w * 3) // 5, 1, 2).astype(np.uint8)
    return np.where((which == 1)[..., None], a, b).astype(F), which


def corner_shift(m, ref, h, w):
    """The largest distance, in float64, between the images of a frame corner under the models m and ref."""
    worst = 0.0
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        p = []
        for q in (m, ref):
            q = [float(v) for v in q]
            W = q[6] * x + q[7] * y + q[8]
            p.append(((q[0] * x + q[1] * y + q[2]) / W, (q[3] * x + q[4] * y + q[5]) / W))
        worst = max(worst, ((p[0][0] - p[1][0]) ** 2 + (p[0][1] - p[1][1]) ** 2) ** 0.5)
    return worst
