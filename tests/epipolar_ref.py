"""dflow_epipolar_fit restated from include/dflow.h ("Epipolar-geometry fit"): the draws, the float64 elimination with complete
pivoting, the cubic and its bisections in plain Python floats (IEEE doubles), the float32 score, the keys and the apply step in
np.float32 arithmetic in the written order.  And the scenes the tests fit: a pinhole camera moved through a smooth depth map,
with a rectangle that moves on its own.  Philox, the planes of a field and the normalisation are motion_ref's."""
import math

import numpy as np

import motion_ref as M
from motion_ref import Field, normalisation, philox

F = np.float32
UVV, DYDX = M.UVV, M.DYDX
CHUNK = 2048                      # FIT_CHUNK of csrc/fit_common.h: the scored pixels a block stages
ATTEMPTS = 16
PIVOT_MIN = 2.0 ** -40
BISECTIONS = 60
M32 = 0xFFFFFFFF
NO_MODEL = np.zeros(9, F)
COUNTS = ("scored", "inliers", "degenerate", "best_round", "best_slot", "best_count", "models_per_1000", "reserved")


class Coords:
    """The float32 normalised coordinates (a, b, p, q) of every pixel of a Field, and t2 = (thresh*s)*(thresh*s)."""

    def __init__(self, fd, thresh):
        self.cx, self.cy, self.s, self.P = normalisation(fd.h, fd.w)
        cx, cy, s = F(self.cx), F(self.cy), F(self.s)
        with np.errstate(all="ignore"):
            self.a, self.b = (fd.xf - cx) * s, (fd.yf - cy) * s
            self.p, self.q = (fd.tx - cx) * s, (fd.ty - cy) * s
            t = F(thresh) * s
            self.t2 = F(t * t)


def terms(m, a, b, p, q):
    """(e*e, den) of the float32 model m at float32 scalars or arrays, in the written order."""
    with np.errstate(all="ignore"):
        l0, l1, l2 = (m[0] * a + m[1] * b) + m[2], (m[3] * a + m[4] * b) + m[5], (m[6] * a + m[7] * b) + m[8]
        e = (p * l0 + q * l1) + l2
        m0, m1 = (m[0] * p + m[3] * q) + m[6], (m[1] * p + m[4] * q) + m[7]
        den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
        return e * e, den


def inlier(m, a, b, p, q, t2, strict=False):
    """INLIER.  strict: the mutation `<` for `<=`."""
    ee, den = terms(m, a, b, p, q)
    with np.errstate(all="ignore"):
        ok = (den > 0) & (den < np.inf)
        return ok & ((ee < t2 * den) if strict else (ee <= t2 * den))


def scored_inliers(fd, co, m, at=None, strict=False):
    at = fd.scored if at is None else at
    return at[inlier(m, co.a[at], co.b[at], co.p[at], co.q[at], co.t2, strict)]


# ---- the float64 solve of one sample
def det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def null_space(A, complete=True):
    """ELIMINATION of the 7 x 9 system A (a list of rows of Python floats) -> (F1, F2), or None for a small pivot.  complete=False
    is the mutation: partial pivoting, the free columns always 7 and 8."""
    perm = list(range(9))
    for c in range(7):
        pr, pk, best = c, c, abs(A[c][c])
        for r in range(c, 7):
            for k in range(c, 9 if complete else c + 1):
                if abs(A[r][k]) > best:
                    pr, pk, best = r, k, abs(A[r][k])
        if not best >= PIVOT_MIN:
            return None
        A[c], A[pr] = A[pr], A[c]
        if pk != c:
            for r in range(7):
                A[r][c], A[r][pk] = A[r][pk], A[r][c]
            perm[c], perm[pk] = perm[pk], perm[c]
        for r in range(c + 1, 7):
            f = A[r][c] / A[c][c]
            for k in range(c + 1, 9):
                A[r][k] = A[r][k] - f * A[c][k]
    out = []
    for free in (7, 8):
        x = [0.0] * 9
        x[free] = 1.0
        for r in range(6, -1, -1):
            t = -A[r][free]
            for k in range(r + 1, 7):
                t = t - A[r][k] * x[k]
            x[r] = t / A[r][r]
        f = [0.0] * 9
        for i in range(9):
            f[perm[i]] = x[i]
        out.append(f)
    return out


def cubic_roots(c3, c2, c1, c0, closed):
    """ROOTS of c3 x^3 + c2 x^2 + c1 x + c0 in [-1, 1] (closed) or (-1, 1), ascending, each by 60 bisections of a monotone piece."""
    g = lambda x: ((c3 * x + c2) * x + c1) * x + c0
    qa, qb = 3.0 * c3, 2.0 * c2
    disc = qb * qb - (4.0 * qa) * c1
    pts = [-1.0]
    if disc > 0.0:
        sq = math.sqrt(disc)
        qq = -0.5 * (qb + (-sq if qb < 0.0 else sq))
        x1 = qq / qa if qa != 0.0 else math.inf
        x2 = c1 / qq
        xa, xb = (x1, x2) if x1 < x2 else (x2, x1)
        for x in (xa, xb):
            if -1.0 < x < 1.0:
                pts.append(x)
    pts.append(1.0)
    roots = []
    gu = g(-1.0)
    if closed and gu == 0.0:
        roots.append(-1.0)
    for i in range(1, len(pts)):
        u, v = pts[i - 1], pts[i]
        gv = g(v)
        if gv == 0.0:
            if closed or v != 1.0:
                roots.append(v)
        elif (gu < 0.0 and gv > 0.0) or (gu > 0.0 and gv < 0.0):
            lo, hi = u, v
            for _ in range(BISECTIONS):
                mid = 0.5 * (lo + hi)
                if (g(mid) < 0.0) == (gu < 0.0):
                    lo = mid
                else:
                    hi = mid
            roots.append(0.5 * (lo + hi))
        gu = gv
    return roots


def canonical(f):
    """CANONICAL SCALE of nine Python floats -> nine Python floats (not yet cast)."""
    big = 0
    for i in range(1, 9):
        if abs(f[i]) > abs(f[big]):
            big = i
    d = f[big]
    with np.errstate(all="ignore"):
        return [float(np.float64(v) / np.float64(d)) for v in f]


def solve7(rows, complete=True, both_branches=True):
    """The models of one sample in float64: rows = [(a, b, p, q)] * 7 (Python floats) -> a list of 0..3 lists of nine floats in
    canonical scale (entries may be non-finite: the caller drops those), or None when the elimination is degenerate."""
    A = [[p * a, p * b, p, q * a, q * b, q, a, b, 1.0] for a, b, p, q in rows]
    ns = null_space(A, complete)
    if ns is None:
        return None
    f1, f2 = ns
    k3, k0 = det3(f1), det3(f2)
    dp, dm = det3([x + y for x, y in zip(f1, f2)]), det3([y - x for x, y in zip(f1, f2)])
    k2, k1 = (dp + dm) * 0.5 - k0, (dp - dm) * 0.5 - k3
    if not all(math.isfinite(v) for v in (k0, k1, k2, k3)):
        return []
    out = [[al * x + y for x, y in zip(f1, f2)] for al in cubic_roots(k3, k2, k1, k0, True)]
    if both_branches:
        out += [[x + be * y for x, y in zip(f1, f2)] for be in cubic_roots(k0, k1, k2, k3, False)]
    return [canonical(f) for f in out[:3]]


def sample_rows(co, pts):
    """The float64 normalised coordinates of the sample's pixels (flat indices are not needed: Field's float32 planes)."""
    return [((float(x) - co.cx) * co.s, (float(y) - co.cy) * co.s, (float(tx) - co.cx) * co.s, (float(ty) - co.cy) * co.s)
            for x, y, tx, ty in pts]


def models_of(co, pts, **mut):
    """The float32 models of the slots 3j .. 3j+2 of a sample: [model or None] * 3."""
    sol = solve7(sample_rows(co, pts), **mut)
    out = [None, None, None]
    for m, f in enumerate(sol or []):
        with np.errstate(all="ignore"):
            f32 = np.array(f, np.float64).astype(F)
        if np.isfinite(f32).all():
            out[m] = f32
    return out


def draw_points(fd, co, seed, r, j, cur):
    """The sample of hypothesis j of round r: [(xf, yf, tx, ty)] * 7, or None when a point finds no pixel in 16 attempts."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    idx, pts = [], []
    for k in range(7):
        for a in range(ATTEMPTS):
            i = (philox(j, (r * 8 + k) * ATTEMPTS + a, k0, k1) * fd.n) >> 32
            if not fd.part[i] or i in idx:
                continue
            if r > 0 and not inlier(cur, co.a[i], co.b[i], co.p[i], co.q[i], co.t2):
                continue
            idx.append(i)
            pts.append((fd.xf[i], fd.yf[i], fd.tx[i], fd.ty[i]))
            break
        else:
            return None
    return pts


def fit(flow, thresh=1.0, n_hyp=64, lo_rounds=1, step=1, seed=0, exclude=None, strict=False, **mut):
    """dflow_epipolar_fit -> dict: model (9,), models (3 n_hyp, 9), hyp_counts (3 n_hyp,), key, counts [8], cls (h,w) uint8,
    residual (h,w) float32.  strict, complete=False and both_branches=False are the mutations the tests must catch."""
    fd = Field(flow, exclude, step)
    co = Coords(fd, thresh)
    h, w = fd.h, fd.w
    cur, key, ndeg, ndeg0 = NO_MODEL.copy(), 0, 0, 0
    for r in range(lo_rounds + 1):
        models, counts = np.zeros((3 * n_hyp, 9), F), np.zeros(3 * n_hyp, np.int32)
        for j in range(n_hyp):
            pts = draw_points(fd, co, seed, r, j, cur)
            ms = [None] * 3 if pts is None else models_of(co, pts, **mut)
            for m, model in enumerate(ms):
                slot = 3 * j + m
                if model is None:
                    ndeg += 1
                    ndeg0 += r == 0
                    continue
                models[slot], counts[slot] = model, scored_inliers(fd, co, model, strict=strict).size
                key = max(key, (int(counts[slot]) << 32) | (M32 - (r * 65536 + slot)))
        if key and (M32 - (key & M32)) >> 16 == r:
            cur = models[(M32 - (key & M32)) & 0xFFFF].copy()
    every = np.arange(fd.n)
    inl = np.zeros(fd.n, bool)
    inl[scored_inliers(fd, co, cur, every, strict)] = True
    inl &= fd.good
    cls = np.where(~fd.good, 0, np.where(fd.excluded, 3, np.where(inl, 1, 2))).astype(np.uint8)
    ee, den = terms(cur, co.a, co.b, co.p, co.q)
    with np.errstate(all="ignore"):
        ok = (den > 0) & (den < np.inf)
        res = np.where(fd.good, np.where(ok, np.sqrt(ee / den) * F(co.P), F(np.inf)), F(-1.0)).astype(F)
    best = M32 - (key & M32)
    out_counts = [int(fd.scored.size), int(inl[fd.scored].sum()), ndeg, best >> 16 if key else -1, best & 0xFFFF if key else -1,
                  key >> 32, (1000 * (3 * n_hyp - ndeg0)) // n_hyp, 0]
    return dict(model=cur, models=models, hyp_counts=counts, key=key, counts=out_counts, cls=cls.reshape(h, w), residual=res.reshape(h, w))


def slot_counts_of(flow, js, thresh=1.0, step=1, seed=0, exclude=None):
    """d_hyp_counts[3j .. 3j+2] of round 0 for the samples js only."""
    fd = Field(flow, exclude, step)
    co = Coords(fd, thresh)
    out = []
    for j in js:
        pts = draw_points(fd, co, seed, 0, j, NO_MODEL)
        for model in ([None] * 3 if pts is None else models_of(co, pts)):
            out.append(0 if model is None else int(scored_inliers(fd, co, model).size))
    return out


def geometry(model, h, w):
    """pipeline.epipolar_geometry in plain float64: (F in pixel coordinates, e1, e2, foe or None)."""
    cx, cy, s, _ = normalisation(h, w)
    T = np.array([[s, 0.0, -cx * s], [0.0, s, -cy * s], [0.0, 0.0, 1.0]])
    Fp = T.T @ np.asarray(model, np.float64).reshape(3, 3) @ T

    def null(rows):
        cs = [np.cross(rows[i], rows[j]) for i, j in ((0, 1), (0, 2), (1, 2))]
        return max(cs, key=lambda c: float(c @ c))
    e1, e2 = null(Fp), null(Fp.T)
    scale = float(np.abs(e1).max())
    foe = None if not abs(e1[2]) > 1e-12 * scale else (float(e1[0] / e1[2]), float(e1[1] / e1[2]))
    return Fp, e1, e2, foe


# ---- scenes: a pinhole camera (focal length max(h, w), principal point the frame's centre) moved through a smooth depth map
SCENES = {  # name: (h, w, t, rot)
    "sideways": (33, 65, (0.4, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "forward": (33, 65, (0.0, 0.0, 0.9), (0.0, 0.0, 0.0)),
    "mixed": (48, 160, (0.3, -0.1, 0.6), (0.004, -0.006, 0.003)),
}
OBJECT_MOTION = (3.0, -4.0)


def rotation(rot):
    rx, ry, rz = rot
    th = math.sqrt(rx * rx + ry * ry + rz * rz)
    K = np.array([[0.0, -rz, ry], [rz, 0.0, -rx], [-ry, rx, 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def rigid_flow(h, w, seed, t, rot, objects=()):
    """The restatement's own scene, independent of synth.rigid_flow but of the same model: (flow (h,w,3) float64 [U,V,1], mask)."""
    rng = np.random.RandomState(seed)
    f, cx, cy = float(max(h, w)), (w - 1) * 0.5, (h - 1) * 0.5
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 4)
    Z = 8.0 + 2.0 * np.sin(2 * np.pi * 1.3 * xs / w + ph[0]) * np.cos(2 * np.pi * 0.9 * ys / h + ph[1]) \
        + 1.5 * np.sin(2 * np.pi * (0.7 * xs / w + 1.1 * ys / h) + ph[2]) + 1.0 * np.cos(2 * np.pi * 2.1 * xs / w + ph[3])
    X = np.stack([(xs - cx) / f * Z, (ys - cy) / f * Z, Z], axis=-1)
    Y = X @ rotation(rot).T + np.asarray(t, np.float64)
    U, V = f * Y[..., 0] / Y[..., 2] + cx - xs, f * Y[..., 1] / Y[..., 2] + cy - ys
    mask = np.zeros((h, w), bool)
    for y0, x0, y1, x1, du, dv in objects:
        U[y0:y1, x0:x1] += du
        V[y0:y1, x0:x1] += dv
        mask[y0:y1, x0:x1] = True
    return np.stack([U, V, np.ones((h, w))], axis=-1), mask


def scene(name, seed=0, noise=0.1, moving=True):
    """(flow (h,w,3) float32 [U,V,1], mask of the moving rectangle) of a planted scene with Gaussian noise on every vector."""
    h, w, t, rot = SCENES[name]
    objects = ((h // 4, w // 2, h // 4 + h // 3, w // 2 + w // 4) + OBJECT_MOTION,) if moving else ()
    f, mask = rigid_flow(h, w, seed, t, rot, objects)
    rng = np.random.RandomState(seed + 1000)
    f[..., :2] += noise * rng.standard_normal((h, w, 2))
    return f.astype(F), mask


def dirty(flow, seed):
    """Holes, NaN / inf / huge vectors on a scene, and an exclude mask -> (flow, exclude)."""
    rng = np.random.RandomState(seed)
    f = flow.copy()
    h, w = f.shape[:2]
    u = rng.rand(h, w)
    f[u < 0.05, 2] = 0
    f[(u >= 0.05) & (u < 0.07), 0] = np.nan
    f[(u >= 0.07) & (u < 0.08), 1] = np.inf
    f[(u >= 0.08) & (u < 0.09), 0] = -np.inf
    f[(u >= 0.09) & (u < 0.11), 0] = F(1e30)
    f[(u >= 0.11) & (u < 0.12), 1] = F(-3e38)
    out = rng.rand(h, w) < 0.2
    f[out, :2] += rng.uniform(-20, 20, (int(out.sum()), 2)).astype(F)
    return f, (rng.rand(h, w) < 0.1).astype(np.uint8)


def field(h, w, seed, dirt=True):
    """A rigid scene of any size with 0.1 px noise, a moving rectangle where the frame has room for one and, with dirt, holes,
    NaN / inf / huge vectors and outliers -> (flow (h,w,3) float32, exclude (h,w) uint8)."""
    objects = ((h // 4, w // 2, h // 4 + h // 3, w // 2 + w // 4) + OBJECT_MOTION,) if h >= 8 and w >= 8 else ()
    f, _ = rigid_flow(h, w, seed, SCENES["mixed"][2], SCENES["mixed"][3], objects)
    f[..., :2] += 0.1 * np.random.RandomState(seed + 1000).standard_normal((h, w, 2))
    f = f.astype(F)
    return dirty(f, seed + 1) if dirt else (f, np.zeros((h, w), np.uint8))
