"""Numpy restatement of the variational refinement that dflow_var_refine computes (DESIGN.md "Variational refinement"),
written from the definition, not from the HIP code.  `dtype` selects the arithmetic: float64 is the reference, float32 the
yardstick that says how far a float32 evaluation of the same formulas may drift.  Also, independent of the iteration:
energy() (the energy whose lagged fixed-point scheme refine() is) and linear_system() (the dense matrix and right-hand
side of one inner iteration, for checking the SOR solver against np.linalg.solve)."""
import math

import numpy as np

EPS2 = 1e-6          # all three robust functions
ZETA2 = 0.01         # data normalisation
DEFAULTS = dict(alpha=1.0, gamma=0.71, delta=0.0, sigma=1.0, niter_outer=5, niter_inner=1, niter_solver=30, sor_omega=1.9)
PRESETS = {
    "sintel": dict(niter_outer=5, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
    "kitti": dict(niter_outer=2, alpha=1.0, gamma=0.77, delta=0.0, sigma=1.7),
    "middlebury": dict(niter_outer=25, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
}


def make_params(preset=None, **kw):
    P = dict(DEFAULTS)
    if preset is not None:
        P.update(PRESETS[preset])
    for k, v in kw.items():
        if k not in DEFAULTS:
            raise KeyError(k)
        P[k] = v
    return P


def gauss_taps(sigma):
    """exp(-i^2 / 2 sigma^2), i = -r..r, r = ceil(3 sigma), normalised in double and rounded to float32; sigma is the float32
    the parameter struct carries (1.7 is 1.70000005), widened to double."""
    sigma = float(np.float32(sigma))
    r = int(math.ceil(3.0 * sigma))
    i = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-i * i / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def _shift(f, k, axis):
    """f sampled at index + k along axis, replicate border."""
    n = f.shape[axis]
    return np.take(f, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)


def smooth(img, sigma, dt):
    """(H,W,3) uint8 -> (H,W,3) dt: separable Gaussian, along x then along y, taps summed from -r to r."""
    f = np.asarray(img).astype(dt)
    if sigma == 0:
        return f
    taps = gauss_taps(sigma).astype(dt)
    r = len(taps) // 2
    for axis in (1, 0):
        acc = np.zeros_like(f)
        for i in range(-r, r + 1):
            acc = acc + taps[i + r] * _shift(f, i, axis)
        f = acc
    return f


def D(f, axis):
    """(f(-2) - 8 f(-1) + 8 f(+1) - f(+2)) / 12, replicate border."""
    dt = f.dtype.type
    return (((_shift(f, -2, axis) - dt(8) * _shift(f, -1, axis)) + dt(8) * _shift(f, 1, axis)) - _shift(f, 2, axis)) / dt(12)


def Dx(f):
    return D(f, 1)


def Dy(f):
    return D(f, 0)


def central(f, axis):
    return f.dtype.type(0.5) * (_shift(f, 1, axis) - _shift(f, -1, axis))


def psi_prime(s2):
    dt = s2.dtype.type
    return dt(1) / (dt(2) * np.sqrt(s2 + dt(EPS2)))


def local_weight(I1):
    """omega = exp(-5 sqrt((Dx L)^2 + (Dy L)^2) / 255) of the smoothed first image (BGR)."""
    dt = I1.dtype.type
    L = (dt(0.114) * I1[..., 0] + dt(0.587) * I1[..., 1]) + dt(0.299) * I1[..., 2]
    lx, ly = Dx(L), Dy(L)
    return np.exp(dt(-5) * np.sqrt(lx * lx + ly * ly) / dt(255))


def warp(I2, u, v):
    """Bilinear sample of I2 at (x + u, y + v), coordinates clamped; mask 1 where the unclamped sample lies in the image.
    A non-finite flow value: mask 0, the pixel sampled at itself."""
    H, W = u.shape
    dt = I2.dtype.type
    yy, xx = np.meshgrid(np.arange(H).astype(dt), np.arange(W).astype(dt), indexing="ij")
    fin = np.isfinite(u) & np.isfinite(v)
    with np.errstate(invalid="ignore"):
        xs = np.where(fin, xx + u, xx)
        ys = np.where(fin, yy + v, yy)
        m = fin & (xs >= 0) & (xs <= dt(W - 1)) & (ys >= 0) & (ys <= dt(H - 1))
    xs = np.clip(xs, dt(0), dt(W - 1))
    ys = np.clip(ys, dt(0), dt(H - 1))
    x0 = np.floor(xs)
    y0 = np.floor(ys)
    fx = (xs - x0)[..., None]
    fy = (ys - y0)[..., None]
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    x1 = np.minimum(x0 + 1, W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    one = dt(1)
    top = (one - fx) * I2[y0, x0] + fx * I2[y0, x1]
    bot = (one - fx) * I2[y1, x0] + fx * I2[y1, x1]
    return (one - fy) * top + fy * bot, m.astype(I2.dtype)


def derivatives(I1, I2w):
    dt = I1.dtype.type
    Ibar = dt(0.5) * (I1 + I2w)
    Ix, Iy = Dx(Ibar), Dy(Ibar)
    Iz = I2w - I1
    return dict(Ix=Ix, Iy=Iy, Iz=Iz, Ixx=Dx(Ix), Ixy=Dy(Ix), Iyy=Dy(Iy), Ixz=Dx(Iz), Iyz=Dy(Iz))


def _sum3(a):
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def edge_weights(u, v, du, dv, omega, alpha):
    """(sx, sy): sx (H,W-1) the weights of the edges (x, x+1), sy (H-1,W) of the edges (y, y+1)."""
    dt = u.dtype.type
    U, V = u + du, v + dv
    ux, uy, vx, vy = central(U, 1), central(U, 0), central(V, 1), central(V, 0)
    p = omega * psi_prime(((ux * ux + uy * uy) + vx * vx) + vy * vy)
    sx = dt(alpha) * (dt(0.5) * (p[:, :-1] + p[:, 1:]))
    sy = dt(alpha) * (dt(0.5) * (p[:-1, :] + p[1:, :]))
    return sx, sy


def neighbour_weights(sx, sy, H, W):
    """(sL, sR, sU, sD), each (H,W): the weight of the edge to that neighbour, 0 where it leaves the image."""
    z = np.zeros((H, W), sx.dtype)
    sL, sR, sU, sD = z.copy(), z.copy(), z.copy(), z.copy()
    sL[:, 1:] = sx
    sR[:, :-1] = sx
    sU[1:, :] = sy
    sD[:-1, :] = sy
    return sL, sR, sU, sD


def _neigh(f):
    """(left, right, up, down) neighbours of f, zeros outside the image (their weights are 0)."""
    P = np.pad(f, 1)
    return P[1:-1, :-2], P[1:-1, 2:], P[:-2, 1:-1], P[2:, 1:-1]


def _wsum(ws, fs, centre=None):
    acc = None
    for s, f in zip(ws, fs):
        t = s * (f if centre is None else f - centre)
        acc = t if acc is None else acc + t
    return acc


def data_term(d, m, du, dv, gamma, delta):
    dt = du.dtype.type
    z2 = dt(ZETA2)
    du3, dv3 = du[..., None], dv[..., None]
    Ixx, Ixy, Iyy, Ixz, Iyz = d["Ixx"], d["Ixy"], d["Iyy"], d["Ixz"], d["Iyz"]
    nx = dt(1) / ((Ixx * Ixx + Ixy * Ixy) + z2)
    ny = dt(1) / ((Ixy * Ixy + Iyy * Iyy) + z2)
    rx = (Ixz + Ixx * du3) + Ixy * dv3
    ry = (Iyz + Ixy * du3) + Iyy * dv3
    g = (dt(gamma) * m) * psi_prime(_sum3(nx * (rx * rx) + ny * (ry * ry)))
    a11 = g * _sum3(nx * (Ixx * Ixx) + ny * (Ixy * Ixy))
    a12 = g * _sum3(nx * (Ixx * Ixy) + ny * (Ixy * Iyy))
    a22 = g * _sum3(nx * (Ixy * Ixy) + ny * (Iyy * Iyy))
    b1 = -(g * _sum3(nx * (Ixx * Ixz) + ny * (Ixy * Iyz)))
    b2 = -(g * _sum3(nx * (Ixy * Ixz) + ny * (Iyy * Iyz)))
    if delta > 0:
        Ix, Iy, Iz = d["Ix"], d["Iy"], d["Iz"]
        n = dt(1) / ((Ix * Ix + Iy * Iy) + z2)
        r = (Iz + Ix * du3) + Iy * dv3
        k = (dt(delta) * m) * psi_prime(_sum3(n * (r * r)))
        a11 = a11 + k * _sum3(n * (Ix * Ix))
        a12 = a12 + k * _sum3(n * (Ix * Iy))
        a22 = a22 + k * _sum3(n * (Iy * Iy))
        b1 = b1 - k * _sum3(n * (Ix * Iz))
        b2 = b2 - k * _sum3(n * (Iy * Iz))
    return a11, a12, a22, b1, b2


def inner_coefficients(d, m, omega, u, v, du, dv, P):
    """(a11, a12, a22, b1, b2, (sL, sR, sU, sD)) of one inner iteration: the data term at (du, dv), the lagged smoothness
    weights, and the divergence of the current flow added to b."""
    H, W = u.shape
    sx, sy = edge_weights(u, v, du, dv, omega, P["alpha"])
    ws = neighbour_weights(sx, sy, H, W)
    a11, a12, a22, b1, b2 = data_term(d, m, du, dv, P["gamma"], P["delta"])
    b1 = b1 + _wsum(ws, _neigh(u), u)
    b2 = b2 + _wsum(ws, _neigh(v), v)
    return a11, a12, a22, b1, b2, ws


def sor(a11, a12, a22, b1, b2, ws, du, dv, niter, omega_sor):
    """niter iterations of red-black SOR (red = (x + y) even first), in place on copies of du, dv."""
    dt = du.dtype.type
    H, W = du.shape
    w = dt(omega_sor)
    ss = ((ws[0] + ws[1]) + ws[2]) + ws[3]
    A11, A22 = a11 + ss, a22 + ss
    det = A11 * A22 - a12 * a12
    ok = det > 0
    safe = np.where(ok, det, dt(1))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    colour = (xx + yy) & 1
    du, dv = du.copy(), dv.copy()
    for _ in range(niter):
        for c in (0, 1):
            B1 = b1 + _wsum(ws, _neigh(du))
            B2 = b2 + _wsum(ws, _neigh(dv))
            ndu = (dt(1) - w) * du + w * ((A22 * B1 - a12 * B2) / safe)
            ndv = (dt(1) - w) * dv + w * ((A11 * B2 - a12 * B1) / safe)
            sel = ok & (colour == c)
            du = np.where(sel, ndu, du)
            dv = np.where(sel, ndv, dv)
    return du, dv


def prepare(img1, img2, P, dt):
    I1, I2 = smooth(img1, P["sigma"], dt), smooth(img2, P["sigma"], dt)
    return I1, I2, local_weight(I1)


def refine(img1, img2, flow, dtype=np.float64, preset=None, **params):
    """Two (H,W,3) uint8 BGR images and a (H,W,2) [dy,dx] flow -> the refined (H,W,2) flow in `dtype`."""
    P = make_params(preset, **params)
    dt = np.dtype(dtype).type
    flow = np.asarray(flow)
    v, u = flow[..., 0].astype(dt), flow[..., 1].astype(dt)
    I1, I2, omega = prepare(img1, img2, P, dt)
    for _ in range(P["niter_outer"]):
        I2w, m = warp(I2, u, v)
        d = derivatives(I1, I2w)
        du, dv = np.zeros_like(u), np.zeros_like(v)
        for _ in range(P["niter_inner"]):
            a11, a12, a22, b1, b2, ws = inner_coefficients(d, m, omega, u, v, du, dv, P)
            du, dv = sor(a11, a12, a22, b1, b2, ws, du, dv, P["niter_solver"], P["sor_omega"])
        u, v = u + du, v + dv
    return np.stack([v, u], axis=-1)


def linear_system(img1, img2, flow, preset=None, **params):
    """The dense (2N, 2N) matrix and right-hand side, float64, of the first inner iteration of the first outer iteration
    (du = dv = 0 in the lagged weights); unknowns ordered [du(0..N-1), dv(0..N-1)], N = H*W in row-major order."""
    P = make_params(preset, **params)
    flow = np.asarray(flow)
    v, u = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    H, W = u.shape
    N = H * W
    I1, I2, omega = prepare(img1, img2, P, np.float64)
    I2w, m = warp(I2, u, v)
    d = derivatives(I1, I2w)
    z = np.zeros_like(u)
    a11, a12, a22, b1, b2, ws = inner_coefficients(d, m, omega, u, v, z, z, P)
    A = np.zeros((2 * N, 2 * N))
    offs = (-1, 1, -W, W)
    for y in range(H):
        for x in range(W):
            i = y * W + x
            ss = sum(s[y, x] for s in ws)
            A[i, i] = a11[y, x] + ss
            A[N + i, N + i] = a22[y, x] + ss
            A[i, N + i] = A[N + i, i] = a12[y, x]
            for s, o in zip(ws, offs):
                if s[y, x] != 0:
                    A[i, i + o] -= s[y, x]
                    A[N + i, N + i + o] -= s[y, x]
    return A, np.concatenate([b1.ravel(), b2.ravel()])


def _bilinear(img, xs, ys):
    """Plain bilinear lookup with clamped coordinates (energy's own, independent of warp())."""
    H, W = img.shape[:2]
    xs = np.clip(xs, 0, W - 1)
    ys = np.clip(ys, 0, H - 1)
    x0 = np.minimum(np.floor(xs).astype(int), max(W - 2, 0))
    y0 = np.minimum(np.floor(ys).astype(int), max(H - 2, 0))
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = (xs - x0)[..., None], (ys - y0)[..., None]
    return (img[y0, x0] * (1 - ax) + img[y0, x1] * ax) * (1 - ay) + (img[y1, x0] * (1 - ax) + img[y1, x1] * ax) * ay


def energy(img1, img2, flow, preset=None, **params):
    """E(w) = sum_pixels m [gamma Psi(sum_c nx (dx I2(x+w) - dx I1)^2 + ny (dy I2(x+w) - dy I1)^2)
                            + delta Psi(sum_c n (I2(x+w) - I1)^2)] + alpha sum omega Psi(|grad u|^2 + |grad v|^2),
    Psi(s^2) = sqrt(s^2 + eps^2), in float64.  The normalisations are those of the scheme, evaluated at w."""
    P = make_params(preset, **params)
    flow = np.asarray(flow, np.float64)
    v, u = flow[..., 0], flow[..., 1]
    H, W = u.shape
    I1, I2, omega = prepare(img1, img2, P, np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = (xx + u >= 0) & (xx + u <= W - 1) & (yy + v >= 0) & (yy + v <= H - 1)
    J = _bilinear(I2, xx + u, yy + v)
    mean = 0.5 * (I1 + J)
    diff = J - I1
    gx, gy = Dx(mean), Dy(mean)
    gxx, gxy, gyy = Dx(gx), Dy(gx), Dy(gy)
    ex, ey = Dx(diff), Dy(diff)
    grad = (ex ** 2 / (gxx ** 2 + gxy ** 2 + ZETA2) + ey ** 2 / (gxy ** 2 + gyy ** 2 + ZETA2)).sum(axis=-1)
    e_data = P["gamma"] * np.sqrt(grad + EPS2)
    if P["delta"] > 0:
        col = (diff ** 2 / (gx ** 2 + gy ** 2 + ZETA2)).sum(axis=-1)
        e_data = e_data + P["delta"] * np.sqrt(col + EPS2)
    smooth_ = central(u, 1) ** 2 + central(u, 0) ** 2 + central(v, 1) ** 2 + central(v, 0) ** 2
    return float((inside * e_data).sum() + P["alpha"] * (omega * np.sqrt(smooth_ + EPS2)).sum())
