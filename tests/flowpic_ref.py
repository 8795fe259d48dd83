"""dflow_flow_color and dflow_warp_eval (include/dflow.h) restated in numpy from their definitions, not from the HIP code, and
the inputs tests/test_gpu_flowpic.py runs them on (made here so that tests/test_flowpic_ref.py can judge them without a GPU).
The colour picture is float64 with one rounding per operation (numpy does not fuse) and keeps the unrounded 255 * col next
to the bytes; the warp is float32, operation for operation, the statistics as Python ints and a sequential double sum."""
import numpy as np

import eval_ref

F = np.float32
SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))


def wheel():
    """(55,3) int (r,g,b): the Middlebury colour wheel, integer divisions."""
    rows = []
    for name, n in SEGMENTS:
        for i in range(n):
            t = 255 * i // n
            rows.append({"RY": (255, t, 0), "YG": (255 - t, 255, 0), "GC": (0, 255, t), "CB": (0, 255 - t, 255),
                         "BM": (t, 0, 255), "MR": (255, 0, 255 - t)}[name])
    return np.array(rows, np.int64)


def split(flow):
    """(H,W,3) [U,V,valid] or (H,W,2) [dy,dx] float32 -> U, V, known."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] in (2, 3)
    if flow.shape[2] == 3:
        U, V, valid = flow[..., 0], flow[..., 1], flow[..., 2]
    else:
        U, V, valid = flow[..., 1], flow[..., 0], np.ones(flow.shape[:2], F)
    with np.errstate(all="ignore"):
        known = (valid > F(0.5)) & (np.abs(U) <= F(1e9)) & (np.abs(V) <= F(1e9))
    return U, V, known


def flow_color(flow, max_flow=0.0):
    """-> dict: maxrad (float32), c (H,W,3) float64 = the unrounded 255 * col in (b,g,r) order (0 at unknown pixels), bgr
    (H,W,3) uint8 = its integer part, known (H,W) bool."""
    U, V, known = split(flow)
    if max_flow > 0:
        maxrad = F(max_flow)
    else:
        r = np.sqrt(U[known] * U[known] + V[known] * V[known])
        assert r.dtype == np.float32
        maxrad = r.max() if r.size and r.max() > 0 else F(1.0)
    m = np.float64(maxrad)
    fx, fy = np.where(known, U, F(0)).astype(np.float64) / m, np.where(known, V, F(0)).astype(np.float64) / m
    rad = np.sqrt(fx * fx + fy * fy)
    a = np.arctan2(-fy, -fx) / np.pi
    fk = (a + 1.0) / 2.0 * 54.0
    k0 = np.minimum(54, np.floor(fk).astype(np.int64))
    k1 = (k0 + 1) % 55
    f = fk - k0
    w = wheel().astype(np.float64) / 255.0
    c0, c1 = w[k0], w[k1]                                   # (H,W,3) in (r,g,b)
    col = c0 + f[..., None] * (c1 - c0)
    col = np.where((rad <= 1.0)[..., None], 1.0 - rad[..., None] * (1.0 - col), col * 0.75)
    c = np.where(known[..., None], 255.0 * col, 0.0)[..., ::-1]
    return dict(maxrad=maxrad, c=np.ascontiguousarray(c), bgr=c.astype(np.int64).astype(np.uint8), known=known)


def near_integer(c):
    """(H,W) bool: a channel of the pixel lies in the band 0 < |c - rint(c)| <= 1e-6, where another libm's atan2 may move
    the byte."""
    d = np.abs(c - np.rint(c))
    return ((d > 0) & (d <= 1e-6)).any(axis=-1)


def warp(img1, img2, flow, err_thresh=10.0, err_max=30.0):
    """-> dict: the fields of struct dflow_photo_stats (counts as Python ints, sum_err the sequential double sum in pixel
    order, max_err a float), warped (H,W,3) uint8, err (H,W) float32, bgr (H,W,3) uint8."""
    U, V, known = split(flow)
    H, W = U.shape
    yi, xi = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        xs, ys = xi.astype(F) + U, yi.astype(F) + V
        inside = known & (xs >= F(0)) & (xs <= F(W - 1)) & (ys >= F(0)) & (ys <= F(H - 1))
    xs, ys = np.where(inside, xs, F(0)), np.where(inside, ys, F(0))
    x0f, y0f = np.floor(xs), np.floor(ys)
    ax, ay = (xs - x0f)[..., None], (ys - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    I1, I2 = np.asarray(img1).astype(F), np.asarray(img2).astype(F)
    top = (F(1) - ax) * I2[y0, x0] + ax * I2[y0, x1]
    bot = (F(1) - ax) * I2[y1, x0] + ax * I2[y1, x1]
    wv = (F(1) - ay) * top + ay * bot
    d = np.abs(wv - I1)
    e = ((d[..., 0] + d[..., 1]) + d[..., 2]) / F(3)
    assert wv.dtype == np.float32 and e.dtype == np.float32
    t = np.minimum(e, F(err_max)) / F(err_max)
    idx = np.minimum(255, (t * F(256.0)).astype(np.int32))
    ec = e[inside]
    s = 0.0
    for v in ec.tolist():
        s += v
    return dict(n=int(inside.sum()), n_outside=int((known & ~inside).sum()), n_unknown=int((~known).sum()),
                n_above=int((ec > F(err_thresh)).sum()), sum_err=s, max_err=float(ec.max()) if ec.size else 0.0,
                warped=np.where(inside[..., None], np.floor(wv + F(0.5)), F(0)).astype(np.uint8),
                err=np.where(inside, e, F(-1)).astype(F),
                bgr=np.where(inside[..., None], eval_ref.jet_lut()[idx][..., ::-1], 0).astype(np.uint8))


# ---------------------------------------------------------------------------------- the inputs of the GPU tests
SHAPES = [(1, 1), (1, 7), (5, 1), (33, 65), (37, 61)]          # 37 x 61 = 2257 px: no multiple of 4, three blocks
SCALES = (4.0, 20.0)
# 1,052,675 px, a three-pixel tail, 1029 blocks' worth of groups: more than the 1024 blocks of the capped grid, whose first
# blocks take a second grid-stride step; one scale, so that its references stay within a second or two
BIG_SHAPE, BIG_SCALE = (1025, 1027), 4.0
BIG = F(125.0)                                                  # the planted maximum: beyond 6 sigma of either scale


def color_planted():
    """Rows (U, V, valid), the most telling first."""
    nan, inf = F(np.nan), F(np.inf)
    rows = [(BIG, 0.0, 1), (0.0, 0.0, 1), (nan, 1, 1), (5, 5, 0), (0.0, 7.0, 1), (1, inf, 1), (2e9, 0, 1),
            # from here on only fields of more than 7 pixels; (BIG, -0) is wheel entry 54 at rad = 1, whose blue channel is
            # 255 * (1 - 1 * (1 - 43 / 255)) = 43.000000000000014: the one planted pixel inside the band of near_integer
            (BIG, -0.0, 1), (-0.0, 0.0, 1), (0.0, -0.0, 1), (-0.0, -0.0, 1), (-inf, nan, 1), (0, -2e9, 1), (1, 1, 0.5),
            (-BIG, 0.0, 1), (0.0, -BIG, 1), (75.0, 100.0, 1)]
    return np.array(rows, F)


def _random_flow(H, W, scale, seed):
    rng = np.random.default_rng(seed)
    flow = np.zeros((H * W, 3), F)
    flow[:, :2] = rng.normal(0, scale, (H * W, 2))
    flow[:, 2] = rng.random(H * W) > 0.2
    return rng, flow


_cases = {}


def color_case(H, W, scale):
    """(flow (H,W,3) [U,V,valid], the flat indices of the planted pixels): a random real-valued field with a fifth of the
    mask off and the planted rows at random places (as many as fit).  Made once and shared: nobody writes to it."""
    key = ("color", H, W, scale)
    if key not in _cases:
        rng, flow = _random_flow(H, W, scale, 0)
        rows = color_planted()
        where = rng.permutation(H * W)[:min(len(rows), H * W)]
        flow[where] = rows[:len(where)]
        _cases[key] = (flow.reshape(H, W, 3), where)
    return _cases[key]


def dydx(flow):
    """The [U,V,valid] field as [dy,dx] (every pixel then counts as valid)."""
    return np.ascontiguousarray(flow[..., 1::-1])


def warp_case(H, W, scale):
    """(img1, img2, flow (H,W,3), the flat indices of the planted pixels): two random images, a random real-valued flow and,
    as many as fit: a target exactly on the last column (inside) and one float32 step beyond it (outside), the same for the
    last row, zero and signed-zero flows, half-pixel flows, and the unknown kinds."""
    key = ("warp", H, W, scale)
    if key not in _cases:
        rng, flow = _random_flow(H, W, scale, 1)
        img1, img2 = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
        n = H * W
        beyond = int(rng.integers(H)) * W                   # a pixel of column 0: xs = U there
        rest = [int(p) for p in rng.permutation(n) if p != beyond]
        up = lambda v: np.nextafter(F(v), F(np.inf))
        nan, inf = F(np.nan), F(np.inf)
        kinds = [lambda x, y: (W - 1 - x, 0, 1), lambda x, y: (0, H - 1 - y, 1), lambda x, y: (0, 0, 1), lambda x, y: (nan, 0, 1),
                 lambda x, y: (1, 1, 0), lambda x, y: (0, inf, 1), lambda x, y: (2e9, 0, 1), lambda x, y: (-0.0, -0.0, 1),
                 lambda x, y: (0.5 if x + 1 < W else -0.5, 0.5 if y + 1 < H else -0.5, 1), lambda x, y: (-x, -y, 1),
                 lambda x, y: (-x - 0.25, 0, 1), lambda x, y: (0, up(H - 1 - y) if y == 0 else H, 1), lambda x, y: (-1e9, 0, 1)]
        where = [beyond] + rest[:min(len(kinds), n - 1)]
        flow[beyond] = (up(W - 1), 0, 1)
        for p, kind in zip(where[1:], kinds):
            flow[p] = kind(p % W, p // W)
        _cases[key] = (img1, img2, flow.reshape(H, W, 3), np.array(where))
    return _cases[key]
