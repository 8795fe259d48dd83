"""dflow_frame_interp (include/dflow.h) in numpy: the definition the device is compared against byte for byte.  Every float32
operation is written on its own (one rounding per operation, as the kernels are built with -ffp-contract=off), the keys are
integers.  And the inputs the CPU and the GPU tests share."""
import numpy as np

UVV, DYDX = 0, 1                  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX
F = np.float32
FREE = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("from1", "from2", "filled", "unknown", "blended", "one_sided", "fallback", "lost")


def split(flow):
    """(h,w,3) [U,V,valid] or (h,w,2) [dy,dx] float32 -> U, V, good (valid under its layout, both components finite)."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] in (2, 3)
    if flow.shape[2] == 3:
        U, V, valid = flow[..., 0], flow[..., 1], flow[..., 2]
    else:
        U, V, valid = flow[..., 1], flow[..., 0], np.ones(flow.shape[:2], F)
    with np.errstate(all="ignore"):
        good = (valid > F(0.5)) & np.isfinite(U) & np.isfinite(V)
    return U, V, good


def inside(xs, ys, h, w):
    with np.errstate(all="ignore"):
        return (xs >= F(0)) & (xs <= F(w - 1)) & (ys >= F(0)) & (ys <= F(h - 1))


def bilinear(img, xs, ys, ok):
    """dflow_warp_eval's sample of img (h,w,3) as float32 at the positions where ok (elsewhere the sample of (0,0))."""
    h, w = img.shape[:2]
    xs, ys = np.where(ok, xs, F(0)), np.where(ok, ys, F(0))
    x0f, y0f = np.floor(xs), np.floor(ys)
    ax, ay = (xs - x0f)[..., None], (ys - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    top = (F(1) - ax) * img[y0, x0] + ax * img[y0, x1]
    bot = (F(1) - ax) * img[y1, x0] + ax * img[y1, x1]
    wv = (F(1) - ay) * top + ay * bot
    assert wv.dtype == np.float32
    return wv


def mean_abs_diff(a, b):
    d = np.abs(a - b)
    e = ((d[..., 0] + d[..., 1]) + d[..., 2]) / F(3)
    assert e.dtype == np.float32
    return e


def claims(own, other, flow, step, base):
    """One side's claimants: own, other (h,w,3) float32 pictures, step = t or s -> (target raster indices, keys, count)."""
    h, w = own.shape[:2]
    U, V, good = split(flow)
    yi, xi = np.mgrid[0:h, 0:w]
    xf, yf = xi.astype(F), yi.astype(F)
    with np.errstate(all="ignore"):
        xs, ys = xf + U, yf + V
        part = good & inside(xs, ys, h, w)
        px, py = np.rint(xf + step * U), np.rint(yf + step * V)           # ties to even, as rintf
        part &= inside(px, py, h, w)
    assert px.dtype == np.float32
    e = mean_abs_diff(bilinear(other, xs, ys, part), own)
    idx = (base + yi * w + xi).astype(np.uint64)
    keys = (e.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
    target = (np.where(part, py, F(0)).astype(np.int64) * w + np.where(part, px, F(0)).astype(np.int64))
    return target[part], keys[part], int(part.sum())


def fill_round(m):
    """One Jacobi round on the (h,w,3) field [mU,mV,known]: reads only m."""
    h, w = m.shape[:2]
    out = m.copy()
    todo = m[..., 2] == 0
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):                       # up, left, right, down
        nb = np.zeros_like(m)
        ys, yd = (slice(0, h - 1), slice(1, h)) if dy < 0 else (slice(1, h), slice(0, h - 1)) if dy > 0 else (slice(0, h),) * 2
        xs, xd = (slice(0, w - 1), slice(1, w)) if dx < 0 else (slice(1, w), slice(0, w - 1)) if dx > 0 else (slice(0, w),) * 2
        nb[yd, xd] = m[ys, xs]
        take = todo & (nb[..., 2] != 0)
        out[take] = nb[take]
        todo &= ~take
    return out


def frame_interp(img1, img2, fwd, bwd=None, t=0.5, fill_rounds=8, occl_thresh=30.0):
    """-> dict: out (h,w,3) uint8, keys (h,w) uint64, motion (h,w,3) float32, source (h,w) uint8, counts: list of 8 ints."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    assert img1.dtype == np.uint8 and img2.dtype == np.uint8 and img1.shape == img2.shape and img1.shape[2] == 3
    h, w = img1.shape[:2]
    n = h * w
    t = F(t)
    assert np.isfinite(t) and F(0) < t < F(1) and 0 <= fill_rounds <= 64
    s = F(F(1) - t)
    occl = F(occl_thresh)
    I1, I2 = img1.astype(F), img2.astype(F)

    # A. claimants and winners
    keys = np.full(n, FREE, np.uint64)
    tg, k, nclaim = claims(I1, I2, fwd, t, 0)
    np.minimum.at(keys, tg, k)
    if bwd is not None:
        tg, k, c = claims(I2, I1, bwd, s, n)
        np.minimum.at(keys, tg, k)
        nclaim += c
    keys = keys.reshape(h, w)
    won = keys != FREE
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    from2 = won & (ids >= n)
    from1 = won & ~from2
    motion = np.zeros((h, w, 3), F)
    U, V, _ = split(fwd)
    src1 = ids[from1]
    motion[from1] = np.stack([U.ravel()[src1], V.ravel()[src1], np.ones(src1.size, F)], axis=-1)
    if bwd is not None:
        Ub, Vb, _ = split(bwd)
        src2 = ids[from2] - n
        motion[from2] = np.stack([np.negative(Ub.ravel()[src2]), np.negative(Vb.ravel()[src2]), np.ones(src2.size, F)], axis=-1)
    source = np.where(from1, 1, np.where(from2, 2, 0)).astype(np.uint8)

    # B. fill
    for _ in range(fill_rounds):
        motion = fill_round(motion)
    known = motion[..., 2] != 0
    source[known & ~won] = 3

    # C. render
    yi, xi = np.mgrid[0:h, 0:w]
    xf, yf = xi.astype(F), yi.astype(F)
    mU, mV = motion[..., 0], motion[..., 1]
    with np.errstate(all="ignore"):
        x1, y1 = xf - t * mU, yf - t * mV
        x2, y2 = xf + s * mU, yf + s * mV
        use1, use2 = known & inside(x1, y1, h, w), known & inside(x2, y2, h, w)
    c1, c2 = bilinear(I1, x1, y1, use1), bilinear(I2, x2, y2, use2)
    both = use1 & use2
    agree = both & (mean_abs_diff(c1, c2) <= occl)
    first = np.where(source == 1, True, np.where(source == 2, False, t <= F(0.5)))
    pick1 = (both & ~agree & first) | (use1 & ~use2)
    pick2 = (both & ~agree & ~first) | (use2 & ~use1)
    v = s * I1 + t * I2                                                     # the fallback
    v = np.where(agree[..., None], s * c1 + t * c2, v)
    v = np.where(pick1[..., None], c1, v)
    v = np.where(pick2[..., None], c2, v)
    assert v.dtype == np.float32
    out = np.floor(v + F(0.5)).astype(np.int32).astype(np.uint8)
    one_sided = pick1 | pick2
    counts = [int(from1.sum()), int(from2.sum()), int((source == 3).sum()), int((source == 0).sum()),
              int(agree.sum()), int(one_sided.sum()), int(n - agree.sum() - one_sided.sum()), nclaim - int(won.sum())]
    return dict(out=out, keys=keys, motion=motion, source=source, counts=counts)


def psnr(a, b, mask):
    d = np.asarray(a, np.float64)[mask] - np.asarray(b, np.float64)[mask]
    return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


# ---------------------------------------------------------------------------------- the inputs of the GPU tests
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (33, 65), (64, 257)]
T_VALUES = (0.5, 0.25, float(F(1) / F(3)), 2.0 ** -20, 1.0 - 2.0 ** -20)
FILL_ROUNDS = (0, 1, 8, 64)
OCCL = (0.0, 30.0, 3e38)


def images(h, w, seed):
    """Two pictures that resemble each other (so that errors tie and differ), (h,w,3) uint8."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    b = np.roll(a, (1, 2), (0, 1))
    flip = rng.random((h, w)) < 0.3
    b[flip] = rng.integers(0, 256, (int(flip.sum()), 3)).astype(np.uint8)
    return a, b


def as_layout(uvv, layout):
    """An (h,w,3) [U,V,valid] field in the asked layout; under DYDX an invalid pixel becomes a NaN vector."""
    if layout == UVV:
        return np.ascontiguousarray(uvv)
    d = np.stack([uvv[..., 1], uvv[..., 0]], axis=-1).astype(F)
    d[uvv[..., 2] <= 0.5] = np.nan
    return np.ascontiguousarray(d)


def flow_field(h, w, seed, kind):
    """(h,w,3) float32 [U,V,valid].  'int': integer vectors within a few pixels; 'frac': fractional vectors (quarters, so that
    half-way places occur), 30 % invalid, and a sprinkle of NaN, +-inf and huge vectors; 'one': every source aims at one pixel;
    'none': all invalid."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w, 3), F)
    yi, xi = np.mgrid[0:h, 0:w]
    if kind == "int":
        f[..., 0] = rng.integers(-4, 5, (h, w))
        f[..., 1] = rng.integers(-3, 4, (h, w))
        f[..., 2] = 1
    elif kind == "frac":
        f[..., 0] = rng.integers(-24, 25, (h, w)) / 4.0 + (rng.random((h, w)) < 0.3) * rng.normal(0, 1, (h, w))
        f[..., 1] = rng.integers(-16, 17, (h, w)) / 4.0 + (rng.random((h, w)) < 0.3) * rng.normal(0, 1, (h, w))
        f[..., 2] = rng.random((h, w)) >= 0.3
        odd = rng.random((h, w))
        for lo, val in ((0.00, np.nan), (0.01, np.inf), (0.02, -np.inf), (0.03, 3e38)):
            f[..., rng.integers(0, 2)][(odd >= lo) & (odd < lo + 0.01)] = val
    elif kind == "one":
        ty, tx = h // 2, w // 3
        f[..., 0], f[..., 1], f[..., 2] = (tx - xi) * 2, (ty - yi) * 2, 1        # at t = 0.5 all land on (tx, ty)
    else:
        assert kind == "none"
        f[..., :2] = rng.normal(0, 3, (h, w, 2))
    return f


def edge_case(h=9, w=11):
    """Crafted vectors whose sampling positions land on -0.5, h-1 and h-0.5 (and the same in x) at t = 0.5: identical frames'
    worth of claims with vectors of +-1 and +-2 along the borders.  -> (img1, img2, fwd, bwd) with [U,V,valid] fields."""
    a, b = images(h, w, 99)
    fwd, bwd = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
    fwd[..., 2] = bwd[..., 2] = 1
    fwd[h - 3, :, 1] = 2                # lands on h-2 with motion 2: side 2 samples y = h-1 exactly
    fwd[:, w - 3, 0] = 2                # and x = w-1
    fwd[0, :, 1] = 1                  # row 0 moves down by 1: its place is rint(0.5) = 0, side 1 samples y = -0.5: not inside
    fwd[h - 2, :, 1] = 1                # lands on h-1 exactly; place rint(h - 1.5)
    fwd[h - 1, :, 1] = -1               # from the last row upwards: side 1 samples y = h - 0.5 for a target at h-1
    fwd[:, 0, 0] = 1
    fwd[:, w - 1, 0] = -1
    bwd[h - 1, :, 1] = -2
    bwd[0, :, 1] = 2
    bwd[:, w - 1, 0] = -1
    return a, b, fwd, bwd
