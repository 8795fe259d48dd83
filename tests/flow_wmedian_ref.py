"""The numpy definition of dflow_flow_wmedian (include/dflow.h, DESIGN.md "Weighted median filter"), written from the header's
words and independently of the kernel's method: the samples of every window are sorted by key, their weights summed up in int64,
and the median is the first sample with 2 * cum >= W.  Also the case generators that test_flow_wmedian_ref.py and
test_gpu_flow_wmedian.py share."""
import numpy as np

F = np.float32
UVV, DYDX = 0, 1                  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX
KEEP_HOLES, REJECT = 1, 2         # DFLOW_WMED_KEEP_HOLES, DFLOW_WMED_REJECT
NCOLOR = 766

SHAPES = ((1, 1), (1, 7), (5, 1), (17, 19), (33, 65))
RADII = (1, 3, 8)
KINDS = ("int", "frac", "holes", "zeros", "wide", "const", "none")
REJECTS = (0.0, 1.5, 1e30)


def split(flow):
    """A field in either layout -> (U bits, V bits, good), the bits as uint32 (h,w) planes."""
    flow = np.ascontiguousarray(flow, F)
    if flow.shape[2] == 3:
        U, V, valid = flow[..., 0], flow[..., 1], flow[..., 2]
        good = valid > F(0.5)                                 # a NaN compares false
    else:
        V, U = flow[..., 0], flow[..., 1]
        good = np.ones(U.shape, bool)
    good = good & np.isfinite(U) & np.isfinite(V)
    return np.ascontiguousarray(U).view(np.uint32), np.ascontiguousarray(V).view(np.uint32), good


def keys(bits):
    bits = np.asarray(bits, np.uint32)
    return np.where(bits >> 31 != 0, bits ^ np.uint32(0xFFFFFFFF), bits | np.uint32(0x80000000)).astype(np.uint32)


def as_layout(flow, layout):
    """An (h,w,3) [U,V,valid] field in `layout`; DYDX keeps the vectors and drops the valid plane (every pixel valid)."""
    return flow if layout == UVV else np.ascontiguousarray(flow[..., [1, 0]])


def flow_wmedian(flow, bgr=None, radius=3, wspace=None, wcolor=None, reject_thresh=0.0, flags=0):
    """-> (out (h,w,3) float32, counts [good inputs, valid outputs, filled, altered])."""
    assert (bgr is None) == (wcolor is None)
    ub, vb, good = split(flow)
    h, w = good.shape
    r = radius
    n = 2 * r + 1
    S = np.ones((r + 1, r + 1), np.int64) if wspace is None else np.asarray(wspace, np.uint8).reshape(r + 1, r + 1).astype(np.int64)
    pad = lambda a, fill: np.pad(a, ((r, r), (r, r)), constant_values=fill)
    pg, pu, pv = pad(good, False), pad(keys(ub), 0), pad(keys(vb), 0)
    pub, pvb = pad(ub, 0), pad(vb, 0)
    if bgr is not None:
        img = np.asarray(bgr, np.uint8).astype(np.int64)
        pimg = np.pad(img, ((r, r), (r, r), (0, 0)))
        C = np.asarray(wcolor, np.uint8).astype(np.int64)
        assert C.shape == (NCOLOR,)
    wts = np.zeros((h, w, n * n), np.int64)
    ku, kv, bu, bv = (np.zeros((h, w, n * n), np.uint32) for _ in range(4))
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            k = (dy + r) * n + dx + r
            win = (slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
            wq = np.full((h, w), S[abs(dy), abs(dx)], np.int64)
            if bgr is not None:
                wq = wq * C[np.abs(pimg[win] - img).sum(axis=2)]
            wts[..., k] = np.where(pg[win], wq, 0)            # outside the frame: not good
            ku[..., k], kv[..., k], bu[..., k], bv[..., k] = pu[win], pv[win], pub[win], pvb[win]
    W = wts.sum(axis=2)

    def median(key, bits):
        order = np.argsort(key, axis=2, kind="stable")
        cum = np.cumsum(np.take_along_axis(wts, order, axis=2), axis=2)
        first = np.argmax(2 * cum >= W[..., None], axis=2)
        pick = np.take_along_axis(order, first[..., None], axis=2)
        return np.take_along_axis(bits, pick, axis=2)[..., 0]

    mu, mv = median(ku, bu), median(kv, bv)
    some = W > 0
    one = np.uint32(F(1.0).view(np.uint32))
    out = np.zeros((h, w, 3), np.uint32)
    if flags & REJECT:
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.abs(ub.view(F) - mu.view(F)) + np.abs(vb.view(F) - mv.view(F))
            keep = some & good & (d <= F(reject_thresh))
        out[..., 0], out[..., 1], out[..., 2] = np.where(keep, ub, 0), np.where(keep, vb, 0), np.where(keep, one, 0)
    else:
        keep = some & (good if flags & KEEP_HOLES else True)
        out[..., 0], out[..., 1], out[..., 2] = np.where(keep, mu, 0), np.where(keep, mv, 0), np.where(keep, one, 0)
    valid = out[..., 2] != 0
    altered = good & (~valid | (out[..., 0] != ub) | (out[..., 1] != vb))
    counts = [int(good.sum()), int(valid.sum()), int((valid & ~good).sum()), int(altered.sum())]
    return out.view(F), counts


def tables(radius, sigma_space=None, sigma_color=None):
    """pipeline.wmedian_tables restated: float64, floor(255 e + 0.5)."""
    space = color = None
    if sigma_space is not None:
        d = np.arange(radius + 1, dtype=np.float64)
        space = np.floor(255.0 * np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * sigma_space ** 2)) + 0.5).astype(np.uint8)
    if sigma_color is not None:
        color = np.floor(255.0 * np.exp(-np.arange(NCOLOR, dtype=np.float64) / (3.0 * sigma_color)) + 0.5).astype(np.uint8)
    return space, color


# ---- cases
def image(h, w, seed):
    """A guide of a few flat regions with noise: colour distances from 0 to several hundred."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((yy * 3) // max(h, 1) + (xx * 2) // max(w, 1)) % 4
    base = rng.integers(0, 256, (4, 3))
    return np.clip(base[region] + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def field(h, w, seed, kind):
    """An (h,w,3) [U,V,valid] float32 field of one of KINDS."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    f = np.ones((h, w, 3), F)
    if kind in ("int", "holes", "none"):
        f[..., :2] = rng.integers(-3, 4, (h, w, 2))                       # many ties
    elif kind == "frac":
        f[..., :2] = rng.normal(0, 4, (h, w, 2))
    elif kind == "zeros":
        f[..., :2] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], F), (h, w, 2))
    elif kind == "wide":                                                   # every key bit, both signs
        f[..., :2] = (rng.choice(np.array([-1.0, 1.0]), (h, w, 2)) * 10.0 ** rng.uniform(-30, 30, (h, w, 2))).astype(F)
    elif kind == "const":
        f[..., 0], f[..., 1] = 3.0, -2.0
    if kind == "holes":                                                    # 30 % not good, in every way a pixel can be
        how = rng.random((h, w))
        f[how < 0.10, 2] = 0.0
        f[(how >= 0.10) & (how < 0.20), 0] = np.nan
        f[(how >= 0.20) & (how < 0.25), 1] = np.inf
        f[(how >= 0.25) & (how < 0.30), 1] = -np.inf
    if kind == "none":
        f[..., 2] = 0.0
    return f


def table_sets(radius, seed):
    """name -> (wspace, wcolor): none, space only, colour only, both, with zeros (space[0] == 0), all zeros, all 255."""
    rng = np.random.default_rng([seed, radius])
    space, color = tables(radius, 0.6 * radius + 0.4, 10.0)
    zs = np.zeros((radius + 1, radius + 1), np.uint8)                      # only the window's outermost rows weigh: W == 0 occurs
    zs[radius] = rng.integers(0, 3, radius + 1) * 100
    zs[radius, radius] = 200
    zc = (rng.integers(0, 2, NCOLOR) * rng.integers(1, 256, NCOLOR)).astype(np.uint8)
    full = np.full(NCOLOR, 255, np.uint8)
    return {"none": (None, None), "space": (space, None), "colour": (None, color), "both": (space, color),
            "zeros": (zs, zc), "zero_space": (zs, None), "nothing": (np.zeros_like(zs), None), "full": (np.full((radius + 1, radius + 1), 255, np.uint8), full)}
