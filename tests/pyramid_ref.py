"""dflow_pyr_down and dflow_flow_upsample (include/dflow.h) in numpy: the definitions the device is compared against bit for
bit.  The image level is integer arithmetic with one rounding at the end, formed here as the full 5x5 sum (not separably); the
flow is float32 with the written operation order, one rounding per operation."""
import numpy as np

UVV, DYDX = 0, 1                  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX
K = (1, 4, 6, 4, 1)


def coarse_size(h, w):
    return (h + 1) // 2, (w + 1) // 2


def pyr_down(img):
    """(h,w,3) uint8 -> ((h+1)//2, (w+1)//2, 3) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w, _ = img.shape
    hc, wc = coarse_size(h, w)
    a = img.astype(np.int64)
    ys, xs = 2 * np.arange(hc), 2 * np.arange(wc)
    acc = np.zeros((hc, wc, 3), np.int64)
    for i in range(-2, 3):
        rows = a[np.clip(ys + i, 0, h - 1)]
        for j in range(-2, 3):
            acc += K[i + 2] * K[j + 2] * rows[:, np.clip(xs + j, 0, w - 1)]
    return ((acc + 128) >> 8).astype(np.uint8)


def flow_upsample(coarse, size):
    """coarse (hc,wc,2) [dy,dx] or (hc,wc,3) [U,V,valid] float32, size = (h,w) with coarse_size(h,w) == (hc,wc)
    -> ((h,w,3) float32 [U,V,valid], [bilinear, nearest, invalid]).  Elementwise float32 numpy: one rounding per operation."""
    coarse = np.asarray(coarse)
    assert coarse.dtype == np.float32
    h, w = size
    hc, wc = coarse_size(h, w)
    assert coarse.shape[:2] == (hc, wc), (coarse.shape, size)
    if coarse.shape[2] == 3:                              # UVV
        U, V, ok = coarse[..., 0], coarse[..., 1], coarse[..., 2] > np.float32(0.5)      # a NaN compares false
    else:                                                 # DYDX
        U, V, ok = coarse[..., 1], coarse[..., 0], np.ones((hc, wc), bool)
    ok = ok & np.isfinite(U) & np.isfinite(V)             # GOOD
    ys, xs = np.arange(h), np.arange(w)
    y0, y1 = ys >> 1, np.minimum((ys + 1) >> 1, hc - 1)
    x0, x1 = xs >> 1, np.minimum((xs + 1) >> 1, wc - 1)

    def corners(a):
        return a[y0][:, x0], a[y0][:, x1], a[y1][:, x0], a[y1][:, x1]
    g00, g01, g10, g11 = corners(ok)
    half, two = np.float32(0.5), np.float32(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        bil, near = [], []
        for a in (U, V):
            a00, a01, a10, a11 = corners(a)
            bil.append(((a00 + a01) + (a10 + a11)) * half)
            near.append(two * a00)
    for a in bil + near:
        assert a.dtype == np.float32
    is_bil = g00 & g01 & g10 & g11 & np.isfinite(bil[0]) & np.isfinite(bil[1])
    is_near = ~is_bil & g00 & np.isfinite(near[0]) & np.isfinite(near[1])
    out = np.zeros((h, w, 3), np.float32)
    for k in (0, 1):
        out[..., k] = np.where(is_bil, bil[k], np.where(is_near, near[k], np.float32(0.0)))
    out[..., 2] = (is_bil | is_near).astype(np.float32)
    nb, nn = int(is_bil.sum()), int(is_near.sum())
    return out, [nb, nn, h * w - nb - nn]


def compose(O, levels, img1, img2, bcd_times, seed=0, f16=False, coarse_bcd_times=None, prior_stride=2, seed_labels=True):
    """PyramidFlow.run on the CPU.  O: the oracle module; levels: pipeline.pyramid_levels' list (level 0 the finest).  Per level,
    from the coarsest: pyr_down's images, the oracle's front end (on descriptors rounded to binary16 with f16), for every level
    but the coarsest prior_ref.prior_proposals on flow_upsample of the next coarser level, then the oracle's sweeps.  Returns one dict
    per level: bestlabels (H,W) int64, flow (H,W,2) float64 [dy,dx], and where there was a prior its counts."""
    import prior_ref
    imgs = [(np.ascontiguousarray(img1), np.ascontiguousarray(img2))]
    for _ in levels[1:]:
        imgs.append(tuple(pyr_down(a) for a in imgs[-1]))
    out, prior = [None] * len(levels), None
    for level in range(len(levels) - 1, -1, -1):
        g = dict(levels[level])
        p = O.make_params(g.pop("pich"), g.pop("picw"), g.pop("cellh"), g.pop("cellw"), seed=seed,
                          **{k: v for k, v in g.items() if k not in ("flags", "label_pitch")})
        d1, d2 = (O.daisy(a) for a in imgs[level])
        if f16:
            d1, d2 = (d.astype(np.float16).astype(np.float32) for d in (d1, d2))
        proposals, lcosts, nprop, bestlabels = O.knn_proposals(p, d1, d2)
        O.neighbour_proposals(p, d1, d2, proposals, lcosts, nprop, bestlabels)
        res = {}
        if prior is not None:
            packed = ((proposals[..., 0] & 0xFFFF) | ((proposals[..., 1] & 0xFFFF) << 16)).astype(np.uint32)
            lc = lcosts.astype(np.float32)
            assert np.array_equal(lc.astype(np.float64), lcosts)
            res["upsample_counts"] = prior[1]
            res["prior_counts"] = prior_ref.prior_proposals(packed, lc, nprop, bestlabels, d1, d2, prior[0], prior_stride,
                                                            prior_ref.SEED_LABELS if seed_labels else 0, p.maxnprop, p.tphi)
            proposals[..., 0] = (packed & 0xFFFF).astype(np.uint16).view(np.int16)
            proposals[..., 1] = (packed >> 16).astype(np.uint16).view(np.int16)
            lcosts[...] = lc
        for _ in range(bcd_times if level == 0 or coarse_bcd_times is None else coarse_bcd_times):
            O.bcd_sweep(p, proposals, lcosts, nprop, bestlabels)
        res.update(bestlabels=bestlabels, flow=O.labels_to_flow(p, proposals, bestlabels), nprop=nprop)
        out[level] = res
        if level > 0:
            prior = flow_upsample(res["flow"].astype(np.float32), (levels[level - 1]["pich"], levels[level - 1]["picw"]))
    return out


# The reach case of the tests: a 96x128 pair whose second image is the first shifted by (0,+24) with a replicated edge, 8x8 cells and
# window 1 on every level (15 px of reach per level), 2 sweeps.  REACH_PIXELS: the pixels whose final vector is (0,24) with 2
# levels, as compose() gives it (tests/test_pyramid_compose.py recomputes it on the CPU); 96 * (128 - 24) = 9984 pixels have
# their target inside the frame.
REACH = dict(H=96, W=128, cell=8, shift=24, pair_seed=11, seed=3, sweeps=2)
REACH_PIXELS = 7987


def reach_pair(synth):
    img1 = synth.make_pair(REACH["H"], REACH["W"], seed=REACH["pair_seed"])[0]
    img2 = np.ascontiguousarray(img1[:, np.clip(np.arange(REACH["W"]) - REACH["shift"], 0, REACH["W"] - 1)])
    return img1, img2
