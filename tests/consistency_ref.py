"""dflow_flow_consistency (include/dflow.h) in plain numpy loops with np.float32 scalars: the definition the device is compared
against bit for bit, one rounding per written operation.  And compose_pair: PyramidFlow.run_pair composed on the CPU from the
oracle's front end and sweeps, pyramid_ref, prior_ref and the check defined here."""
import numpy as np

UVV, DYDX = 0, 1                  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX
BILINEAR = 1                      # DFLOW_FBC_BILINEAR
CONSISTENT, ABOVE, BWD_INVALID, OUTSIDE, FWD_INVALID = range(5)      # the order of d_counts
F = np.float32


def good_vector(field, y, x):
    """(V, U) = (dy, dx) of pixel (y,x) as np.float32, or None: invalid under [U,V,valid] (a NaN compares false) or a component
    that is not finite."""
    q = field[y, x]
    if q.shape[0] == 3:
        if not (q[2] > F(0.5)):
            return None
        v, u = q[1], q[0]
    else:
        v, u = q[0], q[1]
    if not (np.isfinite(v) and np.isfinite(u)):
        return None
    return v, u


@np.errstate(over="ignore", invalid="ignore")
def classify(fwd, bwd, y, x, thresh, flags):
    """Pixel (y,x) of fwd against bwd -> (class, err): err an np.float32 for ABOVE and CONSISTENT, else None."""
    h, w = fwd.shape[:2]
    g = good_vector(fwd, y, x)
    if g is None:
        return FWD_INVALID, None
    V, U = g
    if flags & BILINEAR:
        py, px = F(F(y) + V), F(F(x) + U)
        if not (py >= F(0) and py <= F(h - 1) and px >= F(0) and px <= F(w - 1)):
            return OUTSIDE, None
        y0, x0 = int(np.floor(py)), int(np.floor(px))
        ay, ax = F(py - F(y0)), F(px - F(x0))
        y1 = y0 + 1 if ay > F(0) else y0
        x1 = x0 + 1 if ax > F(0) else x0
        c = [good_vector(bwd, yy, xx) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
        if any(v is None for v in c):
            return BWD_INVALID, None
        b = []
        for k in (0, 1):                                              # bv, then bu
            a00, a01, a10, a11 = (v[k] for v in c)
            t = F(a00 + F(ax * F(a01 - a00)))
            bt = F(a10 + F(ax * F(a11 - a10)))
            b.append(F(t + F(ay * F(bt - t))))
        bv, bu = b
    else:
        ry, rx = np.rint(V), np.rint(U)                               # ties to even, as rintf
        if abs(float(ry)) > 32767.0 or abs(float(rx)) > 32767.0:
            return OUTSIDE, None
        ty, tx = y + int(ry), x + int(rx)
        if not (0 <= ty < h and 0 <= tx < w):
            return OUTSIDE, None
        g = good_vector(bwd, ty, tx)
        if g is None:
            return BWD_INVALID, None
        bv, bu = g
    du, dv = F(U + bu), F(V + bv)
    err = np.sqrt(F(F(du * du) + F(dv * dv)))
    assert err.dtype == np.float32
    return (CONSISTENT if err <= thresh else ABOVE), err              # a NaN err compares false: ABOVE


def one_direction(fwd, bwd, thresh, flags=0):
    """fwd, bwd (h,w,2) [dy,dx] or (h,w,3) [U,V,valid] float32 -> (out (h,w,3) [U,V,valid], err (h,w), counts[5], cls (h,w))."""
    fwd, bwd = np.asarray(fwd), np.asarray(bwd)
    assert fwd.dtype == np.float32 and bwd.dtype == np.float32 and fwd.shape[:2] == bwd.shape[:2]
    h, w = fwd.shape[:2]
    thresh = F(thresh)
    out, err = np.zeros((h, w, 3), np.float32), np.full((h, w), -1.0, np.float32)
    cls = np.zeros((h, w), np.int8)
    counts = [0] * 5
    iu, iv = (0, 1) if fwd.shape[2] == 3 else (1, 0)
    with np.errstate(over="ignore", invalid="ignore"):
        for y in range(h):
            for x in range(w):
                k, e = classify(fwd, bwd, y, x, thresh, flags)
                counts[k] += 1
                cls[y, x] = k
                if e is not None:
                    err[y, x] = e
                if k == CONSISTENT:
                    out[y, x, 0], out[y, x, 1], out[y, x, 2] = fwd[y, x, iu], fwd[y, x, iv], 1.0       # its own bits
    return out, err, counts, cls


def flow_consistency(fwd, bwd, thresh, flags=0, both=False):
    """One direction: (out, err, counts[5]); both: (out_fwd, out_bwd, err_fwd, err_bwd, counts[10])."""
    f = one_direction(fwd, bwd, thresh, flags)
    if not both:
        return f[:3]
    b = one_direction(bwd, fwd, thresh, flags)
    return f[0], b[0], f[1], b[1], f[2] + b[2]


def compose_pair(O, levels, img1, img2, bcd_times, seed=0, coarse_bcd_times=None, gate=None, gate_bilinear=False, prior_stride=2,
                 seed_labels=True):
    """PyramidFlow.run_pair on the CPU.  O: the oracle module; levels: pipeline.pyramid_levels' list (level 0 the finest).  Per
    level, from the coarsest, forward and then backward (the images swapped): the oracle's front end, prior_ref.prior_proposals
    on pyramid_ref.flow_upsample of the next coarser level's flow, the oracle's sweeps; with gate=T the two flows of a coarse
    level go through flow_consistency(both) first.  Returns per level a pair (forward, backward) of dicts: bestlabels, flow
    (H,W,2) float64 [dy,dx]; on the coarse levels with a gate also gate_counts, the int[5] of that direction."""
    import prior_ref
    import pyramid_ref
    imgs = [(np.ascontiguousarray(img1), np.ascontiguousarray(img2))]
    for _ in levels[1:]:
        imgs.append(tuple(pyramid_ref.pyr_down(a) for a in imgs[-1]))
    out, priors = [None] * len(levels), (None, None)
    for level in range(len(levels) - 1, -1, -1):
        g = dict(levels[level])
        p = O.make_params(g.pop("pich"), g.pop("picw"), g.pop("cellh"), g.pop("cellw"), seed=seed,
                          **{k: v for k, v in g.items() if k not in ("flags", "label_pitch")})
        descr = [O.daisy(a) for a in imgs[level]]
        res = []
        for prior, (d1, d2) in zip(priors, ((descr[0], descr[1]), (descr[1], descr[0]))):
            proposals, lcosts, nprop, bestlabels = O.knn_proposals(p, d1, d2)
            O.neighbour_proposals(p, d1, d2, proposals, lcosts, nprop, bestlabels)
            r = {}
            if prior is not None:
                packed = ((proposals[..., 0] & 0xFFFF) | ((proposals[..., 1] & 0xFFFF) << 16)).astype(np.uint32)
                lc = lcosts.astype(np.float32)
                assert np.array_equal(lc.astype(np.float64), lcosts)
                r["prior_counts"] = prior_ref.prior_proposals(packed, lc, nprop, bestlabels, d1, d2, prior, prior_stride,
                                                              prior_ref.SEED_LABELS if seed_labels else 0, p.maxnprop, p.tphi)
                proposals[..., 0] = (packed & 0xFFFF).astype(np.uint16).view(np.int16)
                proposals[..., 1] = (packed >> 16).astype(np.uint16).view(np.int16)
                lcosts[...] = lc
            for _ in range(bcd_times if level == 0 or coarse_bcd_times is None else coarse_bcd_times):
                O.bcd_sweep(p, proposals, lcosts, nprop, bestlabels)
            r.update(bestlabels=bestlabels, flow=O.labels_to_flow(p, proposals, bestlabels))
            res.append(r)
        out[level] = tuple(res)
        if level > 0:
            flows = [r["flow"].astype(np.float32) for r in res]
            if gate is not None:
                gf, gb, _, _, counts = flow_consistency(flows[0], flows[1], gate, BILINEAR if gate_bilinear else 0, both=True)
                res[0]["gate_counts"], res[1]["gate_counts"] = counts[:5], counts[5:]
                flows = [gf, gb]
            size = (levels[level - 1]["pich"], levels[level - 1]["picw"])
            priors = tuple(pyramid_ref.flow_upsample(f, size)[0] for f in flows)
    return out
