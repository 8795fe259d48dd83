"""Numpy restatement of the match pre-filter that dflow_epic_prefilter computes (DESIGN.md "Match pre-filter"), written from
the definition, not from the HIP code, on top of epic_ref.voronoi / seed_graph / neighbour_list.  saliency(img, dtype)
evaluates stage A in float64 (the reference) or float32 (the yardstick that says how far a float32 evaluation may drift);
stage B is float64 throughout."""
import numpy as np

import epic_ref as ER
from variational_ref import _shift, gauss_taps

DEFAULTS = dict(saliency_th=0.045, pref_nn=25, pref_th=5.0, k=0.8)     # EpicFlow's, recalled, not checked against the binary
SIGMA_IMAGE, SIGMA_TENSOR = 0.8, 1.0
NONE, KEPT, SALIENCY, CONSISTENCY = 0, 1, 2, 3


def _smooth(f, sigma, dt):
    """Separable Gaussian of a (H,W) plane, along x then along y, taps summed from -r to r, replicate border."""
    taps = gauss_taps(sigma).astype(dt)
    r = len(taps) // 2
    for axis in (1, 0):
        acc = np.zeros_like(f)
        for i in range(-r, r + 1):
            acc = acc + taps[i + r] * _shift(f, i, axis)
        f = acc
    return f


def saliency(img, dt=np.float64):
    """(H,W,3) uint8 BGR -> (H,W) dt: s = sqrt(max(0, lambda_min)) of the smoothed structure tensor."""
    img = np.asarray(img)
    J = [None, None, None]
    for c in range(3):
        f = _smooth(img[..., c].astype(dt), SIGMA_IMAGE, dt)
        fx = dt(0.5) * (_shift(f, 1, 1) - _shift(f, -1, 1))
        fy = dt(0.5) * (_shift(f, 1, 0) - _shift(f, -1, 0))
        for i, prod in enumerate((fx * fx, fx * fy, fy * fy)):
            J[i] = prod if c == 0 else J[i] + prod
    jxx, jxy, jyy = (_smooth(j, SIGMA_TENSOR, dt) for j in J)
    d = jxx - jyy
    lmin = dt(0.5) * (jxx + jyy) - np.sqrt(dt(0.25) * (d * d) + jxy * jxy)
    return np.sqrt(np.maximum(dt(0), lmin))


def estimate(sparse, lst, k):
    """(u^, v^) in float64 from a neighbour list [(id, G)] without its first entry; None when there is no other entry."""
    flat = np.asarray(sparse, np.float32).reshape(-1, 3)
    if len(lst) < 2:
        return None
    sw = su = sv = 0.0
    for t, g in lst[1:]:                                 # list order
        w = float(np.exp(-(k * float(g)) / 2000.0))
        sw += w; su += w * float(flat[t, 0]); sv += w * float(flat[t, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(su) / np.float64(sw)), float(np.float64(sv) / np.float64(sw))


def judge(mid, graph, sd, pref_nn, k):
    """(u^, v^, |estimate - flow|) in float64 of seed sd of the stage-A survivors `mid` over their seed graph; a seed with
    no other seed in reach gets its own flow and 0."""
    flat = np.asarray(mid, np.float32).reshape(-1, 3)
    lst = ER.neighbour_list(graph, sd, pref_nn + 1)
    assert lst[0] == (sd, 0)
    u, v = float(flat[sd, 0]), float(flat[sd, 1])
    e = estimate(mid, lst, k) or (u, v)
    return e[0], e[1], float(np.sqrt((e[0] - u) ** 2 + (e[1] - v) ** 2))


def dropped(mid, sd, eu, ev, pref_th):
    """The decision itself, as the definition writes it: (u^ - u)^2 + (v^ - v)^2 > pref_th^2 in double."""
    flat = np.asarray(mid, np.float32).reshape(-1, 3)
    u, v = float(flat[sd, 0]), float(flat[sd, 1])
    return (eu - u) * (eu - u) + (ev - v) * (ev - v) > pref_th * pref_th


def prefilter(sparse, edges, img1=None, saliency_th=0.045, pref_nn=25, pref_th=5.0, k=0.8):
    """dict: out (H,W,3) float32, reason (H,W) uint8, saliency (H,W) float64 (None when stage A is skipped), mid (the
    stage-A survivors), estimate (H,W,2) float64, dist {seed: |estimate - flow|} for the seeds of stage B."""
    sp = np.asarray(sparse, np.float32)
    H, W = sp.shape[:2]
    seeds = ER.seed_mask(sp)
    reason = np.where(seeds, KEPT, NONE).astype(np.uint8)
    s = None
    if saliency_th != 0:
        s = saliency(img1)
        reason[seeds & (s < saliency_th)] = SALIENCY
    mid = sp.copy()
    mid[reason == SALIENCY] = 0
    est = np.zeros((H, W, 2))
    dist = {}
    if pref_nn > 0 and (reason == KEPT).any():
        S, D = ER.voronoi(mid, edges)
        graph = ER.seed_graph(S, D, edges)
        for sd in np.flatnonzero((reason == KEPT).ravel()).tolist():
            eu, ev, dist[sd] = judge(mid, graph, sd, pref_nn, k)
            est.reshape(-1, 2)[sd] = (eu, ev)
            if dropped(mid, sd, eu, ev, pref_th):
                reason.ravel()[sd] = CONSISTENCY
    out = sp.copy()
    out[reason >= SALIENCY] = 0
    return dict(out=out, reason=reason, saliency=s, mid=mid, estimate=est, dist=dist)
