"""Independent numpy restatement of the edge-aware interpolation that dflow_epic_interpolate computes (EpicFlow's
sparse-to-dense step with integer geodesics, DESIGN.md "EpicFlow interpolation").  Written from the definition, not from
the HIP code: a heapq Dijkstra for the Voronoi diagram, a vectorised fixed-point verifier that proves a diagram exact at any
size, a numpy seed-graph builder, a per-seed heapq Dijkstra for the neighbour lists and the NW / LA fit in float64."""
import heapq
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the eigenvalue threshold of the LA fit, px^2: the one the kernel is compiled with
TAU = float(re.search(r"#define\s+DFLOW_EPIC_TAU\s+(\S+)", open(os.path.join(ROOT, "include", "dflow.h")).read()).group(1))
INF = np.iinfo(np.uint64).max


def seed_mask(sparse):
    s = np.asarray(sparse, np.float32)
    return (s[..., 2] > 0.5) & np.isfinite(s[..., 0]) & np.isfinite(s[..., 1])


def costs(edges):
    """c = 1 + rint(1000 e), e = clamp(E, 0, 1) with NaN read as 1; the product in float32."""
    e = np.asarray(edges, np.float32)
    e = np.where(np.isnan(e), np.float32(1), np.clip(e, np.float32(0), np.float32(1))).astype(np.float32)
    return 1 + np.rint(np.float32(1000) * e).astype(np.int64)


def _neighbours(p, H, W):
    y, x = divmod(p, W)
    if x > 0:
        yield p - 1
    if x + 1 < W:
        yield p + 1
    if y > 0:
        yield p - W
    if y + 1 < H:
        yield p + W


def voronoi(sparse, edges):
    """(S, D): (H,W) int64 seed ids (-1 without seeds) and geodesic distances (0xFFFFFFFF without seeds), by a heapq
    Dijkstra over (D, seed id) keys."""
    seeds = seed_mask(sparse)
    H, W = seeds.shape
    c = costs(edges).ravel()
    S = np.full(H * W, -1, np.int64)
    D = np.full(H * W, 0xFFFFFFFF, np.int64)
    heap = [(0, int(p), int(p)) for p in np.flatnonzero(seeds.ravel())]
    heapq.heapify(heap)
    done = np.zeros(H * W, bool)
    while heap:
        d, s, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p] = True
        S[p], D[p] = s, d
        for q in _neighbours(p, H, W):
            if not done[q]:
                heapq.heappush(heap, (d + int(c[p]) + int(c[q]), s, q))
    return S.reshape(H, W), D.reshape(H, W)


def verify_fixed_point(sparse, edges, S, D):
    """None if (S, D) is THE diagram: key(seed) = (0, id) and key(p) = min over 4-neighbours q of key(q) + c(p) + c(q)
    everywhere else (positive integer steps make that fixed point unique); otherwise a message naming the first bad pixel."""
    seeds = seed_mask(sparse)
    H, W = seeds.shape
    S = np.asarray(S).astype(np.int64)
    D = np.asarray(D).astype(np.int64) & 0xFFFFFFFF
    if not seeds.any():
        return None if (S == -1).all() and (D == 0xFFFFFFFF).all() else "no seed, yet S / D are not empty"
    if (S < 0).any() or (S >= H * W).any() or not seeds.ravel()[S.ravel()].all():
        return "S names a pixel that is not a seed"
    c = costs(edges)
    key = (D.astype(np.uint64) << np.uint64(32)) | S.astype(np.uint64)
    best = np.full((H, W), INF, np.uint64)

    def relax(dst, src):                                # best[dst] = min(best[dst], key(src) + step)
        cand = ((D[src] + c[src] + c[dst]).astype(np.uint64) << np.uint64(32)) | S[src].astype(np.uint64)
        best[dst] = np.minimum(best[dst], cand)
    a, b = slice(1, None), slice(None, -1)
    if W > 1:
        relax((slice(None), a), (slice(None), b))
        relax((slice(None), b), (slice(None), a))
    if H > 1:
        relax((a, slice(None)), (b, slice(None)))
        relax((b, slice(None)), (a, slice(None)))
    ids = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    want = np.where(seeds, ids, best)
    bad = np.argwhere(want != key)
    if bad.size:
        y, x = bad[0]
        return "%d pixels off the fixed point, first (y=%d, x=%d): key (%d, %d), want (%d, %d)" % (
            len(bad), y, x, D[y, x], S[y, x], int(want[y, x]) >> 32, int(want[y, x]) & 0xFFFFFFFF)
    return None


def seed_graph(S, D, edges):
    """{s: {t: w}} with w the minimum over 4-neighbour pairs p, q with S(p) = s != t = S(q) of D(p) + c(p) + c(q) + D(q)."""
    S = np.asarray(S).astype(np.int64)
    D = np.asarray(D).astype(np.int64)
    c = costs(edges)
    a, b, w = [], [], []
    for sp, sq in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                   ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        m = S[sp] != S[sq]
        a.append(S[sp][m]); b.append(S[sq][m]); w.append((D[sp] + c[sp] + c[sq] + D[sq])[m])
    a, b, w = (np.concatenate(v) for v in (a, b, w))
    s, t, w = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    order = np.lexsort((w, t, s))                       # per (s, t) the smallest weight first
    s, t, w = s[order], t[order], w[order]
    first = np.ones(len(s), bool)
    first[1:] = (s[1:] != s[:-1]) | (t[1:] != t[:-1])
    graph = {}
    for si, ti, wi in zip(s[first].tolist(), t[first].tolist(), w[first].tolist()):
        graph.setdefault(si, {})[ti] = wi
    return graph


def neighbour_list(graph, s, nn):
    """[(id, G)]: the nn seeds nearest to s by (G, id) in the seed graph, s itself first, by a heapq Dijkstra."""
    out, done, heap = [], set(), [(0, s)]
    while heap and len(out) < nn:
        g, t = heapq.heappop(heap)
        if t in done:
            continue
        done.add(t)
        out.append((t, g))
        for u, w in graph.get(t, {}).items():
            if u not in done:
                heapq.heappush(heap, (g + w, u))
    return out


def fit(sparse, s, lst, k, method):
    """(model, lambda_min): model = (u0, u_x, u_y, v0, v_x, v_y) in float64 for seed s from its list; lambda_min the
    smallest eigenvalue of the weighted position covariance (None when the list is shorter than 3)."""
    sp = np.asarray(sparse, np.float32)
    W = sp.shape[1]
    ys, xs = divmod(s, W)
    sw = sx = sy = sxx = sxy = syy = su = sv = sxu = syu = sxv = syv = 0.0
    for t, g in lst:                                    # list order
        w = 1.0 if t == s else float(np.exp(-(k * float(g)) / 2000.0))
        ty, tx = divmod(t, W)
        dx, dy = float(tx - xs), float(ty - ys)
        u, v = float(sp[ty, tx, 0]), float(sp[ty, tx, 1])
        wx, wy = w * dx, w * dy
        sw += w; sx += wx; sy += wy; sxx += wx * dx; sxy += wx * dy; syy += wy * dy
        su += w * u; sv += w * v; sxu += wx * u; syu += wy * u; sxv += wx * v; syv += wy * v
    mu, mv = su / sw, sv / sw
    model = (mu, 0.0, 0.0, mv, 0.0, 0.0)
    lmin = None
    if len(lst) >= 3:
        mx, my = sx / sw, sy / sw
        cxx, cxy, cyy = sxx / sw - mx * mx, sxy / sw - mx * my, syy / sw - my * my
        h = 0.5 * (cxx - cyy)
        lmin = 0.5 * (cxx + cyy) - np.sqrt(h * h + cxy * cxy)
        if method == "LA" and lmin >= TAU:
            det = cxx * cyy - cxy * cxy
            cxu, cyu = sxu / sw - mx * mu, syu / sw - my * mu
            cxv, cyv = sxv / sw - mx * mv, syv / sw - my * mv
            bu, cu = (cyy * cxu - cxy * cyu) / det, (cxx * cyu - cxy * cxu) / det
            bv, cv = (cyy * cxv - cxy * cyv) / det, (cxx * cyv - cxy * cxv) / det
            model = (mu - bu * mx - cu * my, bu, cu, mv - bv * mx - cv * my, bv, cv)
    return model, lmin


def list_arrays(lists, seeds, nn):
    """{s: [(id, G)]} -> (ids, G): (len(seeds), nn) int64 arrays in the order of `seeds`, -1 pads after a short list."""
    ids = np.full((len(seeds), nn), -1, np.int64)
    G = np.full((len(seeds), nn), -1, np.int64)
    for i, s in enumerate(seeds):
        l = lists[s][:nn]
        ids[i, :len(l)] = [t for t, _ in l]
        G[i, :len(l)] = [g for _, g in l]
    return ids, G


def fit_prefixes(sparse, seeds, ids, G, k, nns):
    """fit() of every seed of `seeds` on the first nn entries of its list, for every nn of nns, in one pass over the list
    positions: the sums grow entry by entry in list order, so the operations and their order are those of fit(), one seed
    per array element.  ids, G as list_arrays() gives them.  {nn: {"NW": (n,6), "LA": (n,6), "lmin": (n,)}} in float64; lmin
    is NaN where the list is shorter than 3."""
    sp = np.asarray(sparse, np.float32)
    W = sp.shape[1]
    flat = sp.reshape(-1, 3).astype(np.float64)
    seeds = np.asarray(seeds, np.int64)
    n = len(seeds)
    xs, ys = seeds % W, seeds // W
    sw, sx, sy, sxx, sxy, syy, su, sv, sxu, syu, sxv, syv = (np.zeros(n) for _ in range(12))
    count = np.zeros(n, np.int64)
    out = {}
    for j in range(max(nns)):
        live = ids[:, j] >= 0
        t = np.where(live, ids[:, j], 0)
        with np.errstate(over="ignore"):
            w = np.exp(-(k * G[:, j].astype(np.float64)) / 2000.0)
        w = np.where(live, np.where(t == seeds, 1.0, w), 0.0)
        dx, dy = (t % W - xs).astype(np.float64), (t // W - ys).astype(np.float64)
        u, v = np.where(live, flat[t, 0], 0.0), np.where(live, flat[t, 1], 0.0)
        wx, wy = w * dx, w * dy
        sw += w; sx += wx; sy += wy; sxx += wx * dx; sxy += wx * dy; syy += wy * dy
        su += w * u; sv += w * v; sxu += wx * u; syu += wy * u; sxv += wx * v; syv += wy * v
        count += live
        if j + 1 not in nns:
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            mu, mv = su / sw, sv / sw
            zero = np.zeros(n)
            nw = np.stack([mu, zero, zero, mv, zero, zero], axis=1)
            mx, my = sx / sw, sy / sw
            cxx, cxy, cyy = sxx / sw - mx * mx, sxy / sw - mx * my, syy / sw - my * my
            h = 0.5 * (cxx - cyy)
            lmin = np.where(count >= 3, 0.5 * (cxx + cyy) - np.sqrt(h * h + cxy * cxy), np.nan)
            det = cxx * cyy - cxy * cxy
            cxu, cyu = sxu / sw - mx * mu, syu / sw - my * mu
            cxv, cyv = sxv / sw - mx * mv, syv / sw - my * mv
            bu, cu = (cyy * cxu - cxy * cyu) / det, (cxx * cyu - cxy * cxu) / det
            bv, cv = (cyy * cxv - cxy * cyv) / det, (cxx * cyv - cxy * cxv) / det
            affine = np.stack([mu - bu * mx - cu * my, bu, cu, mv - bv * mx - cv * my, bv, cv], axis=1)
            la = np.where((lmin >= TAU)[:, None], affine, nw)
        out[j + 1] = {"NW": nw, "LA": la, "lmin": lmin}
    return out


def fill_plane(S, seeds, models, dt=np.float64):
    """fill() for models given as an (n,6) array in the order of `seeds`, evaluated in dt: float64 as fill() does, or
    float32 on the models rounded to float32, in the written order (m0 + m1 dx) + m2 dy: the float32 yardstick."""
    H, W = S.shape
    index = np.full(H * W + 1, len(seeds), np.int64)      # S = -1 reads the zero model appended below
    index[np.asarray(seeds, np.int64)] = np.arange(len(seeds))
    Sf = S.ravel()
    m = np.concatenate([np.asarray(models, np.float64), np.zeros((1, 6))]).astype(dt)[index[Sf]]
    ys, xs = np.divmod(np.arange(H * W), W)
    dx, dy = np.where(Sf >= 0, xs - Sf % W, 0).astype(dt), np.where(Sf >= 0, ys - Sf // W, 0).astype(dt)
    flow = np.zeros((H * W, 2), dt)
    flow[:, 1] = (m[:, 0] + m[:, 1] * dx) + m[:, 2] * dy
    flow[:, 0] = (m[:, 3] + m[:, 4] * dx) + m[:, 5] * dy
    return flow.reshape(H, W, 2)


def interpolate(sparse, edges, nn=100, k=0.8, method="LA"):
    """The whole step: dict with flow (H,W,2) float64 [dy,dx], S, D, lists {s: [(id, G)]}, lmin {s: lambda_min}."""
    sp = np.asarray(sparse, np.float32)
    H, W = sp.shape[:2]
    S, D = voronoi(sp, edges)
    flow = np.zeros((H, W, 2))
    res = {"S": S, "D": D, "lists": {}, "lmin": {}, "flow": flow}
    if (S < 0).all():
        return res
    graph = seed_graph(S, D, edges)
    models = {}
    for s in np.flatnonzero(seed_mask(sp).ravel()).tolist():
        lst = neighbour_list(graph, s, nn)
        res["lists"][s] = lst
        models[s], res["lmin"][s] = fit(sp, s, lst, k, method)
    res["flow"] = fill(S, models)
    return res


def fill(S, models):
    """(H,W,2) float64 [dy,dx]: every pixel evaluates its seed's model at its own offset from the seed."""
    H, W = S.shape
    flow = np.zeros((H, W, 2))
    ys, xs = np.divmod(np.arange(H * W), W)
    Sf = S.ravel()
    for s, m in models.items():
        sel = Sf == s
        dx, dy = xs[sel] - s % W, ys[sel] - s // W
        flow.reshape(-1, 2)[sel, 1] = m[0] + m[1] * dx + m[2] * dy
        flow.reshape(-1, 2)[sel, 0] = m[3] + m[4] * dx + m[5] * dy
    return flow
