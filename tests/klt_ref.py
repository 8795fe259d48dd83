"""dflow_klt_pyramid, dflow_corners and dflow_klt_track (include/dflow_klt.h) in numpy, written from the header's text and
vectorised over pixels and over tracks: the definitions the device is compared against bit for bit.  Sums are int64, float32
chains are numpy float32 arrays with the written operation order (numpy fuses nothing), the 2x2 solve is float64."""
import numpy as np

F = np.float32
FREE, LIVE, LEFT, NOFLOW, NOBACK, INCONSISTENT, FLAT, RESIDUAL = range(8)
K = (1, 4, 6, 4, 1)


# ---------------------------------------------------------------- the pyramid
def level_sizes(h, w, levels):
    out = []
    for _ in range(levels):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def level_offsets(h, w, levels):
    """The byte offset of every level in the one buffer, and the total."""
    offs, at = [], 0
    for hl, wl in level_sizes(h, w, levels):
        offs.append(at)
        at += hl * wl
    return offs, at


def grey(bgr):
    a = np.asarray(bgr).astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == 3
    return ((29 * a[..., 0] + 150 * a[..., 1] + 77 * a[..., 2] + 128) >> 8).astype(np.uint8)


def down(L):
    """(h,w) uint8 -> ((h+1)//2, (w+1)//2) uint8: the 5x5 binomial, border replicated, one rounding."""
    h, w = L.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    a = L.astype(np.int64)
    ys, xs = 2 * np.arange(hc), 2 * np.arange(wc)
    acc = np.zeros((hc, wc), np.int64)
    for i in range(-2, 3):
        rows = a[np.clip(ys + i, 0, h - 1)]
        for j in range(-2, 3):
            acc += K[i + 2] * K[j + 2] * rows[:, np.clip(xs + j, 0, w - 1)]
    return ((acc + 128) >> 8).astype(np.uint8)


def pyramid(bgr, levels):
    """The list of levels, level 0 the grey image."""
    out = [grey(bgr)]
    for _ in range(levels - 1):
        out.append(down(out[-1]))
    return out


def pack(pyr):
    return np.concatenate([L.reshape(-1) for L in pyr])


def unpack(buf, h, w, levels):
    offs, total = level_offsets(h, w, levels)
    assert buf.shape == (total,) and buf.dtype == np.uint8
    return [buf[o:o + hl * wl].reshape(hl, wl) for o, (hl, wl) in zip(offs, level_sizes(h, w, levels))]


# ---------------------------------------------------------------- corners
def inside(x, y, w, h):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= F(w - 1)) & (y >= 0) & (y <= F(h - 1))


def response(Y, rc):
    h, w = Y.shape
    a = Y.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    gx = a[:, np.minimum(xs + 1, w - 1)] - a[:, np.maximum(xs - 1, 0)]
    gy = a[np.minimum(ys + 1, h - 1)] - a[np.maximum(ys - 1, 0)]
    A, B, C = (np.zeros((h, w), np.int64) for _ in range(3))
    for i in range(-rc, rc + 1):
        yy = np.clip(ys + i, 0, h - 1)
        for j in range(-rc, rc + 1):
            xx = np.clip(xs + j, 0, w - 1)
            g1, g2 = gx[yy][:, xx], gy[yy][:, xx]
            A += g1 * g1
            B += g1 * g2
            C += g2 * g2
    rad = (A - C) * (A - C) + 4 * (B * B)
    assert rad.max() < 2 ** 53
    lam = ((A + C).astype(np.float64) - np.sqrt(rad.astype(np.float64))) * 0.5
    return np.where(lam > 0.0, lam, 0.0).astype(F)


def occupation(h, w, pos, state, n):
    occ = np.zeros((h, w), np.uint8)
    n = min(max(int(n), 0), len(state))
    pos, state = pos[:n], state[:n]
    on = (state == LIVE) & inside(pos[:, 0], pos[:, 1], w, h)
    occ[np.rint(pos[on, 1]).astype(np.int64), np.rint(pos[on, 0]).astype(np.int64)] = 1
    return occ


def corners(Y, rc=2, min_dist=4, border=4, quality=0.01, min_response=0.0, tracks=None):
    """-> (R (h,w) float32, mask (h,w) uint8, counts int32[4], Rmax float32).  tracks: None or (pos, state, n)."""
    h, w = Y.shape
    R = response(Y, rc)
    rmax = R.max()
    thr = F(quality) * rmax
    assert thr.dtype == F
    ys, xs = np.mgrid[0:h, 0:w]
    cand = (xs >= border) & (xs <= w - 1 - border) & (ys >= border) & (ys <= h - 1 - border) & (R >= thr) & (R >= F(min_response)) & (R > 0)
    occ = occupation(h, w, *tracks) if tracks is not None else np.zeros((h, w), np.uint8)
    m = min_dist
    Rp = np.pad(R, m, constant_values=-np.inf)
    Op = np.pad(occ, m)
    beaten, taken = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for dy in range(-m, m + 1):
        for dx in range(-m, m + 1):
            Rn = Rp[m + dy:m + dy + h, m + dx:m + dx + w]
            beaten |= (Rn > R) | ((Rn == R) & ((dy < 0) or (dy == 0 and dx < 0)))
            taken |= Op[m + dy:m + dy + h, m + dx:m + dx + w] != 0
    top = cand & ~beaten
    corner = top & ~taken
    counts = np.array([cand.sum(), top.sum(), (top & taken).sum(), corner.sum()], np.int32)
    return R, np.where(corner, 255, 0).astype(np.uint8), counts, rmax


def corner_positions(mask):
    """(n,2) float32 [x,y] of the corners in raster order: what dflow_track_seed with step 1 makes of the mask."""
    ys, xs = np.nonzero(mask)
    return np.stack([xs, ys], 1).astype(F)


# ---------------------------------------------------------------- the tracker
def sample(G, x, y):
    """SAMPLE: 32 * grey of level G at float32 (x, y), int64."""
    assert x.dtype == F and y.dtype == F
    hl, wl = G.shape
    g = G.astype(np.int64)
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    bx, by = F(1) - ax, F(1) - ay
    s = F(16384)
    w00 = np.rint((bx * by) * s).astype(np.int64)
    w01 = np.rint((ax * by) * s).astype(np.int64)
    w10 = np.rint((bx * ay) * s).astype(np.int64)
    w11 = 16384 - w00 - w01 - w10
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(xi, 0, wl - 1), np.clip(xi + 1, 0, wl - 1)
    ya, yb = np.clip(yi, 0, hl - 1), np.clip(yi + 1, 0, hl - 1)
    return (w00 * g[ya, xa] + w01 * g[ya, xb] + w10 * g[yb, xa] + w11 * g[yb, xb] + 256) >> 9


def one_pass(pyr_a, pyr_b, p, run, r, iters, eps, min_eig, max_err):
    """PASS for the tracks that have `run`: -> (res int32 (LIVE, LEFT, FLAT, RESIDUAL), q (N,2), err float32 (-1 where it was
    not formed), converged bool (at level 0))."""
    levels, N = len(pyr_a), len(p)
    run = run.copy()
    res = np.full(N, LIVE, np.int32)
    conv = np.zeros(N, bool)
    dx, dy = np.zeros(N, F), np.zeros(N, F)
    n = (2 * r + 1) ** 2
    ti, tj = np.mgrid[-r - 1:r + 2, -r - 1:r + 2]
    ti, tj = ti.astype(F)[None], tj.astype(F)[None]
    ii, jj = ti[:, 1:-1, 1:-1], tj[:, 1:-1, 1:-1]
    eps2 = np.float64(F(eps)) * np.float64(F(eps))
    px, py = p[:, 0].copy(), p[:, 1].copy()
    px[~run], py[~run] = 0, 0                           # a place to sample for the slots that take no part: nothing of it is kept
    T = Ix = Iy = None
    with np.errstate(all="ignore"):
        for l in range(levels - 1, -1, -1):
            Ga, Gb = pyr_a[l], pyr_b[l]
            hl, wl = Ga.shape
            s = F(1) / F(1 << l)
            plx, ply = px * s, py * s
            if l < levels - 1:
                dx, dy = F(2) * dx, F(2) * dy
            T = sample(Ga, plx[:, None, None] + tj, ply[:, None, None] + ti)
            Ix = T[:, 1:-1, 2:] - T[:, 1:-1, :-2]
            Iy = T[:, 2:, 1:-1] - T[:, :-2, 1:-1]
            A, B, C = ((a * b).sum((1, 2)).astype(np.float64) for a, b in ((Ix, Ix), (Ix, Iy), (Iy, Iy)))
            D = A * C - B * B
            lam = ((A + C) - np.sqrt((A - C) * (A - C) + 4.0 * (B * B))) * 0.5 / (4096.0 * n)
            flat = (lam < np.float64(F(min_eig))) | ~(D > 0)
            if l == 0:
                res[run & flat] = FLAT
                run &= ~flat
            on = run & ~flat
            Tin = T[:, 1:-1, 1:-1]
            for _ in range(iters):
                if not on.any():
                    break
                qx, qy = plx + dx, ply + dy
                if l > 0:
                    qx = np.minimum(np.maximum(qx, F(0)), F(wl - 1))
                    qy = np.minimum(np.maximum(qy, F(0)), F(hl - 1))
                    dx, dy = np.where(on, qx - plx, dx), np.where(on, qy - ply, dy)
                else:
                    out = on & ~inside(qx, qy, wl, hl)
                    res[out] = LEFT
                    run &= ~out
                    on &= ~out
                qx, qy = np.where(on, qx, F(0)), np.where(on, qy, F(0))
                e = sample(Gb, qx[:, None, None] + jj, qy[:, None, None] + ii) - Tin
                bx, by = (e * Ix).sum((1, 2)).astype(np.float64), (e * Iy).sum((1, 2)).astype(np.float64)
                ex, ey = -2.0 * ((C * bx - B * by) / D), -2.0 * ((A * by - B * bx) / D)
                dx, dy = np.where(on, dx + ex.astype(F), dx), np.where(on, dy + ey.astype(F), dy)
                stop = on & (ex * ex + ey * ey < eps2)
                if l == 0:
                    conv |= stop
                on &= ~stop
        assert dx.dtype == F and dy.dtype == F
        h, w = pyr_a[0].shape
        qx, qy = px + dx, py + dy
        out = run & ~inside(qx, qy, w, h)
        res[out] = LEFT
        run &= ~out
        sx, sy = np.where(run, qx, F(0)), np.where(run, qy, F(0))
        e = sample(pyr_b[0], sx[:, None, None] + jj, sy[:, None, None] + ii) - T[:, 1:-1, 1:-1]
        err = (np.abs(e).sum((1, 2)).astype(np.float64) / (32.0 * n)).astype(F)
        err = np.where(run, err, F(-1))
        if F(max_err) > 0:
            bad = run & (err > F(max_err))
            res[bad] = RESIDUAL
            run &= ~bad
    return res, np.stack([qx, qy], 1), err, conv


def track(pyr1, pyr2, pos, state, r=7, iters=20, eps=0.01, min_eig=1.0, max_err=0.0, fb=0.5):
    """-> (pos_out, state_out, err, back, counts int32[8])."""
    pos, state = np.ascontiguousarray(pos, F), np.ascontiguousarray(state, np.int32)
    h, w = pyr1[0].shape
    live0 = state == LIVE
    start = live0 & inside(pos[:, 0], pos[:, 1], w, h)
    st = state.copy()
    st[live0 & ~start] = LEFT
    res, q, err, conv = one_pass(pyr1, pyr2, pos, start, r, iters, eps, min_eig, max_err)
    st[start] = res[start]
    conv &= start
    back = np.full(pos.shape, np.nan, F)
    if F(fb) > 0:
        go = start & (res == LIVE)
        res2, p2, _, _ = one_pass(pyr2, pyr1, q, go, r, iters, eps, min_eig, max_err)
        ok = go & (res2 == LIVE)
        back[ok] = p2[ok]
        with np.errstate(invalid="ignore"):
            bx, by = p2[:, 0] - pos[:, 0], p2[:, 1] - pos[:, 1]
            far = bx * bx + by * by > F(fb) * F(fb)
        st[go & (~ok | far)] = INCONSISTENT
    pos_out = np.where((st == LIVE)[:, None] & live0[:, None], q, pos).astype(F)
    pos_out.view(np.uint32)[~live0] = pos.view(np.uint32)[~live0]                   # position bits included
    counts = np.array([(live0 & (st == LIVE)).sum(), (live0 & (st == LEFT)).sum(), (live0 & (st == FLAT)).sum(),
                       (live0 & (st == RESIDUAL)).sum(), (live0 & (st == INCONSISTENT)).sum(), (~live0).sum(), conv.sum(), 0], np.int32)
    return pos_out, st, err, back, counts


def sparse_flow(h, w, pos_a, state_a, pos_b, state_b):
    """The [U,V,valid] field of the tracks that are LIVE in both snapshots (dflow_track_flow: the smallest index wins a pixel)."""
    out = np.zeros((h, w, 3), F)
    part = (state_a == LIVE) & (state_b == LIVE) & inside(pos_a[:, 0], pos_a[:, 1], w, h)
    for i in np.flatnonzero(part)[::-1]:
        y, x = int(np.rint(pos_a[i, 1])), int(np.rint(pos_a[i, 0]))
        out[y, x] = (pos_b[i, 0] - pos_a[i, 0], pos_b[i, 1] - pos_a[i, 1], 1)
    return out
