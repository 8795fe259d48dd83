"""dflow_track_advance, dflow_track_seed and dflow_track_flow (include/dflow.h, "Point trajectories") restated in numpy: float32
throughout, one operation per written operation, so that the library's bytes can be compared with these.  Flow fields are (h,w,2)
[dy,dx] or (h,w,3) [U,V,valid]; the last dimension says which.  Nothing is modified in place."""
import numpy as np

F = np.float32
FREE, LIVE, LEFT, NOFLOW, NOBACK, INCONSISTENT = range(6)
NO_OWNER = 0x7fffffff
SEED_BLOCK = 1024                                   # cells per block sum of d_scan


def scan_len(h, w, step):
    """The int32 elements of dflow_track_seed's d_scan."""
    ncells = -(-h // step) * -(-w // step)
    return ncells + -(-ncells // SEED_BLOCK) + 1


def planes(flow):
    """(U, V, good) of a field in either layout."""
    flow = np.asarray(flow, F)
    if flow.shape[2] == 3:
        U, V = flow[..., 0], flow[..., 1]
        with np.errstate(invalid="ignore"):
            valid = flow[..., 2] > F(0.5)
    else:
        V, U = flow[..., 0], flow[..., 1]
        valid = np.ones(U.shape, bool)
    return U, V, valid & np.isfinite(U) & np.isfinite(V)


def inside(x, y, h, w):
    with np.errstate(invalid="ignore"):
        return (x >= F(0)) & (x <= F(w - 1)) & (y >= F(0)) & (y <= F(h - 1))


def sample(flow, x, y):
    """The bilinear sample of `flow` at the inside float32 positions (x, y): (U, V, good); U and V mean nothing where not good."""
    U, V, good = planes(flow)
    y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    ay, ax = y - y0.astype(F), x - x0.astype(F)
    y1, x1 = np.where(ay > 0, y0 + 1, y0), np.where(ax > 0, x0 + 1, x0)
    ok = good[y0, x0] & good[y0, x1] & good[y1, x0] & good[y1, x1]
    out = []
    with np.errstate(all="ignore"):
        for P in (U, V):
            t = P[y0, x0] + ax * (P[y0, x1] - P[y0, x0])
            b = P[y1, x0] + ax * (P[y1, x1] - P[y1, x0])
            out.append((t + ay * (b - t)).astype(F))
    assert out[0].dtype == F and ay.dtype == F
    return out[0], out[1], ok


def advance(h, w, fwd, bwd, pos, state, rel=0.01, abs=0.5):
    """-> (pos_out, state_out, err, counts[6])."""
    pos, state = np.asarray(pos, F), np.asarray(state, np.int32)
    rel, abs = F(rel), F(abs)
    pos_out, state_out = pos.copy(), state.copy()
    err = np.full(len(state), -1, F)
    live = np.flatnonzero(state == LIVE)
    x, y = pos[live, 0], pos[live, 1]
    ins = inside(x, y, h, w)
    state_out[live[~ins]] = LEFT
    live, x, y = live[ins], x[ins], y[ins]
    U, V, ok = sample(fwd, x, y)
    state_out[live[~ok]] = NOFLOW
    live, x, y, U, V = live[ok], x[ok], y[ok], U[ok], V[ok]
    nx, ny = x + U, y + V
    ins = inside(nx, ny, h, w)
    state_out[live[~ins]] = LEFT
    live, nx, ny, U, V = live[ins], nx[ins], ny[ins], U[ins], V[ins]
    if bwd is not None:
        bu, bv, ok = sample(bwd, nx, ny)
        state_out[live[~ok]] = NOBACK
        live, nx, ny, U, V, bu, bv = live[ok], nx[ok], ny[ok], U[ok], V[ok], bu[ok], bv[ok]
        with np.errstate(all="ignore"):
            du, dv = U + bu, V + bv
            e2 = du * du + dv * dv
            m2 = (U * U + V * V) + (bu * bu + bv * bv)
            ok = e2 <= rel * m2 + abs
        assert e2.dtype == F and (rel * m2 + abs).dtype == F
        err[live] = e2
        state_out[live[~ok]] = INCONSISTENT
        live, nx, ny = live[ok], nx[ok], ny[ok]
    pos_out[live, 0], pos_out[live, 1] = nx, ny
    was_live = state == LIVE
    counts = [int(((state_out == k) & was_live).sum()) for k in (LIVE, LEFT, NOFLOW, NOBACK, INCONSISTENT)] + [int((~was_live).sum())]
    return pos_out, state_out, err, np.array(counts, np.int32)


def seed(h, w, step, frame, mask, pos, state, birth, n):
    """-> (pos, state, birth, n, counts[4]); cap is the length of the set, n whatever *d_n holds."""
    pos, state, birth = np.array(pos, F), np.array(state, np.int32), np.array(birth, np.int32)
    cap = len(state)
    n = min(max(int(n), 0), cap)
    gh, gw = -(-h // step), -(-w // step)
    covered = np.zeros((gh, gw), bool)
    i = np.flatnonzero(state[:n] == LIVE)
    i = i[inside(pos[i, 0], pos[i, 1], h, w)]
    covered[np.rint(pos[i, 1]).astype(np.int64) // step, np.rint(pos[i, 0]).astype(np.int64) // step] = True
    sy = np.minimum(np.arange(gh) * step + step // 2, h - 1)
    sx = np.minimum(np.arange(gw) * step + step // 2, w - 1)
    seedable = ~covered
    if mask is not None:
        seedable &= np.asarray(mask)[sy[:, None], sx[None, :]] != 0
    cy, cx = np.nonzero(seedable)                    # raster order
    total = len(cy)
    seeded = min(total, cap - n)
    slots = n + np.arange(seeded)
    pos[slots, 0], pos[slots, 1] = sx[cx[:seeded]].astype(F), sy[cy[:seeded]].astype(F)
    state[slots] = LIVE
    birth[slots] = frame
    return pos, state, birth, n + seeded, np.array([covered.sum(), total, seeded, total - seeded], np.int32)


def flow(h, w, pos_a, state_a, pos_b, state_b):
    """-> (owner (h,w) int32, out (h,w,3) float32, counts[3])."""
    pos_a, pos_b = np.asarray(pos_a, F), np.asarray(pos_b, F)
    part = (np.asarray(state_a) == LIVE) & (np.asarray(state_b) == LIVE) & inside(pos_a[:, 0], pos_a[:, 1], h, w)
    i = np.flatnonzero(part)
    pix = np.rint(pos_a[i, 1]).astype(np.int64) * w + np.rint(pos_a[i, 0]).astype(np.int64)
    owner = np.full(h * w, NO_OWNER, np.int32)
    np.minimum.at(owner, pix, i.astype(np.int32))
    out = np.zeros((h * w, 3), F)
    p = np.flatnonzero(owner != NO_OWNER)
    o = owner[p]
    out[p, 0], out[p, 1], out[p, 2] = pos_b[o, 0] - pos_a[o, 0], pos_b[o, 1] - pos_a[o, 1], 1
    counts = np.array([len(p), len(i) - len(p), len(part) - len(i)], np.int32)
    return owner.reshape(h, w), out.reshape(h, w, 3), counts


# ---- the inputs the CPU and the GPU tests share
def coverage_case(seed_=4):
    """The 37x53 class-coverage case: (h, w, fwd [U,V,valid], bwd, pos, state).  1000 tracks at random sub-pixel positions, 100 of
    them on integers, 10 on x = w-1, 10 on y = 0, every 17th already terminal, one FREE, and LIVE tracks at NaN, +-Inf, -1 and 1e9."""
    h, w = 37, 53
    rng = np.random.default_rng(seed_)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    fwd = np.zeros((h, w, 3), F)
    fwd[..., 0] = 3 * np.sin(xx / 9) + 2 * np.cos(yy / 7)
    fwd[..., 1] = 2 * np.cos(xx / 11) - 1.5 * np.sin(yy / 5)
    fwd[..., 2] = 1
    bwd = fwd.copy()
    bwd[..., :2] = -bwd[..., :2]
    bwd[:, 30:40, 0] += F(2)
    for f in (fwd, bwd):
        f[..., 2][rng.random((h, w)) < 0.03] = 0
    fwd[5, 7, 0], fwd[20, 40, 1] = np.nan, np.inf
    bwd[9, 11, 1], bwd[30, 3, 0] = np.nan, -np.inf
    n = 1000
    pos = np.stack([rng.random(n) * (w - 1), rng.random(n) * (h - 1)], 1).astype(F)
    pos[:100] = np.rint(pos[:100])
    pos[100:110, 0] = w - 1
    pos[110:120, 1] = 0
    state = np.full(n, LIVE, np.int32)
    state[::17] = rng.integers(LEFT, INCONSISTENT + 1, len(state[::17]))
    state[3] = FREE
    odd = np.array([[np.nan, 3], [4, np.nan], [np.inf, 5], [6, -np.inf], [-1, 7], [8, -1], [1e9, 9], [10, 1e9], [-0.0, 36.0], [52.0, -0.0],
                    [52.000004, 10], [10, 36.000004]], F)
    pos = np.concatenate([pos, odd])
    state = np.concatenate([state, np.full(len(odd), LIVE, np.int32)])
    return h, w, fwd, bwd, pos, state


def to_dydx(flow):
    """[U,V,valid] -> [dy,dx], the vectors that are not valid made NaN (so that the same ones are not good)."""
    out = np.stack([flow[..., 1], flow[..., 0]], -1).astype(F)
    out[~(flow[..., 2] > 0.5)] = np.nan
    return out


def rotation_field(h, w, angle):
    """The flow of the rotation by `angle` about the frame's centre, [U,V,valid] float32 rounded from float64."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    c, s = np.cos(angle), np.sin(angle)
    f = np.ones((h, w, 3), F)
    f[..., 0] = c * (xx - cx) - s * (yy - cy) + cx - xx
    f[..., 1] = s * (xx - cx) + c * (yy - cy) + cy - yy
    return f


def grid_seeds(h, w, step):
    """A seed every `step` pixels from step/2 on (the centres of the whole cells)."""
    ys, xs = np.mgrid[step // 2:h:step, step // 2:w:step]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(F)
