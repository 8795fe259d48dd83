"""dflow_segment_filter's definition (include/dflow.h) as a plain flood fill over the members with the float32 join test: the
reference of tests/test_segments_ref.py and tests/test_gpu_segments.py.  Nothing here is shared with the kernels: a stack-based
fill from every unlabelled member in raster order, so that the seed is the segment's smallest raster index."""
import os

import numpy as np

UVV, DYDX = 0, 1
KEEP_SINGLETONS = 1


def members(flow):
    """(U, V, member) of a (H,W,3) [U,V,valid] or (H,W,2) [dy,dx] float32 field: valid under its layout, both components finite."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] in (2, 3), (flow.shape, flow.dtype)
    if flow.shape[2] == 3:
        U, V, ok = flow[..., 0], flow[..., 1], flow[..., 2] > np.float32(0.5)         # a NaN compares false
    else:
        U, V, ok = flow[..., 1], flow[..., 0], np.ones(flow.shape[:2], bool)
    return U, V, ok & np.isfinite(U) & np.isfinite(V)


def joined(ua, va, ub, vb, thresh):
    """fabsf(ua - ub) + fabsf(va - vb) <= thresh on float32 arrays (or scalars), one rounding per operation; an overflow gives
    inf, which is not <= a finite thresh.  Called on members only, so no NaN arises."""
    ua, va, ub, vb = (np.asarray(a, np.float32) for a in (ua, va, ub, vb))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(ua - ub) + np.abs(va - vb) <= np.float32(thresh)


def segment_filter(flow, thresh, min_size, flags=0):
    """-> (out (H,W,3) float32, segment (H,W) int32, size (H,W) int32, counts [segments, segments removed, members, pixels
    removed])."""
    U, V, mem = members(flow)
    h, w = mem.shape
    thresh = np.float32(thresh)
    segment = np.full((h, w), -1, np.int32)
    size = np.zeros((h, w), np.int32)
    out = np.zeros((h, w, 3), np.float32)
    counts = [0, 0, int(mem.sum()), 0]
    # right[y, x]: (y, x) and (y, x+1) are joined; down[y, x]: (y, x) and (y+1, x)
    right, down = np.zeros((h, w), bool), np.zeros((h, w), bool)
    right[:, :-1] = mem[:, :-1] & mem[:, 1:] & joined(U[:, :-1], V[:, :-1], U[:, 1:], V[:, 1:], thresh)
    down[:-1] = mem[:-1] & mem[1:] & joined(U[:-1], V[:-1], U[1:], V[1:], thresh)
    for y0 in range(h):
        for x0 in range(w):
            if not mem[y0, x0] or segment[y0, x0] >= 0:
                continue
            sid = y0 * w + x0
            segment[y0, x0] = sid
            stack, pixels = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                for yy, xx, link in ((y - 1, x, y > 0 and down[y - 1, x]), (y + 1, x, down[y, x]),
                                     (y, x - 1, x > 0 and right[y, x - 1]), (y, x + 1, right[y, x])):
                    if link and segment[yy, xx] < 0:
                        segment[yy, xx] = sid
                        stack.append((yy, xx))
            n = len(pixels)
            removed = bool(n < min_size and not (flags & KEEP_SINGLETONS and n == 1))
            counts[0] += 1
            counts[1] += int(removed)
            counts[3] += n if removed else 0
            ys, xs = np.array(pixels).T
            size[ys, xs] = n
            if not removed:
                out[ys, xs, 0], out[ys, xs, 1], out[ys, xs, 2] = U[ys, xs], V[ys, xs], 1.0
    return out, segment, size, counts


# ---- fields that both test files use
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def uvv(U, V=None, valid=None):
    """A [U,V,valid] field from planes or scalars; V defaults to 0 and valid to 1."""
    U = np.asarray(U, np.float32)
    f = np.zeros(U.shape + (3,), np.float32)
    f[..., 0] = U
    f[..., 1] = 0 if V is None else V
    f[..., 2] = 1 if valid is None else valid
    return f


def golden_fields():
    """(name, field, T, MIN): seg0_in..seg2_in with their own parameters, sparse_t1 / sparse_t3 of the related goldens at (1, 20)."""
    z = np.load(os.path.join(GOLDEN, "ref_extras.npz"))
    out = [("seg%d" % i, z["seg%d_in" % i], float(z["seg%d_par" % i][0]), int(z["seg%d_par" % i][1])) for i in range(3)]
    for name in ("a40x48_c5x6", "b36x40_c9x8", "c45x35_c9x7"):
        g = np.load(os.path.join(GOLDEN, "ref_%s.npz" % name))
        out += [("%s %s" % (name, k), g[k], 1.0, 20) for k in ("sparse_t1", "sparse_t3")]
    return out
