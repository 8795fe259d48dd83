"""dflow_prior_proposals and dflow_flow_advance (include/dflow.h) in plain numpy loops: the definitions the device is compared
against bit for bit.  The L1 cost is written out in its summation order with np.float32 scalars (no np.sum), so nothing here
depends on how numpy happens to sum."""
import numpy as np

UVV, DYDX = 0, 1                  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX
SEED_LABELS = 1                   # DFLOW_PRIOR_SEED_LABELS
NEGATE = 1                        # DFLOW_ADVANCE_NEGATE
OFFSETS = ((0, 0), (-1, 0), (0, -1), (0, 1), (1, 0))      # times the stride: candidates k = 0..4


def layout_of(field):
    return UVV if field.shape[2] == 3 else DYDX


def usable_vector(field, layout, y, x):
    """The vector of pixel (y,x) as a label: (dy, dx) ints, or None (invalid, not finite, or a rounded component outside
    [-32767, 32767])."""
    if layout == UVV:
        if not (np.float32(field[y, x, 2]) > np.float32(0.5)):
            return None
        fy, fx = np.float32(field[y, x, 1]), np.float32(field[y, x, 0])
    else:
        fy, fx = np.float32(field[y, x, 0]), np.float32(field[y, x, 1])
    if not (np.isfinite(fy) and np.isfinite(fx)):
        return None
    ry, rx = np.rint(fy), np.rint(fx)                     # ties to even, as rintf
    if abs(float(ry)) > 32767.0 or abs(float(rx)) > 32767.0:
        return None
    return int(ry), int(rx)


def pack(dy, dx):
    return (int(dy) & 0xFFFF) | ((int(dx) & 0xFFFF) << 16)


def l1_cost(a, b):
    """sum |a - b| over 68 float32 values in numpy's pairwise order for that length: eight running sums, the tree, then the
    four-element tail; every operation rounds to float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = [np.float32(abs(np.float32(a[j] - b[j]))) for j in range(8)]
        for i in range(8, 64, 8):
            for j in range(8):
                r[j] = np.float32(r[j] + np.float32(abs(np.float32(a[i + j] - b[i + j]))))
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                         + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for i in range(64, 68):
            res = np.float32(res + np.float32(abs(np.float32(a[i] - b[i]))))
    return res


def prior_proposals(packed, lcosts, nprop, bestlabels, descr1, descr2, prior, stride, flags, maxnprop, tphi):
    """packed (H,W,LP) uint32, lcosts (H,W,LP) float32, nprop, bestlabels (H,W) int: modified IN PLACE.  descr1, descr2
    (H,W,68) float32; prior (H,W,2) [dy,dx] or (H,W,3) [U,V,valid].  Returns the counts [appended, found, full, skipped]."""
    H, W = nprop.shape
    layout = layout_of(prior)
    tphi = np.float32(tphi)
    counts = [0, 0, 0, 0]
    for y in range(H):
        for x in range(W):
            for k in range(5 if stride else 1):
                sy, sx = y + OFFSETS[k][0] * stride, x + OFFSETS[k][1] * stride
                if not (0 <= sy < H and 0 <= sx < W):
                    counts[3] += 1
                    continue
                v = usable_vector(prior, layout, sy, sx)
                if v is None or not (0 <= y + v[0] < H and 0 <= x + v[1] < W):
                    counts[3] += 1
                    continue
                label, n = pack(*v), int(nprop[y, x])
                hits = np.flatnonzero(packed[y, x, :n] == np.uint32(label))       # both halves equal
                slot = int(hits[0]) if hits.size else -1
                if slot >= 0:
                    counts[1] += 1
                elif n < maxnprop:
                    slot = n
                    packed[y, x, n] = label
                    l1 = l1_cost(descr1[y, x], descr2[y + v[0], x + v[1]])
                    lcosts[y, x, n] = l1 if l1 < tphi else tphi
                    nprop[y, x] = n + 1
                    counts[0] += 1
                else:
                    counts[2] += 1
                if k == 0 and slot >= 0 and (flags & SEED_LABELS):
                    bestlabels[y, x] = slot
    return counts


def flow_advance(flow, flags=0):
    """flow (H,W,2) [dy,dx] or (H,W,3) [U,V,valid] -> ((H,W,3) float32 [U,V,valid], [claimed, lost, not taking part])."""
    H, W = flow.shape[:2]
    layout = layout_of(flow)
    winner = {}
    part = 0
    for y in range(H):                                    # raster order: the first claimant has the smallest index
        for x in range(W):
            v = usable_vector(flow, layout, y, x)
            if v is None or not (0 <= y + v[0] < H and 0 <= x + v[1] < W):
                continue
            part += 1
            winner.setdefault((y + v[0], x + v[1]), v)
    out = np.zeros((H, W, 3), np.float32)
    for (ty, tx), (dy, dx) in winner.items():
        if flags & NEGATE:
            dy, dx = -dy, -dx                             # the integer is negated: 0 stays +0.0
        out[ty, tx] = (np.float32(dx), np.float32(dy), np.float32(1))
    return out, [len(winner), part - len(winner), H * W - part]

