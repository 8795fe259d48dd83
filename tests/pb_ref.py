"""The soft edge strength of dflow_pb_edges (include/dflow.h, DESIGN.md "Pb edge strength") restated in numpy, independent of
the kernel: integer histograms by indexed adds over the whole frame, then the chi^2 sums in float64, or in float32 in the
stated order (one IEEE operation per written operation)."""
import numpy as np

NORMALS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1))     # (nx, ny) of orientation 0..7


def channels(bgr):
    """(H,W,3) uint8 BGR -> (3,H,W) int64 channels c0, c1, c2 in 0..255."""
    B, G, R = (bgr[..., i].astype(np.int64) for i in range(3))
    c0 = (1868 * B + 9617 * G + 4899 * R + 8192) >> 14
    c1 = (R - G + 255) >> 1
    c2 = (2 * B - R - G + 510) >> 2
    c = np.stack([c0, c1, c2])
    assert c.min() >= 0 and c.max() <= 255
    return c


def offsets(radius):
    """The disc: [(dx, dy)] with 0 < dx^2 + dy^2 <= radius^2."""
    r = range(-radius, radius + 1)
    return [(dx, dy) for dy in r for dx in r if 0 < dx * dx + dy * dy <= radius * radius]


def side_counts(radius):
    """[(offsets on side A, offsets on side B)] of orientation 0..7."""
    out = []
    for nx, ny in NORMALS:
        dots = [dx * nx + dy * ny for dx, dy in offsets(radius)]
        out.append((sum(d > 0 for d in dots), sum(d < 0 for d in dots)))
    return out


def histograms(bgr, radius):
    """(G, H): int64 (8,3,H,W,16), the counts of bin b of channel c on side A / side B of orientation o at every pixel."""
    bins = channels(bgr) >> 4
    _, H, W = bins.shape
    pad = np.pad(bins, ((0, 0), (radius, radius), (radius, radius)), mode="edge")        # replicate border
    G = np.zeros((8, 3, H, W, 16), np.int64)
    Hh = np.zeros_like(G)
    cc, yy, xx = np.meshgrid(np.arange(3), np.arange(H), np.arange(W), indexing="ij")
    for dx, dy in offsets(radius):
        b = pad[:, radius + dy:radius + dy + H, radius + dx:radius + dx + W]
        for o, (nx, ny) in enumerate(NORMALS):
            d = dx * nx + dy * ny
            if d != 0:
                (G if d > 0 else Hh)[o][cc, yy, xx, b] += 1     # every (c, y, x) once per offset: no repeated index
    return G, Hh


def strength_from(G, Hh, radius, dtype):
    """(e (H,W), m (H,W,8)) of the histograms, every operation in `dtype` (np.float64, or np.float32 in the stated order)."""
    num = ((G - Hh) ** 2).astype(dtype)
    den = (G + Hh).astype(dtype)
    s = np.zeros(G.shape[:-1], dtype)
    for b in range(16):                                       # ascending b
        live = den[..., b] > 0
        t = np.zeros_like(s)
        t[live] = num[..., b][live] / den[..., b][live]
        s = np.where(live, s + t, s)
    assert s.dtype == dtype
    N = np.array([a for a, _ in side_counts(radius)])
    chi = s / (2 * N).astype(dtype)[:, None, None, None]     # (8,3,H,W)
    m = (dtype(2) * chi[:, 0] + chi[:, 1] + chi[:, 2]) / dtype(4)
    assert m.dtype == dtype
    m = np.moveaxis(m, 0, -1)
    return m.max(axis=-1), np.ascontiguousarray(m)


def pb(bgr, radius=5, dtype=np.float64):
    G, Hh = histograms(np.asarray(bgr), radius)
    return strength_from(G, Hh, radius, dtype)


def pb_both(bgr, radius=5):
    """((e64, m64), (e32, m32)) from one set of histograms."""
    G, Hh = histograms(np.asarray(bgr), radius)
    return strength_from(G, Hh, radius, np.float64), strength_from(G, Hh, radius, np.float32)


def two_region_frame(H=40, W=56, split=28, seed=0):
    """Two colour regions, columns [0, split) and [split, W), with uniform +-20 noise per channel from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W, 3), np.int64)
    img[:, :split] = (60, 120, 200)
    img[:, split:] = (200, 90, 50)
    img += rng.integers(-20, 21, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def boundary_frame(H, W, seed=0):
    """B, G, R drawn from 0, 15, 16, 239, 240, 255, the bin boundaries and the ends of the range; every other pixel is grey
    (B = G = R), where c0 is that value itself; the others put c1 and c2 at 0, 255 and values next to bin boundaries."""
    rng = np.random.default_rng(seed)
    img = np.array([0, 15, 16, 239, 240, 255], np.uint8)[rng.integers(0, 6, (H, W, 3))]
    grey = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    img[grey] = img[grey][:, :1]
    return np.ascontiguousarray(img)
