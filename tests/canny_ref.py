"""Independent numpy restatement of the Canny edge map (canny_ivice, edge.py:19-35 of the reference) that dflow_canny_edges
computes: whole-image array stencils with explicit border index maps, and scipy.ndimage.label for hysteresis.  Written from
the definition (DESIGN.md "Canny edge maps"), not from the HIP code.  All integer arithmetic: the u8 edge map is exact."""
import math

import numpy as np
from scipy import ndimage

W121 = (1, 2, 1)


def gray(bgr):
    """cv2.cvtColor(BGR2GRAY) on u8: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    a = np.asarray(bgr).astype(np.int64)
    return (1868 * a[..., 0] + 9617 * a[..., 1] + 4899 * a[..., 2] + 8192) >> 14


def reflect101(idx, n):
    """BORDER_REFLECT_101 of indices in [-1, n]: -1 -> 1, n -> n - 2; a length-1 axis maps every index to 0."""
    idx = np.asarray(idx)
    if n == 1:
        return np.zeros_like(idx)
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def replicate(idx, n):
    return np.clip(idx, 0, n - 1)


def _stencil(img, border, taps):
    """sum over (i, j, w) in taps of w * img[border(y + i), border(x + j)]."""
    H, W = img.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.int64)
    for i, j, w in taps:
        out += w * img[np.ix_(border(ys + i, H), border(xs + j, W))]
    return out


def blur(g):
    """cv2.GaussianBlur(g, (3,3), 0) on u8: [1,2,1]^T [1,2,1] at BORDER_REFLECT_101, then (S + 8) >> 4."""
    taps = [(i, j, W121[i + 1] * W121[j + 1]) for i in (-1, 0, 1) for j in (-1, 0, 1)]
    return (_stencil(np.asarray(g, np.int64), reflect101, taps) + 8) >> 4


def sobel(b):
    """3x3 Sobel at BORDER_REPLICATE: (dx, dy)."""
    b = np.asarray(b, np.int64)
    dx = _stencil(b, replicate, [(i, s, s * W121[i + 1]) for i in (-1, 0, 1) for s in (-1, 1)])
    dy = _stencil(b, replicate, [(s, j, s * W121[j + 1]) for j in (-1, 0, 1) for s in (-1, 1)])
    return dx, dy


def thresholds(low, high):
    if low > high:
        low, high = high, low
    return math.floor(low), math.floor(high)


def classes(b, low, high):
    """(candidate, strong) boolean maps after non-maximum suppression of the L1 magnitude."""
    dx, dy = sobel(b)
    H, W = dx.shape
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)                                   # magnitude is 0 outside the image

    def at(oy, ox):                                     # m[y + oy][x + ox]
        return mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]

    lo, hi = thresholds(low, high)
    ax, ay = np.abs(dx), np.abs(dy) << 15
    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    horiz = ay < t22
    vert = ~horiz & (ay > t67)
    diag = ~horiz & ~vert
    s_neg = (dx ^ dy) < 0                               # s = -1: m[y-1][x+1], m[y+1][x-1]
    keep_h = (m > at(0, -1)) & (m >= at(0, 1))
    keep_v = (m > at(-1, 0)) & (m >= at(1, 0))
    keep_d = np.where(s_neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    keep = (horiz & keep_h) | (vert & keep_v) | (diag & keep_d)
    cand = (m > lo) & keep
    return cand, cand & (m > hi)


def hysteresis(cand, strong):
    """255 where a candidate is 8-connected through candidates to a strong one, else 0."""
    lab, _ = ndimage.label(cand, structure=np.ones((3, 3), bool))
    keep = np.unique(lab[strong])
    return np.where(np.isin(lab, keep[keep > 0]), 255, 0).astype(np.uint8)


def edges_from_gray(g, low=100, high=200):
    return hysteresis(*classes(blur(g), low, high))


def canny(bgr, low=100, high=200):
    """(H,W,3) uint8 BGR -> (H,W) uint8 0/255."""
    return edges_from_gray(gray(bgr), low, high)


def ivice(edges):
    """np.array((255 - edges) / 255, dtype='float32'), edge.py:28."""
    return np.array((255 - np.asarray(edges)) / 255, dtype="float32")
