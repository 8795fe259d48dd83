"""Inputs shared by test_epic_prefilter_ref.py (CPU: what the reference does with them) and test_gpu_epic_prefilter.py (the
GPU against the reference): a frame with planted outliers, the two-motion frame, a half-flat image, and the list of images
over which the float32 yardstick of the saliency is measured."""
import os

import numpy as np

from conftest import GOLDEN_NAMES, ROOT, pkg


def random_field(H, W, frac, seed, edge_style="random"):
    """A random sparse field and edge map, as test_gpu_epic.py draws them."""
    rng = np.random.default_rng(seed)
    sp = np.zeros((H, W, 3), np.float32)
    m = rng.random((H, W)) < frac
    sp[..., 0] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 1] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 2] = m
    e = rng.random((H, W)).astype(np.float32) if edge_style == "random" else (rng.random((H, W)) < 0.1).astype(np.float32)
    return sp, e


def planted(H=48, W=64, density=0.5, frac=0.06, seed=7):
    """(sparse, edges, planted mask, field (H,W,2) [dy,dx]): half the pixels carry a smooth affine flow; 6 % of those are
    displaced by 12 to 20 px in a random direction.  With 25 neighbours of which one or two are displaced, an estimate moves
    by about 1 px: far from pref_th = 5 on either side."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = 2.0 + 0.05 * xs - 0.03 * ys, -1.0 + 0.02 * xs + 0.04 * ys
    m = rng.random((H, W)) < density
    bad = m & (rng.random((H, W)) < frac)
    ang, mag = rng.uniform(0, 2 * np.pi, (H, W)), rng.uniform(12, 20, (H, W))
    sp = np.zeros((H, W, 3), np.float32)
    sp[..., 0] = np.where(m, u + bad * mag * np.cos(ang), 0)
    sp[..., 1] = np.where(m, v + bad * mag * np.sin(ang), 0)
    sp[..., 2] = m
    return sp, np.zeros((H, W), np.float32), bad, np.stack([v, u], axis=-1)


def two_motions(H=40, W=64, band=32):
    """(sparse, edges, band): constant motion (3, -1) left of a 1-px column of e = 1, (-20, 22) right of it (a jump of 32.5
    px); every pixel off the band is a seed."""
    xs = np.mgrid[0:H, 0:W][1]
    sp = np.zeros((H, W, 3), np.float32)
    sp[xs < band] = (3.0, -1.0, 1.0)
    sp[xs > band] = (-20.0, 22.0, 1.0)
    e = np.zeros((H, W), np.float32)
    e[:, band] = 1.0
    return sp, e, band


def half_flat_image(H=40, W=64, seed=3):
    """(H,W,3) uint8: the left half one colour, the right half white noise."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img[:, :W // 2] = (90, 120, 150)
    return img


def golden_case(name):
    """(sparse_t3, ivice of img1, img1) of a golden fixture."""
    import canny_ref as CR
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_%s.npz" % name))
    return z["sparse_t3"], CR.ivice(CR.canny(z["img1"])), z["img1"]


def synth_image(H, W, seed):
    return pkg("synth").make_pair(H, W, seed=seed)[0]


# (H, W, seed) of the synthetic frames the GPU tests run stage A on
SYNTH_FRAMES = ((33, 65, 1), (60, 90, 13), (436, 1024, 33))


def saliency_images():
    """Every image the GPU tests compare saliency on: (name, image)."""
    for name in GOLDEN_NAMES:
        yield name, golden_case(name)[2]
    for H, W, seed in SYNTH_FRAMES:
        yield "synth%dx%d" % (H, W), synth_image(H, W, seed)
    yield "half_flat", half_flat_image()
    for size in ((1, 1), (1, 70), (70, 1)):
        yield "noise%dx%d" % size, np.random.default_rng(size[0] + size[1]).integers(0, 256, size + (3,)).astype(np.uint8)
