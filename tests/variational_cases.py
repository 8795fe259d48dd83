"""The inputs of the variational-refinement tests, shared by the CPU tests (which establish that the float64 reference
handles them and measure the float32 yardstick) and the GPU tests (which run the same inputs through dflow_var_refine)."""
import itertools
import os

import numpy as np

import canny_ref as CR
import epic_ref
from conftest import GOLDEN_NAMES, ROOT, pkg

SMALL_SIZES = ((1, 1), (1, 70), (70, 1), (33, 65), (129, 257))
# delta 0 and 0.5, sigma 0, 1 and 1.7, niter_inner 1 and 2: the whole product on the small inputs
PARAM_SETS = tuple(dict(delta=d, sigma=s, niter_inner=n) for d, s, n in itertools.product((0.0, 0.5), (0.0, 1.0, 1.7), (1, 2)))
# on the one Sintel-sized pair, the defaults and the far corner of that product
BIG_PARAM_SETS = (dict(delta=0.0, sigma=1.0, niter_inner=1), dict(delta=0.5, sigma=1.7, niter_inner=2))
# the ends of the Gaussian: sigma = 5 is the largest the C-ABI admits (radius 15, the size the smoothing kernel's LDS arrays are
# built for), sigma = 0.3 has radius 1; on frames smaller and larger than that kernel's 32 x 32 tile and its halo
EDGE_SIGMA_SETS = (dict(delta=0.0, sigma=5.0, niter_inner=1), dict(delta=0.5, sigma=0.3, niter_inner=1))
EDGE_SIGMA_SIZES = ((1, 70), (33, 65), (129, 257))
SOLVE_SIZE, SOLVE_NITER = (12, 16), 200     # the direct-solve case: SOR reaches np.linalg.solve to 1e-8 there (measured 5e-10)


def smooth_perturbation(H, W, amp=0.5):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([amp * np.sin(2 * np.pi * xx / 40.0) * np.cos(2 * np.pi * yy / 50.0),
                     amp * np.cos(2 * np.pi * xx / 35.0 + 1.0) * np.sin(2 * np.pi * yy / 45.0)], axis=-1)


def synth_case(H, W, seed, amp=0.5):
    """A synthetic pair with known motion (a few pixels) and a start: ground truth plus a smooth perturbation of amp px."""
    synth = pkg("synth")
    img1, img2, gt = synth.make_pair(H, W, seed=seed, amp_x=min(6.0, W / 8.0), amp_y=min(4.0, H / 8.0))
    return img1, img2, (gt + smooth_perturbation(H, W, amp)).astype(np.float32), gt


def golden_case(name):
    """A golden fixture's pair and, as the start, epic_ref.interpolate of its sparse_t3 over its Canny map."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_%s.npz" % name))
    img1, img2 = np.ascontiguousarray(z["img1"]), np.ascontiguousarray(z["img2"])
    flow = epic_ref.interpolate(z["sparse_t3"], CR.ivice(CR.canny(img1)), 100, 0.8, "LA")["flow"]
    return img1, img2, np.ascontiguousarray(flow, dtype=np.float32), z["gt"]


def solve_case():
    synth = pkg("synth")
    H, W = SOLVE_SIZE
    img1, img2, gt = synth.make_pair(H, W, seed=5, amp_x=2, amp_y=1)
    start = gt + 0.3 * np.random.default_rng(0).standard_normal(gt.shape)
    return img1, img2, start.astype(np.float32)


def parity_cases():
    """(id, img1, img2, flow, params) for every parity input."""
    for name in GOLDEN_NAMES:
        img1, img2, flow, _ = golden_case(name)
        for P in PARAM_SETS:
            yield "golden-%s" % name, img1, img2, flow, P
    for H, W in SMALL_SIZES:
        img1, img2, flow, _ = synth_case(H, W, seed=100 * H + W)
        for P in PARAM_SETS + (EDGE_SIGMA_SETS if (H, W) in EDGE_SIGMA_SIZES else ()):
            yield "%dx%d" % (H, W), img1, img2, flow, P
    img1, img2, flow, _ = synth_case(436, 1024, seed=9)
    for P in BIG_PARAM_SETS:
        yield "436x1024", img1, img2, flow, P
