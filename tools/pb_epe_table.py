"""The DESIGN.md table "does the edge map help the interpolation?": mean dense EPE of the CPU restatement of the interpolation
(tests/epic_ref.py, LA, nn = 100, k = 0.8) against the known flow, with four edge maps: Canny's ivice as the reference writes
it, 1 - ivice, all zeros, and the Pb strength of tests/pb_ref.py (R = 5).  CPU only: python tools/pb_epe_table.py
Frames: the golden fixtures (seeds sparse_t3), and the two-motion frame of tests/epic_prefilter_cases.py with its seeds
subsampled 1-in-16 and an image of two colour regions (pb_ref.two_region_frame, split at the band) for the detectors."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, "tests"))
import canny_ref, epic_prefilter_cases as PC, epic_ref, pb_ref


def epe(sparse, edges, gt):
    flow = epic_ref.interpolate(sparse, edges.astype(np.float32))["flow"]
    return float(np.hypot(flow[..., 0] - gt[..., 0], flow[..., 1] - gt[..., 1]).mean())


def row(name, sparse, img, gt):
    ivice = canny_ref.ivice(canny_ref.canny(img))
    maps = (ivice, 1.0 - ivice, np.zeros_like(ivice), pb_ref.pb(img, 5, np.float32)[0])
    print("| %s | %.1f %% | %s |" % (name, 100.0 * epic_ref.seed_mask(sparse).mean(), " | ".join("%.3f" % epe(sparse, m, gt) for m in maps)))


print("| frame | seeds | `ivice` as written | `1 - ivice` | all zeros | `pb`, R = 5 |\n|---|---|---|---|---|---|")
for name in ("a40x48_c5x6", "b36x40_c9x8", "c45x35_c9x7"):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_%s.npz" % name))
    row(name.split("_")[0], z["sparse_t3"], z["img1"], z["gt"].astype(np.float64))
sp, _, band = PC.two_motions()
H, W = sp.shape[:2]
sub = np.zeros_like(sp)
sub[::4, ::4] = sp[::4, ::4]
left = np.mgrid[0:H, 0:W][1] < band
gt = np.where(left[..., None], (-1.0, 3.0), (22.0, -20.0))           # [dy,dx] of the (u,v) = (3,-1) and (-20,22) motions
row("two motions, 1-in-16", sub, pb_ref.two_region_frame(H, W, band, seed=0), gt)
