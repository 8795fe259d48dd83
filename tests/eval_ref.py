"""The flow evaluation of include/dflow.h (dflow_flow_eval) restated in numpy from the definition, not from the HIP code:
float32 per pixel, one rounding per operation (numpy does not fuse), the statistics as Python ints and math.fsum."""
import math
import os
import re

import numpy as np

from conftest import PKG, ROOT

F = np.float32
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]      # how d_err holds a NaN

# matplotlib's 'jet', _jet_data of matplotlib/_cm.py
JET = {
    "r": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "g": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "b": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}


def jet_lut():
    """(256,3) uint8 (r,g,b): the segment data interpolated linearly at linspace(0,1,256) in float64, uint8(value * 255)."""
    x = np.linspace(0.0, 1.0, 256)
    return (np.stack([np.interp(x, [p[0] for p in JET[c]], [p[1] for p in JET[c]]) for c in "rgb"], axis=-1) * 255).astype(np.uint8)


def committed_lut():
    """(256,3) uint8 (r,g,b) of csrc/jet_lut.h, the table the kernel is compiled with."""
    text = open(os.path.join(ROOT, PKG, "csrc", "jet_lut.h")).read()
    v = np.array([int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{6})u", text)], np.uint32)
    assert v.size == 256
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)


def evaluate(test, gt, abs_thresh=3.0):
    """test (H,W,3) [U,V,valid] or (H,W,2) [dy,dx], gt (H,W,3) [U,V,valid], float32 -> dict: the fields of struct
    dflow_eval_stats (counts as Python ints, sum_err = math.fsum of the float32 errors, max_err a float), err (H,W)
    float32 and bgr (H,W,3) uint8."""
    test, gt = np.asarray(test, F), np.asarray(gt, F)
    H, W = gt.shape[:2]
    if test.shape[2] == 3:
        tU, tV, tvalid = test[..., 0], test[..., 1], test[..., 2]
    else:
        tU, tV, tvalid = test[..., 1], test[..., 0], np.ones((H, W), F)
    gU, gV, gvalid = gt[..., 0], gt[..., 1], gt[..., 2]
    with np.errstate(all="ignore"):
        gmask, tmask = gvalid > F(0.5), tvalid > F(0.5)
        compared = gmask & tmask
        dfu, dfv = tU - gU, tV - gV
        e = np.sqrt(dfu * dfu + dfv * dfv)
        assert e.dtype == np.float32
        counted = compared & np.isfinite(e)
        gmag = F(0.05) * np.sqrt(gU * gU + gV * gV)
        out_abs = counted & (e > F(abs_thresh))
        out_kitti = counted & (e > F(3.0)) & (e > gmag)
        t = np.minimum(e, F(3.0)) / F(3.0)
        idx = np.minimum(255, (np.where(counted, t, F(0)) * F(256.0)).astype(np.int32))
    err = np.where(compared, np.where(np.isnan(e), QNAN, e), F(-1.0)).astype(F)
    bgr = np.where(counted[..., None], jet_lut()[idx][..., ::-1], 0).astype(np.uint8)
    ec = e[counted]
    return dict(n=int(counted.sum()), n_out_abs=int(out_abs.sum()), n_out_kitti=int(out_kitti.sum()),
                n_nonfinite=int((compared & ~counted).sum()), n_gt_valid=int(gmask.sum()), n_test_valid=int(tmask.sum()),
                sum_err=math.fsum(float(v) for v in ec), max_err=float(ec.max()) if ec.size else 0.0, err=err, bgr=bgr)
