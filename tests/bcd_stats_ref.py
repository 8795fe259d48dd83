"""The definition of dflow_bcd_stats (include/dflow.h) restated in numpy: the reference the GPU tests compare against.

proposals: (H,W,L,2) integers [dy,dx]; lcosts: (H,W,L) float32 (anything else is refused: the device compares and sums the
float32 values); nprop, labels, prev: (H,W) integers.  Integers are exact; data_sum is math.fsum over the float32 costs of
the chosen labels, the correctly rounded sum, so that no summation order is built into the reference."""
import math

import numpy as np

INT_FIELDS = ("smooth_sum", "n_pairs_trunc", "n_data_trunc", "n_changed", "n_bad_label")


def bcd_stats_ref(proposals, lcosts, nprop, labels, tpsi, tphi, prev=None):
    """dict of the six fields of struct dflow_bcd_stats, plus sum_abs = fsum |cost| and n_data = the number of costs summed
    (what the error bound of a double summation in another order is made of)."""
    if lcosts.dtype != np.float32:
        raise TypeError("lcosts must be float32")
    labels = np.asarray(labels).astype(np.int64)
    nprop = np.asarray(nprop).astype(np.int64)
    H, W = labels.shape
    bad = (labels < 0) | (labels >= nprop)
    ok = ~bad
    safe = np.where(ok, labels, 0)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.asarray(proposals)[yy, xx, safe].astype(np.int64)              # (H,W,2)
    c = lcosts[yy, xx, safe]                                               # (H,W) float32
    tphi32 = np.float32(tphi)
    smooth = trunc = 0
    for (a, b, va, vb) in ((f[:, :-1], f[:, 1:], ok[:, :-1], ok[:, 1:]), (f[:-1], f[1:], ok[:-1], ok[1:])):
        d = np.abs(a - b).sum(-1)[va & vb]
        smooth += int(np.minimum(d, tpsi).sum())
        trunc += int((d >= tpsi).sum())
    costs = [float(v) for v in c[ok]]
    return dict(smooth_sum=smooth, n_pairs_trunc=trunc, n_data_trunc=int((c[ok] >= tphi32).sum()),
                n_changed=0 if prev is None else int(((labels != np.asarray(prev).astype(np.int64)) | bad).sum()),
                n_bad_label=int(bad.sum()), data_sum=math.fsum(costs), sum_abs=math.fsum(abs(v) for v in costs),
                n_data=len(costs))


def energy(st, lamda):
    """E = lamda * data_sum + smooth_sum, in double."""
    return float(lamda) * st["data_sum"] + float(st["smooth_sum"])
