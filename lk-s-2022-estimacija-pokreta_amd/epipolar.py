#!/usr/bin/env python3
"""The epipolar geometry of a flow field (DESIGN.md "Epipolar-geometry fit"); no counterpart in the reference.

    python epipolar.py <flow> [--thresh T] [--hyp N] [--lo-rounds R] [--step S] [--seed S]
                       [--classes OUT.png] [--residual OUT.npy] [--gate OUT.flo|OUT.npy] [--json]

Fits the fundamental matrix F, (x',y',1) F (x,y,1)^T = 0 for a pixel (x,y) and the place (x',y') its vector points to, to <flow>
by random 7-point samples (pipeline.epipolar_fit: N samples per round, default 512, each giving up to three models; R further
rounds sampled among the best model's inliers, default 1; a vector agrees with a model when its Sampson distance is at most T
pixels, default 1; --step S scores every S-th row and column only) and prints F in pixel coordinates, the two epipoles, the
focus of expansion and the fraction of the scored vectors that agree.  This is the model of a camera moving through a rigid
scene; vectors that disagree belong to things that move on their own, or are wrong.  A thing that moves along its own epipolar
line cannot be told from the scene (no orientation test is made).  --classes writes a grey picture: 0 no vector, 85 agrees, 170
does not, 255 excluded; --residual the (H,W) float32 Sampson distance in pixels, -1 where there is no vector; --gate the field
with the vectors that disagree removed and every other vector bit for bit: an (H,W,3) [U,V,valid] '.npy' with [0,0,0] there, or
a '.flo' with (0,0).  --json prints one JSON object instead of the text.
<flow>: '.flo' (Middlebury [u,v], every pixel valid) or '.npy': (H,W,2) the hot path's [dy,dx] fields, (H,W,3) [U,V,valid].
Usage errors and unreadable input exit with status 2 before any GPU work.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")
MAX_HYP = 21845


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("flow")
    ap.add_argument("--thresh", type=float, default=1.0, metavar="T")
    ap.add_argument("--hyp", type=int, default=512, metavar="N")
    ap.add_argument("--lo-rounds", type=int, default=1, metavar="R")
    ap.add_argument("--step", type=int, default=1, metavar="S")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--classes", default=None, metavar="OUT.png")
    ap.add_argument("--residual", default=None, metavar="OUT.npy")
    ap.add_argument("--gate", default=None, metavar="OUT.flo")
    ap.add_argument("--json", action="store_true")
    return ap


def gated(flow, cls, np):
    """The field without its outliers (class 2): (H,W,3) [U,V,valid], the survivors' U and V bit for bit."""
    h, w = cls.shape
    out = np.zeros((h, w, 3), np.float32)
    keep = (cls == 1) | (cls == 3)
    uv = flow[..., :2] if flow.shape[2] == 3 else flow[..., ::-1]
    out[..., :2][keep] = uv[keep]
    out[..., 2][keep] = 1.0
    return out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    cli.positive(ap, "--thresh", a.thresh)
    for name, v, lo, hi in (("--hyp", a.hyp, 1, MAX_HYP), ("--lo-rounds", a.lo_rounds, 0, 4), ("--step", a.step, 1, 64),
                            ("--seed", a.seed, 0, 2 ** 64 - 1)):
        cli.in_range(ap, name, v, lo, hi)
    cli.extension(ap, "--classes", a.classes, ".png")
    cli.extension(ap, "--residual", a.residual, ".npy")
    cli.extension(ap, "--gate", a.gate, ".flo", ".npy")
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        flow = flowio.read_flow(a.flow)
    except cli.REFUSED as e:
        return cli.refuse("epipolar", e)
    pipeline = cli.mod("pipeline")
    m, cls, res, cnt = pipeline.epipolar_fit(flow, thresh=a.thresh, n_hyp=a.hyp, lo_rounds=a.lo_rounds, step=a.step, seed=a.seed,
                                             classes=True, residual=True, counts=True)
    cnt = dict(zip(pipeline.EPIPOLAR_FIT_COUNTS[:7], cnt.cpu().tolist()))
    m, cls = m.cpu().numpy(), cls.cpu().numpy()
    h, w = cls.shape
    geo = pipeline.epipolar_geometry(m, h, w)
    if a.classes is not None:
        flowio.write_grey(a.classes, cls, 85)
    if a.residual is not None:
        np.save(a.residual, res.cpu().numpy())
    if a.gate is not None:
        flowio.write_field(a.gate, gated(flow, cls, np))
    fraction, line = cli.inliers(cnt["inliers"], cnt["scored"], cnt["best_slot"] >= 0)
    cli.report(a.json, dict(model=m.tolist(), F=geo["F"].tolist(), e1=geo["e1"].tolist(), e2=geo["e2"].tolist(), foe=geo["foe"],
                            inlier_fraction=fraction, **cnt),
               ["F: %s" % " ".join("%.9g" % v for v in geo["F"].reshape(-1)),
                "epipoles: (%s) (%s); focus of expansion: %s" % (" ".join("%.6g" % v for v in geo["e1"]), " ".join("%.6g" % v for v in geo["e2"]),
                                                                 "none" if geo["foe"] is None else "%.2f %.2f" % geo["foe"]), line])
    return 0


if __name__ == "__main__":
    sys.exit(main())
