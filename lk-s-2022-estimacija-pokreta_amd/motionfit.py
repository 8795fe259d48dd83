#!/usr/bin/env python3
"""The dominant motion of a flow field (DESIGN.md "Global-motion fit"); no counterpart in the reference.

    python motionfit.py <flow> [--model affine|homography] [--thresh T] [--hyp N] [--lo-rounds R] [--polish P] [--step S]
                        [--seed S] [--model-flow OUT.flo] [--residual OUT.flo] [--classes OUT.png] [--layers K] [--json]

Fits an affine map or a homography M: (x,y,1) -> (X,Y,W), position in the second frame (X/W, Y/W), to <flow> by random minimal
samples (pipeline.motion_fit: N hypotheses per round, default 1024; R further rounds sampled among the best model's inliers,
default 1; P least-squares polish steps of an affine map, default 2; a vector agrees with a model when it ends within T pixels,
default 1, of where the model sends its pixel; --step S scores every S-th row and column only) and prints the model and the
fraction of the scored vectors that agree with it.  --model-flow writes the model's own flow, which `daisy i flann.py --prior`
takes as it is; --residual the flow minus the model's; --classes a grey picture: 0 no vector, 85 agrees, 170 does not, 255
excluded.  --layers K fits K models one after the other, each to the vectors that agreed with none before it
(pipeline.motion_layers), and prints every one; --classes then holds the layer map, 255 // K per layer, and --model-flow and
--residual are refused.  --json prints one JSON object instead of the text.
<flow>: '.flo' (Middlebury [u,v], every pixel valid) or '.npy': (H,W,2) the hot path's [dy,dx] fields, (H,W,3) [U,V,valid].
'.flo' outputs hold [u,v], a pixel without a vector as (0,0).  Usage errors and unreadable input exit with status 2 before any
GPU work.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("flow")
    ap.add_argument("--model", choices=("affine", "homography"), default="affine")
    ap.add_argument("--thresh", type=float, default=1.0, metavar="T")
    ap.add_argument("--hyp", type=int, default=1024, metavar="N")
    ap.add_argument("--lo-rounds", type=int, default=1, metavar="R")
    ap.add_argument("--polish", type=int, default=2, metavar="P")
    ap.add_argument("--step", type=int, default=1, metavar="S")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model-flow", default=None, metavar="OUT.flo")
    ap.add_argument("--residual", default=None, metavar="OUT.flo")
    ap.add_argument("--classes", default=None, metavar="OUT.png")
    ap.add_argument("--layers", type=int, default=None, metavar="K")
    ap.add_argument("--json", action="store_true")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    cli.positive(ap, "--thresh", a.thresh)
    for name, v, lo, hi in (("--hyp", a.hyp, 1, 65536), ("--lo-rounds", a.lo_rounds, 0, 4), ("--polish", a.polish, 0, 4),
                            ("--step", a.step, 1, 64), ("--seed", a.seed, 0, 2 ** 64 - 1), ("--layers", a.layers, 1, 255)):
        cli.in_range(ap, name, v, lo, hi)
    if a.layers is not None and (a.model_flow is not None or a.residual is not None):
        ap.error("--model-flow and --residual describe one model: they do not go with --layers")
    for name, path, ext in (("--model-flow", a.model_flow, ".flo"), ("--residual", a.residual, ".flo"), ("--classes", a.classes, ".png")):
        cli.extension(ap, name, path, ext)
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        flow = flowio.read_flow(a.flow)
    except cli.REFUSED as e:
        return cli.refuse("motionfit", e)
    pipeline = cli.mod("pipeline")
    args = dict(model=a.model, thresh=a.thresh, n_hyp=a.hyp, lo_rounds=a.lo_rounds, polish=a.polish, step=a.step, seed=a.seed)
    if a.layers is not None:
        models, layers = pipeline.motion_layers(flow, a.layers, **args)
        layers = layers.cpu().numpy()
        models = [m.cpu().numpy() for m in models]
        good = flow[..., 2] > 0.5 if flow.shape[2] == 3 else np.ones(flow.shape[:2], bool)
        good &= np.isfinite(flow[..., :2]).all(axis=2)
        shares = [float((layers == i + 1).sum()) / max(int(good.sum()), 1) for i in range(a.layers)]
        if a.classes is not None:
            flowio.write_grey(a.classes, layers, 255 // a.layers)
        cli.report(a.json, dict(model=a.model, layers=[dict(matrix=m.tolist(), share=s) for m, s in zip(models, shares)]),
                   ["layer %d: %s; %.2f%% of the vectors" % (i + 1, " ".join("%.9g" % v for v in m.reshape(-1)), 100.0 * s)
                    for i, (m, s) in enumerate(zip(models, shares))])
        return 0
    m, cls, mflow, res, cnt = pipeline.motion_fit(flow, classes=True, model_flow=True, residual=True, counts=True, **args)
    cnt = dict(zip(pipeline.MOTION_FIT_COUNTS, cnt.cpu().tolist()))
    m = m.cpu().numpy()
    if a.model_flow is not None:
        flowio.write_field(a.model_flow, mflow.cpu().numpy())
    if a.residual is not None:
        flowio.write_field(a.residual, res.cpu().numpy())
    if a.classes is not None:
        flowio.write_grey(a.classes, cls.cpu().numpy(), 85)
    fraction, line = cli.inliers(cnt["inliers"], cnt["scored"], cnt["best_j"] >= 0)
    cli.report(a.json, dict(model=a.model, matrix=m.tolist(), inlier_fraction=fraction, **cnt),
               ["%s model: %s" % (a.model, " ".join("%.9g" % v for v in m.reshape(-1))), line])
    return 0


if __name__ == "__main__":
    sys.exit(main())
