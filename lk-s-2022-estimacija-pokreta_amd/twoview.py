#!/usr/bin/env python3
"""Where the camera went and how far away things are, from one flow field (DESIGN.md "Two-view reconstruction"); no counterpart
in the reference.

    python twoview.py <flow> [--focal F | --intrinsics FX FY CX CY] [--thresh T] [--hyp N] [--lo-rounds R] [--step S] [--seed S]
                      [--depth OUT.npy] [--classes OUT.png] [--err OUT.npy] [--json]

Fits the fundamental matrix of <flow> (pipeline.epipolar_fit with --thresh, --hyp, --lo-rounds, --step and --seed as in
epipolar.py), then, with the camera's intrinsics and the fit's inliers as the voters, takes the essential matrix apart
(pipeline.two_view): the rotation R and the unit translation t of the second camera, X2 = R X1 + t, chosen among the four
candidates by how many voters lie in front of both cameras.  Both stages run on the device and nothing is read back until the end.
--focal F is the focal length in pixels (default max(H, W)) with the principal point at the frame's centre; --intrinsics gives
fx, fy, cx and cy.  Prints the rotation's angle and axis, t, the votes and the class counts.  --depth writes the (H,W) float32
depth in camera 1 in units of the baseline (0 where there is no vector or no parallax; negative behind the camera); --classes
a grey picture: 0 no vector, 85 in front of both cameras, 170 behind one (it moves against the epipolar direction), 255 no
parallax or no pose; --err the (H,W) float32 reprojection error in pixels (-1 no vector, inf none).  --json prints one JSON
object instead of the text.
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
    cam = ap.add_mutually_exclusive_group()
    cam.add_argument("--focal", type=float, default=None, metavar="F")
    cam.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--thresh", type=float, default=1.0, metavar="T")
    ap.add_argument("--hyp", type=int, default=512, metavar="N")
    ap.add_argument("--lo-rounds", type=int, default=1, metavar="R")
    ap.add_argument("--step", type=int, default=1, metavar="S")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--depth", default=None, metavar="OUT.npy")
    ap.add_argument("--classes", default=None, metavar="OUT.png")
    ap.add_argument("--err", default=None, metavar="OUT.npy")
    ap.add_argument("--json", action="store_true")
    return ap


def camera(a):
    """(focal, center) for pipeline.two_view from the parsed options, or a message."""
    try:
        if a.intrinsics is not None:
            fx, fy, cx, cy = a.intrinsics
            return ((cli.real(fx, True), cli.real(fy, True)), (cli.real(cx, None), cli.real(cy, None))), None
        return (None if a.focal is None else cli.real(a.focal, True), None), None
    except ValueError:
        return None, ("--focal %s" if a.intrinsics is None else "--intrinsics: FX and FY %s, CX and CY finite") % cli.POSITIVE


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    cli.positive(ap, "--thresh", a.thresh)
    for name, v, lo, hi in (("--hyp", a.hyp, 1, MAX_HYP), ("--lo-rounds", a.lo_rounds, 0, 4), ("--step", a.step, 1, 64),
                            ("--seed", a.seed, 0, 2 ** 64 - 1)):
        cli.in_range(ap, name, v, lo, hi)
    cam, msg = camera(a)
    if msg:
        ap.error(msg)
    for name, path, ext in (("--depth", a.depth, ".npy"), ("--classes", a.classes, ".png"), ("--err", a.err, ".npy")):
        cli.extension(ap, name, path, ext)
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        flow = flowio.read_flow(a.flow)
    except cli.REFUSED as e:
        return cli.refuse("twoview", e)
    pipeline = cli.mod("pipeline")
    import torch
    flow = torch.from_numpy(np.ascontiguousarray(flow)).cuda()
    m, fit_cls, fit_cnt = pipeline.epipolar_fit(flow, thresh=a.thresh, n_hyp=a.hyp, lo_rounds=a.lo_rounds, step=a.step, seed=a.seed,
                                                classes=True, counts=True)
    pose, depth, cls, err, cnt = pipeline.two_view(flow, m, focal=cam[0], center=cam[1], part=fit_cls, step=a.step, depth=True,
                                                   classes=True, err=True, counts=True)
    # the one read-back, after both stages have been queued
    pose, fit_cnt, cnt = pose.cpu().numpy(), fit_cnt.cpu().tolist(), dict(zip(pipeline.TWO_VIEW_COUNTS[:7], cnt.cpu().tolist()))
    info = pipeline.two_view_pose(pose)
    if a.depth is not None:
        np.save(a.depth, depth.cpu().numpy())
    if a.classes is not None:
        flowio.write_grey(a.classes, cls.cpu().numpy(), 85)
    if a.err is not None:
        np.save(a.err, err.cpu().numpy())
    axis = None if info["axis"] is None else info["axis"].tolist()
    if info["candidate"] < 0:
        lines = ["no pose: %d voters, %d of %d scored vectors agree with a fundamental matrix" % (cnt["voters"], fit_cnt[1], fit_cnt[0])]
    else:
        lines = ["rotation: %.6f deg about (%s)" % (info["angle_deg"], "none" if axis is None else " ".join("%.6f" % v for v in axis)),
                 "t: %s" % " ".join("%.9g" % v for v in info["t"]),
                 "votes: %d of %d voters for candidate %d, %d for the runner-up" % (cnt["votes"], cnt["voters"], cnt["candidate"], cnt["runner_up"]),
                 "pixels: %d in front of both cameras, %d behind one, %d without parallax" % (cnt["front"], cnt["behind"], cnt["flat"])]
    cli.report(a.json, dict(model=m.cpu().numpy().tolist(), pose=pose.tolist(), R=info["R"].tolist(), t=info["t"].tolist(),
                            angle_deg=info["angle_deg"], axis=axis, singular=info["singular"].tolist(), fit_inliers=fit_cnt[1],
                            fit_scored=fit_cnt[0], **cnt), lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
