#!/usr/bin/env python3
"""Superpixels of an image and an affine flow model per superpixel (DESIGN.md "Superpixels and per-segment flow models"); no
counterpart in the reference.

    python superpixels.py <image> OUT.npy|OUT.png [--step S] [--compactness M] [--iters N] [--min-size P] [--boundaries OUT.png]
                          [--flow FLOW --fit OUT.flo [--thresh T] [--rounds R] [--classes OUT.png] [--models OUT.npy]] [--json]

Segments <image> ('.npy', '.png' or '.ppm'; (H,W,3) uint8 BGR) into compact regions of similar colour (pipeline.superpixels: an
integer gSLIC on a grid of S pixels, default 16, N iterations, default 10, spatial weight M in [0,255], default 10; segments are
4-connected, have at least P pixels, default S*S/4, and are numbered in raster order) and writes the segment numbers: an (H,W)
int32 '.npy', or a '.png' whose colour is the number (b = n & 255, g = n >> 8 & 255, r = n >> 16).  --boundaries writes the image
with the segment boundaries in red.
With --flow and --fit, an affine model is fitted to the vectors of FLOW in every segment (pipeline.segment_fit: least squares
trimmed in R rounds, default 3, whose thresholds halve down to T pixels, default 1) and the models' own flow is written to
OUT.flo (or an (H,W,3) [U,V,valid] '.npy'): a piecewise-affine version of FLOW in which holes inside a segment are filled.
--classes writes a grey picture: 0 no vector, 85 agrees, 170 does not, 255 no model; --models the (n_seg,6) float32 models.
FLOW: '.flo' (Middlebury [u,v], every pixel valid) or '.npy': (H,W,2) the hot path's [dy,dx] fields, (H,W,3) [U,V,valid].
--json prints one JSON object instead of the text.  Usage errors and unreadable input exit with status 2 before any GPU work.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")
MAX_MIN_SIZE = 1 << 26


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("image")
    ap.add_argument("out", metavar="OUT.npy|OUT.png")
    ap.add_argument("--step", type=int, default=16, metavar="S")
    ap.add_argument("--compactness", type=int, default=10, metavar="M")
    ap.add_argument("--iters", type=int, default=10, metavar="N")
    ap.add_argument("--min-size", type=int, default=None, metavar="P")
    ap.add_argument("--boundaries", default=None, metavar="OUT.png")
    ap.add_argument("--flow", default=None, metavar="FLOW")
    ap.add_argument("--fit", default=None, metavar="OUT.flo")
    ap.add_argument("--thresh", type=float, default=None, metavar="T")
    ap.add_argument("--rounds", type=int, default=None, metavar="R")
    ap.add_argument("--classes", default=None, metavar="OUT.png")
    ap.add_argument("--models", default=None, metavar="OUT.npy")
    ap.add_argument("--json", action="store_true")
    return ap


def label_picture(labels, np):
    """The segment numbers as a BGR picture: b = n & 255, g = n >> 8 & 255, r = n >> 16."""
    n = labels.astype(np.uint32)
    return np.stack([n & 255, (n >> 8) & 255, (n >> 16) & 255], axis=2).astype(np.uint8)


def boundary_picture(img, labels, np):
    """The image with every pixel whose right or lower neighbour lies in another segment painted red."""
    edge = np.zeros(labels.shape, bool)
    edge[:, :-1] |= labels[:, :-1] != labels[:, 1:]
    edge[:-1, :] |= labels[:-1, :] != labels[1:, :]
    out = img.copy()
    out[edge] = (0, 0, 255)
    return out


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    for name, v, lo, hi in (("--step", a.step, 4, 64), ("--compactness", a.compactness, 0, 255), ("--iters", a.iters, 1, 32),
                            ("--min-size", a.min_size, 0, MAX_MIN_SIZE), ("--rounds", a.rounds, 1, 6)):
        cli.in_range(ap, name, v, lo, hi)
    cli.positive(ap, "--thresh", a.thresh)
    if (a.flow is None) != (a.fit is None):
        ap.error("--flow and --fit go together")
    if a.flow is None:
        for name, v in (("--thresh", a.thresh), ("--rounds", a.rounds), ("--classes", a.classes), ("--models", a.models)):
            if v is not None:
                ap.error("%s needs --flow and --fit" % name)
    for name, path, exts in (("OUT", a.out, (".npy", ".png")), ("--boundaries", a.boundaries, (".png",)), ("--fit", a.fit, (".flo", ".npy")),
                             ("--classes", a.classes, (".png",)), ("--models", a.models, (".npy",))):
        cli.extension(ap, name, path, *exts)
    thresh, rounds = 1.0 if a.thresh is None else a.thresh, 3 if a.rounds is None else a.rounds
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        img = flowio.read_image(a.image)
        flow = None if a.flow is None else flowio.read_flow(a.flow)
        if flow is not None and flow.shape[:2] != img.shape[:2]:
            raise ValueError("%s is %dx%d, %s is %dx%d" % (a.flow, flow.shape[1], flow.shape[0], a.image, img.shape[1], img.shape[0]))
    except cli.REFUSED as e:
        return cli.refuse("superpixels", e)
    pipeline = cli.mod("pipeline")
    args = dict(step=a.step, compactness=a.compactness, iters=a.iters, min_size=a.min_size)
    report = {}
    if flow is None:
        labels, cnt = pipeline.superpixels(img, counts=True, **args)
    else:
        labels, models, seg_counts, out, cls, fit_cnt = pipeline.superpixel_flow(img, flow, thresh=thresh, rounds=rounds, classes=True,
                                                                                 counts=True, **args)
        cnt = None
        report = dict(zip(pipeline.SEGMENT_FIT_COUNTS[:7], fit_cnt.cpu().tolist()))
        flowio.write_field(a.fit, out.cpu().numpy())
        if a.classes is not None:
            flowio.write_grey(a.classes, cls.cpu().numpy(), 85)
        if a.models is not None:
            np.save(a.models, models.cpu().numpy())
    labels = labels.cpu().numpy()
    sizes = np.bincount(labels.ravel())
    report = dict(dict(n_seg=int(sizes.size), smallest=int(sizes.min()), largest=int(sizes.max())), **report)
    if cnt is not None:
        report.update(zip(pipeline.SUPERPIXEL_COUNTS[:5], cnt.cpu().tolist()[:5]))
    if a.out.lower().endswith(".npy"):
        np.save(a.out, labels)
    else:
        flowio.write_png8(a.out, label_picture(labels, np))
    if a.boundaries is not None:
        flowio.write_png8(a.boundaries, boundary_picture(img, labels, np))
    lines = ["segments: %d, of %d to %d pixels" % (report["n_seg"], report["smallest"], report["largest"])]
    if flow is not None:
        lines.append("models: %d affine, %d translations; %d of %d vectors agree to within %g px"
                     % (report["affine"], report["translation"], report["agree"], report["part"], thresh))
    cli.report(a.json, report, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
