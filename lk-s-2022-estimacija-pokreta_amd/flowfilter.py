#!/usr/bin/env python3
"""The edge-aware weighted median filter of a flow field (DESIGN.md "Weighted median filter"); no counterpart in the reference.

    python flowfilter.py <flow> <out> [--image IMG] [--radius R] [--sigma-space S] [--sigma-color C] [--iterations N]
                         [--keep-holes] [--reject T] [--counts]

Every pixel of <flow> gets, per component, the weighted median of the good vectors in the (2R + 1)^2 window around it
(pipeline.flow_wmedian; R = 3 by default, 1..8).  With --image the weights follow the similarity of IMG's colours (--sigma-color,
grey levels per channel, default 10): the flow's edges move onto the image's.  --sigma-space weighs near pixels more (default:
every distance alike).  Pixels without a good vector are filled from their windows unless --keep-holes is given.  --iterations N
(1..16) filters N times.  --reject T filters nothing: a vector further than T from the median of its window, in |dU| + |dV|,
is removed and every other one is kept bit for bit (one pass).  --counts prints {good, valid, filled, altered} of the last pass.
<flow>: '.flo' (Middlebury [u,v], every pixel valid) or '.npy': (H,W,2) the hot path's [dy,dx] fields, (H,W,3) [U,V,valid] as
this script and run_batch.py (sparse_field_NN.npy) write it.  <out>: '.flo' ([u,v]; a pixel without a vector is written as
(0,0)) or '.npy' as [U,V,valid].  IMG is read with flowio.read_image ('.npy', '.png', '.ppm').  Usage errors, unreadable input and
inputs of different sizes exit with status 2 before any GPU work.
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
    ap.add_argument("out")
    ap.add_argument("--image", default=None, metavar="IMG", help="the guide image")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--sigma-space", type=float, default=None)
    ap.add_argument("--sigma-color", type=float, default=10.0)
    ap.add_argument("--iterations", type=int, default=1)
    ap.add_argument("--keep-holes", action="store_true")
    ap.add_argument("--reject", type=float, default=None, metavar="T")
    ap.add_argument("--counts", action="store_true")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    cli.in_range(ap, "--radius", a.radius, 1, 8)
    cli.positive(ap, "--sigma-space", a.sigma_space)
    cli.positive(ap, "--sigma-color", a.sigma_color)
    cli.in_range(ap, "--iterations", a.iterations, 1, 16)
    cli.non_negative(ap, "--reject", a.reject)
    if a.reject is not None and a.iterations > 1:
        ap.error("--reject goes with one pass, not with --iterations")
    cli.extension(ap, "<out>", a.out, ".flo", ".npy")
    flowio = cli.mod("flowio")
    try:
        flow = flowio.read_flow(a.flow)
        img = flowio.read_image(a.image) if a.image is not None else None
        if img is not None and img.shape[:2] != flow.shape[:2]:
            raise ValueError("the flow is %dx%d and the image %dx%d" % (flow.shape[1], flow.shape[0], img.shape[1], img.shape[0]))
    except cli.REFUSED as e:
        return cli.refuse("flowfilter", e)
    pipeline = cli.mod("pipeline")
    out, cnt = pipeline.flow_wmedian(flow, img, radius=a.radius, sigma_space=a.sigma_space, sigma_color=a.sigma_color,
                                     iterations=a.iterations, keep_holes=a.keep_holes, reject=a.reject, counts=True)
    flowio.write_field(a.out, out.cpu().numpy())
    if a.counts:
        print(" ".join("%s=%d" % kv for kv in zip(pipeline.FLOW_WMEDIAN_COUNTS, cnt.cpu().tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
