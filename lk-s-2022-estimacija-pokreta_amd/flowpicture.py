#!/usr/bin/env python3
"""Looking at a flow without a ground truth (DESIGN.md "Flow pictures and the warp check"); no counterpart in the reference.

    python flowpicture.py <flow> <picture> [--max-flow M]
    python flowpicture.py <flow> --warp <img1> <img2> [--warped P] [--error-picture P] [--err-thresh T] [--err-max E]

The first form writes the Middlebury colour-wheel picture of the flow (pipeline.flow_color): hue = direction, saturation =
length over M, by default over the largest flow of the field; black where the flow is unknown.
The second form warps <img2> back onto <img1> by the flow (pipeline.warp_eval) and prints the mean photometric error (grey
levels, the mean absolute difference of the three channels), the share of pixels above T (default 10), and how many pixels
were compared and how many targets lie outside the frame or are unknown; --warped writes the warped second image,
--error-picture the jet picture of min(err, E) / E (E default 30).  T and E are this build's defaults.  Both forms may be
combined.
Flows are read with evaluate.ucitajFlow ('.png' KITTI, '.npy' the hot path's fields, '.flo' Middlebury), images with
flowio.read_image as '.npy' ((H,W,3) uint8 BGR), '.ppm' (binary P6) or '.png' (8-bit RGB or grey); pictures are written with
flowio.write_picture ('.png' and '.ppm' always, anything else through PIL if it can be imported).
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
    ap.add_argument("picture", nargs="?", default=None, help="where the colour picture of the flow goes")
    ap.add_argument("--max-flow", type=float, default=None, help="flow length at which the colours saturate (default: the field's maximum)")
    ap.add_argument("--warp", nargs=2, metavar=("IMG1", "IMG2"), default=None, help="the two frames: run the warp check")
    ap.add_argument("--warped", default=None, help="with --warp: where the warped second image goes")
    ap.add_argument("--error-picture", default=None, help="with --warp: where the colour picture of the photometric error goes")
    ap.add_argument("--err-thresh", type=float, default=10.0)
    ap.add_argument("--err-max", type=float, default=30.0)
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.picture is None and a.warp is None:
        ap.error("nothing to do: give a picture path, --warp, or both")
    if a.warp is None and (a.warped or a.error_picture):
        ap.error("--warped and --error-picture need --warp")
    evaluate, pipeline, flowio = cli.mod("evaluate"), cli.mod("pipeline"), cli.mod("flowio")
    read_image, write_picture = flowio.read_image, flowio.write_picture
    flow = evaluate.ucitajFlow(a.flow)
    if a.picture is not None:
        write_picture(a.picture, pipeline.flow_color(flow, a.max_flow).cpu().numpy())
    if a.warp is not None:
        img1, img2 = (read_image(p) for p in a.warp)
        if img1.shape != img2.shape or img1.shape[:2] != flow.shape[:2]:
            return cli.refuse("flowpicture", "the flow is %dx%d, the images %dx%d and %dx%d"
                              % (flow.shape[1], flow.shape[0], img1.shape[1], img1.shape[0], img2.shape[1], img2.shape[0]))
        out = pipeline.warp_eval(img1, img2, flow, a.err_thresh, a.err_max, warped=a.warped is not None,
                                 image=a.error_picture is not None)
        out = out if isinstance(out, tuple) else (out,)
        st = pipeline.photo_stats(out[0])
        print("mean photometric error %.4f, %.2f%% above %g, over %d px; %d targets outside the frame, %d unknown"
              % (st["mean_err"], st["above_pct"], a.err_thresh, st["n"], st["n_outside"], st["n_unknown"]))
        rest = list(out[1:])
        if a.warped is not None:
            write_picture(a.warped, rest.pop(0).cpu().numpy())
        if a.error_picture is not None:
            write_picture(a.error_picture, rest.pop(0).cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
