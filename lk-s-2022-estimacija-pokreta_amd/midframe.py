#!/usr/bin/env python3
"""The frame between two frames from their flow (DESIGN.md "Frame interpolation"); no counterpart in the reference.

    python midframe.py <img1> <img2> <fwd> <out.png> [--backward BWD] [--t T | --frames N] [--fill-rounds K] [--occl-thresh D]
                       [--source FILE.png]

Writes the frame at time T (default 0.5) between <img1> (time 0) and <img2> (time 1), carried along the forward flow <fwd>
and, with --backward, along the backward flow too (pipeline.frame_interp).  With --frames N it writes the N frames at
t = k / (N + 1) as <out>_01.png .. <out>_NN.png (pipeline.frame_sequence).  K (default 8) rounds fill the pixels no vector
lands on from their neighbours; where the two frames, sampled along a pixel's motion, differ by more than D grey levels
(default 30) only the frame the motion came from is used.  Both are this build's defaults.  --source (single frame only)
writes where each pixel's motion came from: black none, blue <img1>, red <img2>, grey filled.
Per frame one line is printed: t and the eight counts {from1, from2, filled, unknown, blended, one_sided, fallback, lost}.
Flows are read with evaluate.ucitajFlow ('.npy' the hot path's [dy,dx] fields or a 3-channel field, '.flo' Middlebury, '.png'
KITTI), images with flowio.read_image, pictures are written with flowio.write_picture, as flowpicture.py does.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")

SOURCE_BGR = ((0, 0, 0), (255, 96, 0), (0, 96, 255), (128, 128, 128))      # none, img1, img2, filled


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("img1")
    ap.add_argument("img2")
    ap.add_argument("fwd", help="the flow of img1's pixels")
    ap.add_argument("out", help="where the frame goes; with --frames the stem of the numbered frames")
    ap.add_argument("--backward", default=None, metavar="BWD", help="the flow of img2's pixels: both sides claim")
    ap.add_argument("--t", type=float, default=None, help="the time of the frame, 0 < t < 1 (default 0.5)")
    ap.add_argument("--frames", type=int, default=None, metavar="N", help="write the N frames at t = k / (N + 1)")
    ap.add_argument("--fill-rounds", type=int, default=8)
    ap.add_argument("--occl-thresh", type=float, default=30.0)
    ap.add_argument("--source", default=None, metavar="FILE.png", help="where the provenance picture goes")
    return ap


def count_line(t, counts):
    return "t=%.6f " % t + " ".join("%s=%d" % kv for kv in zip(("from1", "from2", "filled", "unknown", "blended", "one_sided",
                                                                  "fallback", "lost"), counts))


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.t is not None and a.frames is not None:
        ap.error("--t and --frames exclude each other")
    cli.between(ap, "--t", a.t, 0.0, 1.0)
    cli.in_range(ap, "--frames", a.frames, 1, 99)
    cli.in_range(ap, "--fill-rounds", a.fill_rounds, 0, 64)
    cli.non_negative(ap, "--occl-thresh", a.occl_thresh)
    if a.source is not None and a.frames is not None:
        ap.error("--source goes with a single frame, not with --frames")
    import numpy as np
    evaluate, pipeline, flowio = cli.mod("evaluate"), cli.mod("pipeline"), cli.mod("flowio")
    img1, img2 = flowio.read_image(a.img1), flowio.read_image(a.img2)
    fwd = evaluate.ucitajFlow(a.fwd)
    bwd = evaluate.ucitajFlow(a.backward) if a.backward is not None else None
    sizes = [x.shape[:2] for x in (img1, img2, fwd) + ((bwd,) if bwd is not None else ())]
    if len(set(sizes)) != 1:
        return cli.refuse("midframe", "the images and the flows differ in size: %s" % ", ".join("%dx%d" % (s[1], s[0]) for s in sizes))
    if a.frames is not None:
        frames, counts = pipeline.frame_sequence(img1, img2, fwd, bwd, n=a.frames, fill_rounds=a.fill_rounds,
                                                 occl_thresh=a.occl_thresh, counts=True)
        for k, (frame, cnt) in enumerate(zip(frames, counts), 1):
            flowio.write_picture(flowio.numbered_name(a.out, k), frame.cpu().numpy())
            print(count_line(float(np.float32(k / (a.frames + 1))), cnt.cpu().tolist()))
        return 0
    t = 0.5 if a.t is None else a.t
    frame, src, cnt = pipeline.frame_interp(img1, img2, fwd, bwd, t=t, fill_rounds=a.fill_rounds, occl_thresh=a.occl_thresh,
                                            source=True, counts=True)
    flowio.write_picture(a.out, frame.cpu().numpy())
    if a.source is not None:
        flowio.write_picture(a.source, np.array(SOURCE_BGR, np.uint8)[src.cpu().numpy()])
    print(count_line(float(np.float32(t)), cnt.cpu().tolist()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
