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
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
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


def read_flow(path, flowio, np):
    """-> (H,W,2) [dy,dx] or (H,W,3) [U,V,valid] float32; ValueError for anything else."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".flo":
        return np.ascontiguousarray(flowio.read_flo(path)[..., ::-1])
    if ext == ".npy":
        flow = np.load(path)
        if flow.ndim != 3 or flow.shape[2] not in (2, 3):
            raise ValueError("%s: expected an (H,W,2) or (H,W,3) array, got %s" % (path, flow.shape))
        return np.ascontiguousarray(flow, dtype=np.float32)
    raise ValueError("unsupported flow file: %s" % path)


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    finite_pos = lambda v: v == v and 0.0 < v < float("inf")
    if not 1 <= a.radius <= 8:
        ap.error("--radius must lie in [1, 8]")
    if a.sigma_space is not None and not finite_pos(a.sigma_space):
        ap.error("--sigma-space must be finite and > 0")
    if not finite_pos(a.sigma_color):
        ap.error("--sigma-color must be finite and > 0")
    if not 1 <= a.iterations <= 16:
        ap.error("--iterations must lie in [1, 16]")
    if a.reject is not None and not 0.0 <= a.reject < float("inf"):
        ap.error("--reject must be finite and >= 0")
    if a.reject is not None and a.iterations > 1:
        ap.error("--reject goes with one pass, not with --iterations")
    if os.path.splitext(a.out)[1].lower() not in (".flo", ".npy"):
        ap.error("<out> must be a .flo or a .npy file")
    import numpy as np
    flowio = importlib.import_module(PKG + ".flowio")
    try:
        flow = read_flow(a.flow, flowio, np)
        img = flowio.read_image(a.image) if a.image is not None else None
    except (ValueError, OSError) as e:
        print("flowfilter: %s" % e, file=sys.stderr)
        return 2
    if img is not None and img.shape[:2] != flow.shape[:2]:
        print("flowfilter: the flow is %dx%d and the image %dx%d" % (flow.shape[1], flow.shape[0], img.shape[1], img.shape[0]), file=sys.stderr)
        return 2
    pipeline = importlib.import_module(PKG + ".pipeline")
    out, cnt = pipeline.flow_wmedian(flow, img, radius=a.radius, sigma_space=a.sigma_space, sigma_color=a.sigma_color,
                                     iterations=a.iterations, keep_holes=a.keep_holes, reject=a.reject, counts=True)
    out = out.cpu().numpy()
    if os.path.splitext(a.out)[1].lower() == ".flo":
        flowio.write_flo(a.out, out[..., [1, 0]])
    else:
        np.save(a.out, out)
    if a.counts:
        print(" ".join("%s=%d" % kv for kv in zip(pipeline.FLOW_WMEDIAN_COUNTS, cnt.cpu().tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
