#!/usr/bin/env python3
"""Sparse feature tracks through an image sequence, without a dense pass (DESIGN.md "Sparse feature tracking"); no counterpart in
the reference.

    python klt.py IMG0 IMG1 [IMG2 ...] --out tracks.npz [--levels L] [--radius R] [--iters N] [--min-dist D] [--quality Q]
                  [--fb T] [--max-err E] [--reseed] [--cap N] [--flow A B OUT.flo] [--epic OUT.flo] [--json]

Tracks start at the Shi-Tomasi corners of IMG0 (window radius 2, at least D + 1 pixels apart, response at least Q times the
strongest; defaults 4 and 0.01) and are carried from frame to frame by pyramidal Lucas-Kanade (pipeline.TrackSet.advance_klt): L
pyramid levels (default 3), a (2R+1)^2 window (default 7), at most N steps per level (default 20).  A track ends when it leaves
the frame, when its window is flat, when its mean absolute residual exceeds E grey levels (default 0: no test) or when tracking
back does not return within T pixels (default 0.5; 0: no backward pass).  --reseed starts new tracks after every frame at the
corners no live track is near.  --cap N is the number of tracks the set can hold (default: one per 16 pixels); corners beyond it
are dropped.
--out receives tracks.py's arrays: pos (T,n,2) float32 [x,y], NaN before a track's birth and its last position repeated after its
end; state (T,n) int32, 0 free / 1 live / 2 left / 5 inconsistent / 6 flat / 7 residual; birth (n) and length (n).  --flow A B
OUT.flo writes the displacement of the tracks alive in frames A and B as a flow A -> B, (0,0) where there is none.  --epic OUT.flo
writes the dense flow IMG0 -> IMG1 that pipeline.epic_interpolate makes of the first pair's sparse field, with pipeline.pb_edges
of IMG0 as the edge map.  The counts per state after the last frame are printed, as one JSON object with --json.
Images: '.npy' ((H,W,3) uint8 BGR), '.png' or '.ppm'.  Usage errors and unreadable input exit with status 2 before any GPU work,
and before anything is written.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("images", nargs="+", metavar="IMG")
    ap.add_argument("--out", required=True, metavar="tracks.npz")
    ap.add_argument("--levels", type=int, default=3, metavar="L")
    ap.add_argument("--radius", type=int, default=7, metavar="R")
    ap.add_argument("--iters", type=int, default=20, metavar="N")
    ap.add_argument("--min-dist", type=int, default=4, metavar="D")
    ap.add_argument("--quality", type=float, default=0.01, metavar="Q")
    ap.add_argument("--fb", type=float, default=0.5, metavar="T")
    ap.add_argument("--max-err", type=float, default=0.0, metavar="E")
    ap.add_argument("--reseed", action="store_true")
    ap.add_argument("--cap", type=int, default=None, metavar="N")
    ap.add_argument("--flow", nargs=3, default=None, metavar=("A", "B", "OUT.flo"))
    ap.add_argument("--epic", default=None, metavar="OUT.flo")
    ap.add_argument("--json", action="store_true")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    T = len(a.images)
    if T < 2:
        ap.error("at least two images are needed")
    cli.extension(ap, "--out", a.out, ".npz")
    cli.in_range(ap, "--levels", a.levels, 1, 8)
    cli.in_range(ap, "--radius", a.radius, 1, 10)
    cli.in_range(ap, "--iters", a.iters, 1, 64)
    cli.in_range(ap, "--min-dist", a.min_dist, 1, 32)
    cli.non_negative(ap, "--quality", a.quality)
    if a.quality > 1:
        ap.error("--quality must be at most 1")
    cli.non_negative(ap, "--fb", a.fb)
    cli.non_negative(ap, "--max-err", a.max_err)
    cli.in_range(ap, "--cap", a.cap, 1, 1 << 26)
    span = None
    if a.flow is not None:
        try:
            span = (int(a.flow[0]), int(a.flow[1]))
        except ValueError:
            ap.error("--flow needs two frame numbers and a file")
        for t in span:
            cli.in_range(ap, "--flow: frames", t, 0, T - 1)
        cli.extension(ap, "--flow: the output", a.flow[2], ".flo")
    cli.extension(ap, "--epic", a.epic, ".flo")
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        imgs = [flowio.read_image(p) for p in a.images]
        for p, img in zip(a.images, imgs):
            if img.shape != imgs[0].shape:
                raise ValueError("%s: a %dx%d image among %dx%d ones" % (p, img.shape[1], img.shape[0], imgs[0].shape[1], imgs[0].shape[0]))
        if max(imgs[0].shape[:2]) > 8192:
            raise ValueError("%s: frames are at most 8192x8192" % a.images[0])
    except cli.REFUSED as e:
        return cli.refuse("klt", e)
    pipeline = cli.mod("pipeline")
    H, W = imgs[0].shape[:2]
    corner_args = dict(min_dist=a.min_dist, quality=a.quality)
    ts = pipeline.TrackSet(H, W, cap=a.cap if a.cap is not None else max(1, H * W // 16), step=1)
    pyr = pipeline.klt_pyramid(imgs[0], a.levels)
    ts.seed_corners(pyr, **corner_args)
    dropped = ts.counts()["seed"][3:4].clone()
    for img in imgs[1:]:
        nxt = pipeline.klt_pyramid(img, a.levels)
        ts.advance_klt(pyr, nxt, levels=a.levels, r=a.radius, iters=a.iters, fb=a.fb, max_err=a.max_err)
        pyr = nxt
        if a.reseed:
            ts.seed_corners(pyr, **corner_args)
            dropped += ts.counts()["seed"][3:4]
    sparse = ts.flow(*span) if span is not None else None
    dense = pipeline.epic_interpolate(ts.flow(0, 1), pipeline.pb_edges(imgs[0])) if a.epic is not None else None
    got = ts.read()
    np.savez(a.out, **got)
    if sparse is not None:
        flowio.write_field(a.flow[2], sparse.cpu().numpy())
    if dense is not None:
        flowio.write_flo(a.epic, dense.cpu().numpy())
    last = got["state"][-1]
    names = [(k, name) for k, name in enumerate(pipeline.TRACK_STATES_KLT) if name in ("live", "left", "inconsistent", "flat", "residual")]
    summary = dict(frames=T, tracks=int(len(last)), dropped=int(dropped.cpu()[0]), **{name: int((last == k).sum()) for k, name in names})
    lines = ["%d frames, %d tracks (%d corners dropped): %s" % (T, summary["tracks"], summary["dropped"], ", ".join(
        "%d %s" % (summary[name], name) for _, name in names))]
    if span is not None:
        summary["flow_vectors"] = int((sparse[..., 2] > 0.5).sum().cpu())
        lines.append("flow %d -> %d: %d vectors" % (span[0], span[1], summary["flow_vectors"]))
    if dense is not None:
        lines.append("dense flow 0 -> 1 written to %s" % a.epic)
    cli.report(a.json, summary, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
