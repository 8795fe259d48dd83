#!/usr/bin/env python3
"""Point trajectories through a frame sequence (DESIGN.md "Point trajectories"); no counterpart in the reference.

    python tracks.py FWD0.flo [FWD1.flo ...] [--backward BWD0.flo ...] [--step S] [--reseed] [--rel R] [--abs A] [--cap N]
                     --out tracks.npz [--flow A B OUT.flo] [--json]

FWDt is the flow from frame t to frame t+1 of a sequence of T+1 frames, BWDt (as many as there are FWD files) the flow from frame
t+1 back to frame t.  Tracks start at frame 0 in the centre pixel of every S x S cell (default 4) and are carried from frame to
frame by the bilinear sample of the forward flow (pipeline.TrackSet).  A track ends when it leaves the frame, meets a pixel without
a vector or, with --backward, fails the forward/backward test |f + b|^2 <= R (|f|^2 + |b|^2) + A (defaults 0.01 and 0.5).
--reseed starts new tracks after every frame in the cells no live track covers.  --cap N is the number of tracks the set can hold
(default: four per cell); cells beyond it are dropped.
--out receives pos (T+1,n,2) float32 [x,y], NaN before a track's birth and its last position repeated after its end; state
(T+1,n) int32, 0 free / 1 live / 2 left / 3 noflow / 4 noback / 5 inconsistent; birth (n) and length (n), the frames a track is
live in.  --flow A B OUT.flo writes the displacement of the tracks alive in frames A and B as a flow A -> B, (0,0) where there is
none.  The counts per state after the last frame are printed, as one JSON object with --json.
Flow files: '.flo' (Middlebury [u,v], every pixel valid) or '.npy': (H,W,2) the hot path's [dy,dx] fields, (H,W,3) [U,V,valid].
Usage errors and unreadable input exit with status 2 before any GPU work, and before anything is written.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("forward", nargs="+", metavar="FWD.flo")
    ap.add_argument("--backward", nargs="+", default=None, metavar="BWD.flo")
    ap.add_argument("--step", type=int, default=4, metavar="S")
    ap.add_argument("--reseed", action="store_true")
    ap.add_argument("--rel", type=float, default=0.01, metavar="R")
    ap.add_argument("--abs", type=float, default=0.5, metavar="A")
    ap.add_argument("--cap", type=int, default=None, metavar="N")
    ap.add_argument("--out", required=True, metavar="tracks.npz")
    ap.add_argument("--flow", nargs=3, default=None, metavar=("A", "B", "OUT.flo"))
    ap.add_argument("--json", action="store_true")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    T = len(a.forward)
    if a.backward is not None and len(a.backward) != T:
        ap.error("--backward needs as many files as there are forward flows (%d), got %d" % (T, len(a.backward)))
    cli.in_range(ap, "--step", a.step, 1, 256)
    cli.non_negative(ap, "--rel", a.rel)
    cli.non_negative(ap, "--abs", a.abs)
    cli.in_range(ap, "--cap", a.cap, 1, 1 << 26)
    cli.extension(ap, "--out", a.out, ".npz")
    span = None
    if a.flow is not None:
        try:
            span = (int(a.flow[0]), int(a.flow[1]))
        except ValueError:
            ap.error("--flow needs two frame numbers and a file")
        for t in span:
            cli.in_range(ap, "--flow: frames", t, 0, T)
        cli.extension(ap, "--flow: the output", a.flow[2], ".flo")
    import numpy as np
    flowio = cli.mod("flowio")
    try:
        fwd = [flowio.read_flow(p) for p in a.forward]
        bwd = [flowio.read_flow(p) for p in a.backward] if a.backward is not None else [None] * T
        for p, f in zip(a.forward + (a.backward or []), fwd + [b for b in bwd if b is not None]):
            if f.shape[:2] != fwd[0].shape[:2]:
                raise ValueError("%s: a %dx%d field among %dx%d ones" % (p, f.shape[1], f.shape[0], fwd[0].shape[1], fwd[0].shape[0]))
        if max(fwd[0].shape[:2]) > 8192:
            raise ValueError("%s: frames are at most 8192x8192" % a.forward[0])
    except cli.REFUSED as e:
        return cli.refuse("tracks", e)
    pipeline = cli.mod("pipeline")
    H, W = fwd[0].shape[:2]
    ts = pipeline.TrackSet(H, W, cap=a.cap, step=a.step, rel=a.rel, abs=a.abs)
    ts.seed()
    dropped = ts.counts()["seed"][3:4].clone()
    for f, b in zip(fwd, bwd):
        ts.advance(f, b)
        if a.reseed:
            ts.seed()
            dropped += ts.counts()["seed"][3:4]
    sparse = ts.flow(*span) if span is not None else None
    got = ts.read()
    np.savez(a.out, **got)
    if sparse is not None:
        flowio.write_field(a.flow[2], sparse.cpu().numpy())
    last = got["state"][-1]
    summary = dict(frames=T + 1, tracks=int(len(last)), dropped=int(dropped.cpu()[0]),
                   **{name: int((last == k).sum()) for k, name in enumerate(pipeline.TRACK_STATES) if k})
    lines = ["%d frames, %d tracks (%d cells dropped): %s" % (T + 1, summary["tracks"], summary["dropped"], ", ".join(
        "%d %s" % (summary[name], name) for name in pipeline.TRACK_STATES[1:]))]
    if span is not None:
        summary["flow_vectors"] = int((sparse[..., 2] > 0.5).sum().cpu())
        lines.append("flow %d -> %d: %d vectors" % (span[0], span[1], summary["flow_vectors"]))
    cli.report(a.json, summary, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
