#!/usr/bin/env python3
"""Drop-in for EpicFlow's interpolation binary, the last call of the reference's spremiZaEpic.py:28:

    python epicflow.py <img1> <img2> <edges.bin> <matches.txt> <out.flo> [-nw] [-nn N] [-k K]
                       [--prefilter] [--pref-nn N] [--pref-th T] [--saliency-th T] [--refine] [--refine-preset NAME]

img1 and img2 give H x W (they must have the same size; read as the first CLI reads them).  edges.bin is raw float32
(H,W), exactly H*W*4 bytes, read as edge strength.  Each line of matches.txt is "x1 y1 x2 y2": a seed at (rint(x1),
rint(y1)) with flow (x2 - x1, y2 - y1); matches outside the image are dropped and the later of two lines for one pixel
wins.  The dense flow (pipeline.epic_interpolate on the GPU: locally-weighted affine by default, Nadaraya-Watson with -nw;
-nn neighbours, default 100; kernel coefficient -k, default 0.8) goes to out.flo.  With --prefilter the matches first go
through pipeline.epic_prefilter with img1 (the match pre-filter: seeds in image regions of saliency below --saliency-th,
default 0.045, and seeds further than --pref-th px, default 5, from the estimate of their --pref-nn nearest seeds, default
25, are removed; 0 switches a stage off; any of the three options implies --prefilter; the values are EpicFlow's as recalled,
not checked against the binary; DESIGN.md "Match pre-filter").  With --refine the interpolated flow
first goes through pipeline.variational_refine with img1 and img2 (--refine-preset sintel|kitti|middlebury implies it and
selects that preset's values).  That step is this build's own definition of EpicFlow's variational refinement (DESIGN.md
"Variational refinement"; red-black SOR, not bit-matched to epicflow-static), which is why it has a long option of its own:
EpicFlow's single-dash refinement options (-iter -alpha -gamma -delta -sigma and the dataset presets) would promise that
binary's behaviour and stay refused here; variational.py takes those names for this build's step.  For the same reason
the binary's -prefnn stays refused: --prefilter is this build's definition of the pre-filter.  Malformed input and unsupported options exit with status 2.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

UNSUPPORTED = ("-prefnn", "-iter", "-alpha", "-gamma", "-delta", "-sigma", "-kitti", "-sintel", "-middlebury")


REFINE_PRESETS = ("sintel", "kitti", "middlebury")
# option -> (keyword of pipeline.epic_prefilter, type, largest value)
PREFILTER_OPTIONS = {"--pref-nn": ("pref_nn", int, 255), "--pref-th": ("pref_th", float, None),
                     "--saliency-th": ("saliency_th", float, None)}


class UsageError(ValueError):
    pass


def read_matches(path, H, W):
    """matches.txt -> (H,W,3) float32 [U,V,valid] sparse field."""
    rows = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            parts = line.split()
            if len(parts) != 4:
                raise UsageError("%s:%d: expected 'x1 y1 x2 y2', got %r" % (path, lineno, line.rstrip("\n")))
            try:
                rows.append([float(v) for v in parts])
            except ValueError:
                raise UsageError("%s:%d: not a number in %r" % (path, lineno, line.rstrip("\n")))
    sparse = np.zeros((H, W, 3), np.float32)
    if not rows:
        return sparse
    m = np.array(rows, np.float64)
    if not np.isfinite(m).all():
        raise UsageError("%s: a match is not finite" % path)
    x, y = np.rint(m[:, 0]), np.rint(m[:, 1])
    keep = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    m, x, y = m[keep], x[keep].astype(np.int64), y[keep].astype(np.int64)
    pix = y * W + x
    _, last = np.unique(pix[::-1], return_index=True)          # the later line for a pixel wins
    sel = len(pix) - 1 - last
    flat = sparse.reshape(-1, 3)
    flat[pix[sel], 0] = (m[sel, 2] - m[sel, 0]).astype(np.float32)
    flat[pix[sel], 1] = (m[sel, 3] - m[sel, 1]).astype(np.float32)
    flat[pix[sel], 2] = 1.0
    return sparse


def parse_args(argv):
    pos, nn, k, method = [], 100, 0.8, "LA"
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-nw":
            method = "NW"
        elif a in ("-nn", "-k"):
            if i + 1 >= len(argv):
                raise UsageError("%s needs a value" % a)
            try:
                if a == "-nn":
                    nn = int(argv[i + 1])
                else:
                    k = float(argv[i + 1])
            except ValueError:
                raise UsageError("%s: bad value %r" % (a, argv[i + 1]))
            i += 1
        elif a == "--refine":                                   # the long options are read by parse_refine
            pass
        elif a == "--refine-preset":
            if i + 1 >= len(argv) or argv[i + 1] not in REFINE_PRESETS:
                raise UsageError("--refine-preset needs one of %s" % ", ".join(REFINE_PRESETS))
            i += 1
        elif a == "--prefilter":                                # read by parse_prefilter
            pass
        elif a in PREFILTER_OPTIONS:
            name, kind, top = PREFILTER_OPTIONS[a]
            if i + 1 >= len(argv):
                raise UsageError("%s needs a value" % a)
            try:
                v = kind(argv[i + 1])
            except ValueError:
                raise UsageError("%s: bad value %r" % (a, argv[i + 1]))
            if not (np.isfinite(v) and v >= 0 and (top is None or v <= top)):
                raise UsageError("%s %s must be finite, >= 0%s" % (a, argv[i + 1], "" if top is None else " and <= %d" % top))
            i += 1
        elif a == "-prefnn":
            raise UsageError("-prefnn is not supported: it would promise epicflow-static's pre-filter; this build's own is "
                             "--prefilter [--pref-nn N] [--pref-th T] [--saliency-th T]")
        elif a in UNSUPPORTED:
            raise UsageError("%s is not supported: it would promise epicflow-static's variational refinement; this build's own "
                             "is --refine" % a)
        elif a.startswith("-") and len(a) > 1:
            raise UsageError("unknown option %s" % a)
        else:
            pos.append(a)
        i += 1
    if len(pos) != 5:
        raise UsageError("expected 5 positional arguments, got %d" % len(pos))
    if not 1 <= nn <= 256:
        raise UsageError("-nn %d outside [1,256]" % nn)
    if not (np.isfinite(k) and k > 0):
        raise UsageError("-k %g must be finite and > 0" % k)
    return pos, nn, k, method


def parse_refine(argv):
    """(refine, preset) of an argument list parse_args accepts: --refine, or --refine-preset NAME (which implies it; the
    last one given counts)."""
    preset = None
    for i, a in enumerate(argv):
        if a == "--refine-preset":
            preset = argv[i + 1]
    return "--refine" in argv or preset is not None, preset


def parse_prefilter(argv):
    """None, or the keyword arguments of pipeline.epic_prefilter, of an argument list parse_args accepts: --prefilter, or any
    of --pref-nn N, --pref-th T, --saliency-th T (which imply it; the last one given counts)."""
    kw = {}
    for i, a in enumerate(argv):
        if a in PREFILTER_OPTIONS:
            name, kind, _ = PREFILTER_OPTIONS[a]
            kw[name] = kind(argv[i + 1])
    return kw if kw or "--prefilter" in argv else None


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        (im1, im2, edges_bin, matches, out), nn, k, method = parse_args(argv)
        refine, refine_preset = parse_refine(argv)
        prefilter = parse_prefilter(argv)
        read_bgr = importlib.import_module(PKG + ".flowio").read_bgr
        img1, img2 = read_bgr(im1), read_bgr(im2)
        H, W = img1.shape[:2]
        if img2.shape[:2] != (H, W):
            raise UsageError("%s and %s differ in size" % (im1, im2))
        raw = open(edges_bin, "rb").read()
        if len(raw) != 4 * H * W:
            raise UsageError("%s holds %d bytes, not %d (float32 %dx%d)" % (edges_bin, len(raw), 4 * H * W, W, H))
        edges = np.frombuffer(raw, np.float32).reshape(H, W).copy()
        sparse = read_matches(matches, H, W)
    except (UsageError, OSError) as e:
        print("epicflow: %s" % e, file=sys.stderr)
        if isinstance(e, UsageError):
            print(__doc__, file=sys.stderr)
        return 2
    pipeline = importlib.import_module(PKG + ".pipeline")
    flowio = importlib.import_module(PKG + ".flowio")
    if prefilter is not None:
        sparse = pipeline.epic_prefilter(sparse, edges, img1, k=k, **prefilter)
    flow = pipeline.epic_interpolate(sparse, edges, nn=nn, k=k, method=method)
    if refine:
        flow = pipeline.variational_refine(img1, img2, flow, preset=refine_preset)
    flowio.write_flo(out, flow.cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
