#!/usr/bin/env python3
"""Variational refinement of a dense flow, the second half of what EpicFlow's binary does after its interpolation:

    python variational.py <img1> <img2> <in.flo> <out.flo> [-iter N] [-alpha A] [-gamma G] [-delta D] [-sigma S]
                          [-sintel | -kitti | -middlebury]

img1, img2 and in.flo must have the same size.  The flow is refined by pipeline.variational_refine on the GPU
(dflow_var_refine: DESIGN.md "Variational refinement", this build's own definition of that step, not bit-matched to
epicflow-static) and written to out.flo.  The options carry EpicFlow's names: -iter outer iterations (5), -alpha
smoothness weight (1.0), -gamma gradient-constancy weight (0.71), -delta colour-constancy weight (0.0), -sigma
presmoothing (1.0); a preset sets the variational values EpicFlow documents for that dataset, and options given with it
override it wherever they stand.  The defaults and presets are recalled from EpicFlow's documentation and have not been
checked against its binary.  Malformed input and unknown options exit with status 2.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

OPTIONS = {"-iter": ("niter_outer", int), "-alpha": ("alpha", float), "-gamma": ("gamma", float),
           "-delta": ("delta", float), "-sigma": ("sigma", float)}
PRESETS = ("sintel", "kitti", "middlebury")


class UsageError(ValueError):
    pass


def check_params(params):
    """The bounds of dflow_var_refine on the options a command line can set (include/dflow.h)."""
    with np.errstate(over="ignore"):
        f32 = {k: float(np.float32(v)) for k, v in params.items() if isinstance(v, float)}     # what the struct carries
    for name in ("alpha", "gamma", "delta"):
        v = f32.get(name, 0.0)
        if not (np.isfinite(v) and v >= 0):
            raise UsageError("-%s %g must be finite (in float32) and >= 0" % (name, params[name]))
    s = f32.get("sigma", 1.0)
    if not (np.isfinite(s) and 0 <= s <= 5):
        raise UsageError("-sigma %g outside [0,5]" % params["sigma"])
    if not 0 <= params.get("niter_outer", 5) <= 1000:
        raise UsageError("-iter %d outside [0,1000]" % params["niter_outer"])


def parse_args(argv):
    """-> ([img1, img2, in.flo, out.flo], preset or None, {field: value})."""
    pos, preset, params = [], None, {}
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in OPTIONS:
            field, kind = OPTIONS[a]
            if i + 1 >= len(argv):
                raise UsageError("%s needs a value" % a)
            try:
                params[field] = kind(argv[i + 1])
            except ValueError:
                raise UsageError("%s: bad value %r" % (a, argv[i + 1]))
            i += 1
        elif a[1:] in PRESETS and a.startswith("-"):
            if preset is not None and preset != a[1:]:
                raise UsageError("-%s and %s given together" % (preset, a))
            preset = a[1:]
        elif a.startswith("-") and len(a) > 1:
            raise UsageError("unknown option %s" % a)
        else:
            pos.append(a)
        i += 1
    if len(pos) != 4:
        raise UsageError("expected 4 positional arguments, got %d" % len(pos))
    check_params(params)
    return pos, preset, params


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        (im1, im2, flo_in, flo_out), preset, params = parse_args(argv)
        read_bgr = importlib.import_module(PKG + ".flowio").read_bgr
        flowio = importlib.import_module(PKG + ".flowio")
        img1, img2 = read_bgr(im1), read_bgr(im2)
        try:
            uv = flowio.read_flo(flo_in)
        except ValueError as e:
            raise UsageError(str(e))
        if img1.shape != img2.shape or uv.shape[:2] != img1.shape[:2]:
            raise UsageError("%s %s, %s %s and %s %s differ in size" % (im1, img1.shape[:2], im2, img2.shape[:2], flo_in, uv.shape[:2]))
    except (UsageError, OSError) as e:
        print("variational: %s" % e, file=sys.stderr)
        if isinstance(e, UsageError):
            print(__doc__, file=sys.stderr)
        return 2
    pipeline = importlib.import_module(PKG + ".pipeline")
    try:
        flow = pipeline.variational_refine(img1, img2, np.ascontiguousarray(uv[..., ::-1]), preset=preset, **params)
    except (ValueError, importlib.import_module(PKG + "._lib").DflowError) as e:      # a refusal by the library
        print("variational: %s" % e, file=sys.stderr)
        return 2
    flowio.write_flo(flo_out, flow.cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
