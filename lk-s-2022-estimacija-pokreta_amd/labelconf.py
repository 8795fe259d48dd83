"""The command-line side of the label confidence (pipeline.DiscreteFlow.confidence, DESIGN.md "Label confidence"): the options
"python bcd.py" and run_batch.py share, checked before any device is touched.  No torch here."""
import math

MODES = ("local", "data")


def add_cli_options(ap, with_threshold):
    """--confidence (with_threshold: --confidence T), --conf-mode and --conf-sep on an argparse parser."""
    if with_threshold:
        ap.add_argument("--confidence", default=None, metavar="T",
                        help="take every pass's label margin and drop sparse vectors whose forward margin is below T")
    else:
        ap.add_argument("--confidence", action="store_true", help="also write the margin plane of the final labelling (float32 .npy)")
    ap.add_argument("--conf-mode", default=None, metavar="M", help="with --confidence: local (default) or data")
    ap.add_argument("--conf-sep", default=None, metavar="S", help="with --confidence: labels within S px (L1) of the chosen one do not compete (default 1)")


def threshold(token, error, what="--confidence"):
    """T of --confidence T or --margin FILE T: a float, infinite perhaps, not NaN; error(message) otherwise."""
    try:
        t = float(token)
        if math.isnan(t):
            raise ValueError
    except (TypeError, ValueError):
        error("%s needs T (a number, not NaN), got %r" % (what, token))
    return t


def from_args(ap, a):
    """(mode, min_sep) of the parsed options, the defaults ("local", 1) filled in; ap.error (exit status 2) for an unknown mode, a
    separation outside 0..1024, or either given without --confidence."""
    on = a.confidence is not None and a.confidence is not False
    if not on and (a.conf_mode is not None or a.conf_sep is not None):
        ap.error("--conf-mode and --conf-sep need --confidence")
    mode = "local" if a.conf_mode is None else a.conf_mode
    if mode not in MODES:
        ap.error("--conf-mode needs M (local or data), got %r" % (a.conf_mode,))
    try:
        sep = 1 if a.conf_sep is None else int(a.conf_sep)
        if not 0 <= sep <= 1024:
            raise ValueError
    except ValueError:
        ap.error("--conf-sep needs S (an integer in 0..1024), got %r" % (a.conf_sep,))
    return mode, sep
