"""What a command-line tool does around its one call into pipeline (DESIGN.md "Command-line tools"): the sibling import, the
parser, the value checks, the refusal and the report.  The standard library only, so that a refusal never imports torch.  The
file formats are flowio's."""
import argparse
import importlib
import json
import math
import os
import sys

REFUSED = (ValueError, OSError)             # what reading and comparing the inputs raises: refuse(tool, e) is its end
POSITIVE = "must be finite and > 0"         # real()'s words, for a message about more than one value


def mod(name):
    """The sibling module `name` of this package."""
    return importlib.import_module(__package__ + "." + name)


def parser(doc):
    """The parser of a tool whose module docstring is its help text."""
    return argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)


# ------------------------------------------------------------------------------------------------ the value checks
# The token forms take the text of an option (or its parsed value) and raise ValueError, whose message completes "<option> ...".
def integer(token, lo, hi):
    """token as an integer in [lo, hi]."""
    v = int(token)
    if not lo <= v <= hi:
        raise ValueError("must lie in [%d, %d]" % (lo, hi))
    return v


def real(token, positive):
    """token as a finite float: > 0 if positive, >= 0 if positive is False, of either sign if it is None."""
    v = float(token)
    if not (math.isfinite(v) and (positive is None or (v > 0 if positive else v >= 0))):
        raise ValueError(POSITIVE if positive else "must be finite" + ("" if positive is None else " and >= 0"))
    return v


def segments(tokens):
    """--segments MIN T as run_batch.py and spremiZaEpic.py take it -> (MIN, T)."""
    try:
        return integer(tokens[0], 0, 2 ** 31 - 1), real(tokens[1], False)
    except (IndexError, ValueError):
        raise ValueError("--segments needs MIN (an integer >= 0) and T (finite, >= 0), got %r" % (tokens,)) from None


# The parser forms take the parser, the option's name and its value, pass None (the option was not given) and exit through
# ap.error: "<tool>.py: error: <option> must ...", status 2.
def _check(ap, name, value, read, *args):
    try:
        return None if value is None else read(value, *args)
    except ValueError as e:
        ap.error("%s %s" % (name, e))


def in_range(ap, name, value, lo, hi):
    """An integer in [lo, hi]."""
    return _check(ap, name, value, integer, lo, hi)


def positive(ap, name, value):
    """A float that is finite and > 0."""
    return _check(ap, name, value, real, True)


def non_negative(ap, name, value):
    """A float that is finite and >= 0."""
    return _check(ap, name, value, real, False)


def between(ap, name, value, lo, hi):
    """A float strictly between lo and hi."""
    if value is not None and not lo < value < hi:
        ap.error("%s must lie in (%g, %g)" % (name, lo, hi))


def extension(ap, name, path, *exts):
    """A path whose extension, in either letter case, is one of exts."""
    if path is not None and os.path.splitext(path)[1].lower() not in exts:
        ap.error("%s must be a %s file" % (name, " or ".join(exts)))


# ------------------------------------------------------------------------------------------------ the refusal and the report
def refuse(tool, message):
    """"<tool>: <message>" on stderr; returns the exit status 2."""
    print("%s: %s" % (tool, message), file=sys.stderr)
    return 2


def report(as_json, obj, lines):
    """The end of a tool: obj as one JSON object, or its text lines."""
    print(json.dumps(obj) if as_json else "\n".join(lines))


def inliers(inliers, scored, found):
    """(the inlier fraction, the line that reports it) of a random-sample fit; found: a model was."""
    fraction = inliers / scored if scored else 0.0
    return fraction, "inliers: %d of %d scored vectors (%.2f%%)%s" % (inliers, scored, 100.0 * fraction,
                                                                      "" if found else "; no model was found")
