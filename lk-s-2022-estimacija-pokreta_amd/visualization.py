#!/usr/bin/env python3
"""Drop-in for the reference's evaluation step (README.md of the reference, visualization.py:128-196):

    python visualization.py <ground truth flow> <test flow> [<error image>]

Same positional arguments, same files in the current directory.  Both flows are read with evaluate.ucitajFlow ('.png' KITTI
ground truth, '.npy' the hot path's fields, '.flo' Middlebury), the comparison runs on the GPU (dflow_flow_eval through
pipeline.flow_eval, DESIGN.md "Flow evaluation"), and one line each is appended to srednja_greska.txt (mean end-point error
over the pixels valid in both fields) and procenat_outliera.txt (percentage of them with an error above 3 px), as
errorImage does (:149-152).
The outlier line is str(n_out_abs * 100 / n) on Python ints: string-equal to the reference's.  The mean line is
str(np.float32(sum_err / n)): the reference averages its float32 errors in float32 (numpy's pairwise sum), this build sums
them in double and rounds once, so the two lines may differ in the last digits.  With no pixel valid in both fields both
lines are 'nan' and the exit status is 0 (the reference divides by zero there).  Pixels whose error is not finite are left
out of both numbers, and a warning on stderr says how many.
With a third argument the colour error picture (jet over min(err, 3) / 3, black where nothing is compared; :133-143,:156) is
written there with flowio.write_picture: '.png' and '.ppm' (a binary P6 file) without any imaging library; any other
extension goes through PIL if it can be imported, and otherwise the command exits with status 2 and names those two.
The reference's trailing cv2.waitKey / imshow window is not reproduced.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

ALWAYS = (".png", ".ppm")       # picture formats written without an imaging library


def parse(argv):
    """The command line -> (gt path, test path, error image path or None), or the exit status 2 after saying why."""
    if len(argv) not in (2, 3):
        print(__doc__, file=sys.stderr)
        return 2
    errimg = argv[2] if len(argv) == 3 else None                          # :189-192
    if errimg is not None and os.path.splitext(errimg)[1].lower() not in ALWAYS:
        try:
            import PIL  # noqa: F401
        except ImportError:
            print("visualization: cannot write %r without PIL; '.png' and '.ppm' always work" % errimg, file=sys.stderr)
            return 2
    return argv[0], argv[1], errimg


def main(argv=None):
    parsed = parse(sys.argv[1:] if argv is None else list(argv))
    if parsed == 2:
        return 2
    gt_path, test_path, errimg = parsed
    evaluate = importlib.import_module(PKG + ".evaluate")
    pipeline = importlib.import_module(PKG + ".pipeline")
    gt = evaluate.ucitajFlow(gt_path)                                     # :173-176
    test = evaluate.ucitajFlow(test_path)                                 # :183-185
    if gt.shape != test.shape:
        print("visualization: ground truth is %dx%d, the test flow %dx%d" % (gt.shape[1], gt.shape[0], test.shape[1], test.shape[0]),
              file=sys.stderr)
        return 2
    out = pipeline.flow_eval(test, gt, 3.0, image=errimg is not None)     # ABS_THRESH, :129
    st = pipeline.eval_stats(out[0] if errimg is not None else out)
    n = st["n"]
    if st["n_nonfinite"]:
        print("visualization: %d compared pixels have an error that is not finite; they are left out" % st["n_nonfinite"],
              file=sys.stderr)
    with open("srednja_greska.txt", "a+", encoding="utf-8") as f:         # :148-150
        f.write((str(np.float32(st["sum_err"] / n)) if n else "nan") + "\n")
    with open("procenat_outliera.txt", "a+", encoding="utf-8") as f:      # :151-152
        f.write((str(st["n_out_abs"] * 100 / n) if n else "nan") + "\n")
    if errimg is not None:
        importlib.import_module(PKG + ".flowio").write_picture(errimg, out[1].cpu().numpy())    # :155-156
    return 0


if __name__ == "__main__":
    sys.exit(main())
