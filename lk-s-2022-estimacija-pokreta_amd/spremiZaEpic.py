#!/usr/bin/env python3
"""Drop-in for the reference's third step (README.md:25-67, spremiZaEpic.py:1-28):

    python spremiZaEpic.py <img1> <img2> <forward flow .npy> <backward flow .npy> <con_tresh> canny|sed|pb [--natural-check] [--segments MIN T] [--margin FILE T] [--gpu-epic [--prefilter] [--refine]]

Same positional arguments, same files in the current directory: sparse_field.npy (postProcessing, through
dflow_fb_consistency on the GPU), parovi.txt (napravi_parove.parovi) and ivice.bin (edge.canny_ivice of img1, through
dflow_canny_edges).  Then ../discrete_flow/external/EpicFlow_v1.00/epicflow-static img1 img2 ivice.bin parovi.txt epic.flo
runs if that binary exists; otherwise one line says the inputs are ready and the binary is absent, and the exit status is 0.
'sed' edges need a model the reference does not ship: it exits with status 2 and says so.
'pb' (not in the reference) is the model-free substitute for 'sed': ivice.bin is 1 - e as raw float32, e the soft edge strength
of dflow_pb_edges on img1 (edge.pb_ivice, radius 5; DESIGN.md "Pb edge strength"): sed_ivice's file convention, so
epicflow-static reads it as it would read the sed file.  With --gpu-epic [--prefilter] [--refine] the pre-filter and the
interpolation receive e ITSELF, not 1 - e: edge strength is what the C-ABI defines d_edges to be.
With the opt-in seventh token --gpu-epic, epic.flo is written by this package's own interpolation (epicflow.py,
pipeline.epic_interpolate) from the device-side sparse field and edge map, with EpicFlow's defaults, and the binary is not
run.  ivice.bin is handed over as the reference writes it, (255 - edges) / 255 (DESIGN.md "EpicFlow interpolation").
With --prefilter directly after --gpu-epic, the matches first go through this package's match pre-filter with img1
(pipeline.epic_prefilter, its defaults; DESIGN.md "Match pre-filter"): the first thing epicflow-static does.  Only what the
interpolation reads is filtered: sparse_field.npy and parovi.txt are written unfiltered, as the reference writes them.
With --refine as the last token, after --gpu-epic [--prefilter], the interpolated flow goes through this package's variational
refinement with img1 and img2 (pipeline.variational_refine, its defaults; DESIGN.md "Variational refinement") before epic.flo
is written: the second thing epicflow-static does.
With --natural-check directly after the six positional tokens (before --gpu-epic, if that follows), sparse_field.npy, parovi.txt
and everything after them come from the forward/backward check in image coordinates (pipeline.flow_consistency, nearest lookup,
threshold con_tresh; DESIGN.md "Forward/backward check in image coordinates") in place of the reference's postProcessing, whose
lookup is transposed.
With the three tokens --segments MIN T directly after --natural-check if that is there, else after the six positional tokens, and
before --gpu-epic, the checked field goes through the small-segment filter (pipeline.segment_filter; DESIGN.md "Small-segment
filter"): segments of fewer than MIN pixels, grown over neighbours whose vectors differ by at most T in |dU| + |dV|, are removed.
This is part of postProcessing, where the reference has the call commented out (postprocessing.py:132): unlike --prefilter,
sparse_field.npy, parovi.txt and everything after them come from the filtered field.  Both values must be given: MIN an integer
>= 0, T finite and >= 0.
With the three tokens --margin FILE T directly after --segments MIN T if that is there, else where --segments would stand, and
before --gpu-epic, vectors whose forward margin is below T are dropped from the checked (and segment-filtered) field
(pipeline.flow_gate; DESIGN.md "Label confidence"): FILE is the (H,W) float32 .npy that `"python bcd.py" --confidence` wrote for the
forward pass.  Like --segments it comes before everything that reads sparse_field.npy.  T is a number, infinite perhaps, not NaN.
"""
import importlib
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))

EPICFLOW = "../discrete_flow/external/EpicFlow_v1.00/epicflow-static"     # spremiZaEpic.py:28


EDGE_KINDS = ("canny", "sed", "pb")


def parse(argv):
    """The command line -> (the six positional tokens, gpu_epic, prefilter, refine), or the exit status 2 after saying why."""
    tail = argv[6:]
    gpu_epic = tail in (["--gpu-epic"], ["--gpu-epic", "--prefilter"], ["--gpu-epic", "--refine"],
                        ["--gpu-epic", "--prefilter", "--refine"])
    prefilter, refine = gpu_epic and "--prefilter" in tail, gpu_epic and "--refine" in tail
    if len(argv) != 6 and not gpu_epic:
        print(__doc__, file=sys.stderr)
        return 2
    int(argv[4])                                                           # :14
    if argv[5] not in EDGE_KINDS:
        print("spremiZaEpic: edge kind must be 'canny' or 'sed', not %r" % argv[5], file=sys.stderr)
        return 2
    return argv[:6], gpu_epic, prefilter, refine


def take_natural(argv):
    """The optional seventh token --natural-check: (the command line without it, whether it was there)."""
    natural = argv[6:7] == ["--natural-check"]
    return (argv[:6] + argv[7:] if natural else argv), natural


def take_segments(argv):
    """The optional tokens --segments MIN T after the six positional ones (--natural-check already taken): (the command line
    without them, (MIN, T) or None), or the exit status 2 after saying why."""
    if argv[6:7] != ["--segments"]:
        return argv, None
    cli = importlib.import_module(PKG + ".cli")
    try:
        return argv[:6] + argv[9:], cli.segments(argv[7:9])
    except ValueError as e:
        return cli.refuse("spremiZaEpic", e)


def take_margin(argv):
    """The optional tokens --margin FILE T after the six positional ones (--natural-check and --segments already taken): (the
    command line without them, (FILE, T) or None), or the exit status 2 after saying why."""
    if argv[6:7] != ["--margin"]:
        return argv, None
    try:
        path, thresh = argv[7], float(argv[8])
        if np.isnan(thresh):
            raise ValueError
    except (IndexError, ValueError):
        print("spremiZaEpic: --margin needs FILE and T (a number, not NaN), got %r" % (argv[7:9],), file=sys.stderr)
        return 2
    return argv[:6] + argv[9:], (path, thresh)


def load_margin(path, shape):
    """The margin plane of --margin: an (H,W) float32 .npy of the flow's size, or None after saying why not."""
    try:
        m = np.load(path)
    except (OSError, ValueError) as e:
        print("spremiZaEpic: --margin %s: %s" % (path, e), file=sys.stderr)
        return None
    if m.dtype != np.float32 or m.shape != tuple(shape):
        print("spremiZaEpic: --margin %s holds %s %s, expected float32 %s" % (path, m.dtype, m.shape, tuple(shape)), file=sys.stderr)
        return None
    return m


def main(argv=None):
    argv, natural = take_natural(sys.argv[1:] if argv is None else list(argv))
    taken = take_segments(argv)
    if taken == 2:
        return 2
    argv, segments = taken
    taken = take_margin(argv)
    if taken == 2:
        return 2
    argv, margin = taken
    parsed = parse(argv)
    if parsed == 2:
        return 2
    (kitti1, kitti2, foward, backward, tresh, kind), gpu_epic, prefilter, refine = parsed
    con_tresh = int(tresh)                                                 # :14
    edge = importlib.import_module(PKG + ".edge")
    if kind == "sed":
        try:
            edge.sed_ivice(kitti1, "ivice.bin")
        except NotImplementedError as e:
            print("spremiZaEpic: %s" % e, file=sys.stderr)
            return 2
    fwd_host = np.load(foward).astype(np.float32)
    if margin is not None:
        margin_plane = load_margin(margin[0], fwd_host.shape[:2])
        if margin_plane is None:
            return 2
    import torch
    pipeline = importlib.import_module(PKG + ".pipeline")
    evaluate = importlib.import_module(PKG + ".evaluate")
    dev = torch.device("cuda", torch.cuda.current_device())
    fwd = torch.from_numpy(fwd_host).to(dev)
    bwd = torch.from_numpy(np.load(backward).astype(np.float32)).to(dev)
    sparse_dev = pipeline.flow_consistency(fwd, bwd, con_tresh) if natural else pipeline.fb_consistency(fwd, bwd, con_tresh)
    if segments is not None:
        sparse_dev = pipeline.segment_filter(sparse_dev, segments[1], segments[0])
    if margin is not None:
        sparse_dev = pipeline.flow_gate(sparse_dev, margin_plane, lo=margin[1])
    sparse = sparse_dev.cpu().numpy()                                      # postProcessing, :15
    np.save("sparse_field.npy", sparse)
    evaluate.parovi(sparse, "parovi.txt")                                  # :17
    if gpu_epic:
        if kind == "pb":
            ivice = edge.pb_strength_tensor(kitti1)                        # e itself for the GPU steps, 1 - e in the file
            edge.write_pb_ivice(ivice, "ivice.bin")
        else:
            ivice = edge.canny_ivice_tensor(kitti1)
            with open("ivice.bin", "wb") as f:
                f.write(ivice.cpu().numpy().tobytes())
        read_bgr = importlib.import_module(PKG + ".flowio").read_bgr
        if prefilter:
            sparse_dev = pipeline.epic_prefilter(sparse_dev, ivice, read_bgr(kitti1))
        flow = pipeline.epic_interpolate(sparse_dev, ivice)                # the step epicflow-static would take
        if refine:
            flow = pipeline.variational_refine(read_bgr(kitti1), read_bgr(kitti2), flow)
        importlib.import_module(PKG + ".flowio").write_flo("epic.flo", flow.cpu().numpy())
        print("spremiZaEpic: sparse_field.npy, parovi.txt, ivice.bin and epic.flo written (%sGPU interpolation%s)"
              % ("match pre-filter + " if prefilter else "", " + variational refinement" if refine else ""))
        return 0
    if kind == "pb":
        edge.pb_ivice(kitti1, "ivice.bin")
    else:
        edge.canny_ivice(kitti1, "ivice.bin")                              # :19-23
    if not os.path.exists(EPICFLOW):
        print("spremiZaEpic: sparse_field.npy, parovi.txt and ivice.bin are ready; %s is absent, EpicFlow not run" % EPICFLOW)
        return 0
    return subprocess.run([EPICFLOW, kitti1, kitti2, "ivice.bin", "parovi.txt", "epic.flo"]).returncode


if __name__ == "__main__":
    sys.exit(main())
