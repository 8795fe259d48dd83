#!/usr/bin/env python3
"""Batch driver for BASELINE configs 3 and 4: forward + backward pass of every pair, sharded over the GPUs of one node
(pass p -> rank p mod world, README.md:40 of the reference), RCCL gather of the flow fields on rank 0, then the
forward/backward consistency check (postprocessing.py:123-135) per pair on rank 0.

    python run_batch.py --pairs 8 --bcd-times 4 [--size 436x1024] [--thresh 10] [--out DIR]
    python -m torch.distributed.run --nproc-per-node 8 run_batch.py --pairs 8 ...

Inputs are synthetic pairs (synth.make_pair, seed 1000*pair); outputs per pair in DIR: the reference's flow .npy names
for both directions, a .flo of the forward flow, sparse_field_<pair>.npy and parovi_<pair>.txt; with --edges also
ivice_<pair>.bin, the Canny edge map of the pair's first image (edge.py canny_ivice: the third EpicFlow input); with
--epic also epic_<pair>.flo, the dense flow interpolated from the pair's sparse field and that edge map
(pipeline.epic_interpolate, EpicFlow's defaults); with --epic-refine (implies --epic) that flow goes through the variational
refinement with the pair's two images (pipeline.variational_refine, its defaults) before epic_<pair>.flo is written; with
--prefilter (implies --epic) the sparse field first goes through the match pre-filter with the pair's first image
(pipeline.epic_prefilter, its defaults) before it is interpolated; sparse_field_<pair>.npy and parovi_<pair>.txt stay unfiltered.
--edge-kind pb takes the edges of all of these from the soft detector instead of Canny (pipeline.pb_edges, radius 5; DESIGN.md
"Pb edge strength"), with spremiZaEpic.py's conventions: ivice_<pair>.bin holds 1 - e, the pre-filter and the interpolation
receive the strength e itself.  Without it (canny, the default) nothing changes.
--eval compares every pair's fields with the true flow synth.make_pair returns (pipeline.flow_eval, DESIGN.md "Flow
evaluation"): the forward flow ("fwd"), the sparse field ("sparse": the pixels that survive the consistency check) and, with
--epic, the final dense flow ("epic"), each on the device where it lies.  One line per pair is printed, and eval.json in DIR
holds the per-pair rows and, per kind, the totals accumulated on the device.  Without it output and files are unchanged.
--pictures writes flowcolor_<pair>.png, the colour-wheel picture of the forward flow (pipeline.flow_color, DESIGN.md "Flow
pictures and the warp check"), and with --epic flowcolor_epic_<pair>.png of the final dense flow.  --photo warps each pair's
second image back onto the first by the forward flow ("fwd") and, with --epic, by the final dense flow ("epic")
(pipeline.warp_eval, its default thresholds): no ground truth is involved.  One line per pair is printed, and photo.json in
DIR holds the per-pair rows and, per kind, the totals accumulated on the device.  Without them output and files are unchanged.
--bcd-stats records, for every pass, the labels changed, the data and smoothness sums and the image energy E after every BCD
sweep (pipeline.ceoBCD_batch with a stop rule, DESIGN.md "BCD statistics and the stop rule") and writes them to bcd_stats.json
in DIR.  --stop-changed F ends a pass after the sweep that changed at most the fraction F of its labels, --stop-energy R
after the sweep that lowered E by at most the fraction R; --bcd-times stays the upper bound and names the flow files.  Each
of the three costs one read-back of 48 bytes per pass and sweep; without them the launches are unchanged.
--pyramid L runs every pass coarse to fine (pipeline.PyramidFlow, DESIGN.md "Coarse to fine"): inside a group the levels run
from the coarsest to the finest for all its passes, each level with its own front ends side by side and its sweeps as batched
launches, and a level's flow is upsampled into the prior of the next.  --coarse-bcd-times N sets the sweeps of the coarse
levels (default: --bcd-times), --fine-window W the kNN window of the full-size level.  The files are those of a run without
it (--bcd-stats describes the full-size level); the headers of eval.json, photo.json and bcd_stats.json gain "pyramid": L.
Without it the launches are unchanged.
--check natural replaces the consistency check of every pair by the one in image coordinates (pipeline.flow_consistency, nearest
lookup, DESIGN.md "Forward/backward check in image coordinates": the forward vector at p against the backward vector at
p + f(p)); --thresh is its threshold.  The printed "survives" line, sparse_field_<pair>.npy, parovi_<pair>.txt, --prefilter,
--epic and --eval's "sparse" row follow the choice, and the header of eval.json gains "check": "natural".  The default,
reference, is the reference's check with its transposed lookup (pipeline.fb_consistency): nothing changes.
--segments MIN T sends every pair's checked field through the small-segment filter (pipeline.segment_filter, DESIGN.md
"Small-segment filter"): segments of fewer than MIN pixels, grown over neighbours whose vectors differ by at most T in
|dU| + |dV|, are removed, after the check and before everything that reads the sparse field: the "survives" line,
sparse_field_<pair>.npy, parovi_<pair>.txt, --prefilter, --epic and --eval's "sparse" row.  One line per pair gives the four
counts, and the header of eval.json gains "segments": [MIN, T].  Both values must be given.  Without it nothing is launched
that was not launched before.
--midframe writes mid_<pair>.png, the frame at t = 0.5 between each pair's two images, from the pair's forward and backward flows
(pipeline.frame_interp, DESIGN.md "Frame interpolation"; --mid-fill-rounds K and --mid-occl-thresh D set its fill rounds and
occlusion threshold, default 8 and 30).  One line per pair gives the eight counts and the PSNR of that frame and of the plain
blend (I1 + I2) / 2 against the true middle frame (synth.make_mid, over the pixels whose source lies inside the first image), and
midframe.json in DIR holds the per-pair rows.  Without it nothing is launched that was not launched before.
--wmedian R writes wmedian_<pair>.flo, each pair's forward flow through the weighted median filter of radius R guided by the
pair's first image (pipeline.flow_wmedian with its default sigmas, DESIGN.md "Weighted median filter"); with --eval the pair's
row and the totals gain the kind "filtered".  --wmedian-reject R T sends the sparse field through the same filter in reject
mode, guided: a vector that differs from the weighted median of its window by more than T in |dU| + |dV| is removed and every
other vector stays bit for bit, after the check and --segments and before everything that reads the sparse field (as
--segments).  One line per pair gives the four counts; the header of eval.json gains "wmedian": R and "wmedian_reject": [R, T].
Without them nothing is launched that was not launched before.
--motion MODEL (affine or homography) fits the dominant motion of every pair's forward flow (pipeline.motion_fit with its
defaults, DESIGN.md "Global-motion fit"; --motion-thresh T is its inlier threshold in pixels, default 1) and writes
residual_<pair>.flo, the forward flow minus the model's, and motion.json in DIR with the per-pair rows {pair, matrix, scored,
inliers}.  One line per pair gives the inlier share.  Without it nothing is launched that was not launched before.
--epipolar T fits the epipolar geometry of every pair's checked sparse field (pipeline.epipolar_fit with its defaults and the
Sampson threshold T pixels, DESIGN.md "Epipolar-geometry fit"), after the check, --segments, --wmedian-reject and --confidence
and before --prefilter / --epic, and writes epipolar.json in DIR with the per-pair rows {pair, model, F, e1, e2, foe and the
counts}; with --motion homography a row also holds that fit's counts.  --epipolar-gate drops the vectors that disagree from the
sparse field, every other vector bit for bit.  One line per pair gives the inlier share.  Without it nothing is launched that
was not launched before.
--pose FOCAL, with --epipolar, takes each pair's fit apart into the camera's motion (pipeline.two_view with the focal length FOCAL
pixels, the principal point at the frame's centre and the fit's inliers as the voters, DESIGN.md "Two-view reconstruction"): a
"pose" entry {R, t, angle_deg, axis, singular, candidate and the counts} in the pair's row of epipolar.json and depth_<pair>.npy,
the (H,W) float32 depth in units of the baseline.  One line per pair.  Without it the JSON and the launches are what they were.
--confidence T takes every pass's label margin after its sweeps (DiscreteFlow.confidence, DESIGN.md "Label confidence"; --conf-mode
local|data and --conf-sep S as in "python bcd.py", default local and 1); the margin travels to rank 0 as a third channel of the
pass's flow.  There every pair's checked sparse field is gated with the forward margin (pipeline.flow_gate, margin >= T), after
the check, --segments and --wmedian-reject and before everything that reads the sparse field; one line per pair gives the counts,
and margin_<pair>.npy holds the forward margin.  --eval gains the kind "confident", the forward flow gated by its margin alone,
with no backward pass involved, and the header of eval.json "confidence": [T, mode, S].  Without it nothing is launched that was
not launched before, and the flows travel as (H,W,2).
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))
cli = importlib.import_module(PKG + ".cli")
mod = cli.mod


def parser():
    ap = cli.parser(__doc__)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--bcd-times", type=int, default=4)
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--thresh", type=float, default=10.0)     # README.md:65 of the reference
    ap.add_argument("--check", choices=("reference", "natural"), default="reference",
                    help="the forward/backward check: the reference's (transposed lookup), or the one in image coordinates")
    ap.add_argument("--segments", nargs=2, default=None, metavar=("MIN", "T"),
                    help="after the check: remove segments of fewer than MIN pixels, joined where |dU| + |dV| <= T")
    ap.add_argument("--out", default=".")
    ap.add_argument("--group", type=int, default=4, help="passes of a rank whose BCD sweeps share their launches")
    ap.add_argument("--cell", default=None, help="cell size HxW (default: the geometry's usual cells)")
    ap.add_argument("--fp16-descriptors", action="store_true", help="DAISY values rounded to binary16 (BASELINE configs[4])")
    ap.add_argument("--time", action="store_true", help="run the passes twice and report the wall time of the second run")
    ap.add_argument("--edges", action="store_true", help="also write ivice_NN.bin (Canny edge map of each pair's first image)")
    ap.add_argument("--epic", action="store_true", help="also write epic_NN.flo (edge-aware interpolation of each pair's sparse field)")
    ap.add_argument("--epic-refine", action="store_true", help="--epic, and epic_NN.flo is the variationally refined flow")
    ap.add_argument("--prefilter", action="store_true", help="--epic, and the sparse field goes through the match pre-filter first")
    ap.add_argument("--edge-kind", choices=("canny", "pb"), default="canny",
                    help="edge source of --edges, --epic, --epic-refine and --prefilter: Canny, or the soft Pb-style strength")
    ap.add_argument("--eval", action="store_true",
                    help="compare each pair's forward, sparse and (with --epic) final flow with the true flow; writes eval.json")
    ap.add_argument("--pictures", action="store_true",
                    help="also write flowcolor_NN.png (colour-wheel picture of the forward flow) and, with --epic, flowcolor_epic_NN.png")
    ap.add_argument("--photo", action="store_true",
                    help="warp each pair's second image by the forward and (with --epic) final flow; prints the photometric error, writes photo.json")
    ap.add_argument("--midframe", action="store_true",
                    help="also write mid_NN.png, the frame at t = 0.5 from the pair's two flows; prints its PSNR, writes midframe.json")
    ap.add_argument("--mid-fill-rounds", type=int, default=None, metavar="K", help="with --midframe: fill rounds, 0..64 (default 8)")
    ap.add_argument("--mid-occl-thresh", type=float, default=None, metavar="D", help="with --midframe: occlusion threshold (default 30)")
    ap.add_argument("--wmedian", default=None, metavar="R",
                    help="also write wmedian_NN.flo, the forward flow through the guided weighted median filter of radius R (1..8)")
    ap.add_argument("--wmedian-reject", nargs=2, default=None, metavar=("R", "T"),
                    help="after the check and --segments: remove sparse vectors further than T from their window's weighted median (radius R)")
    ap.add_argument("--motion", default=None, metavar="MODEL",
                    help="also fit the dominant motion (affine or homography) of each forward flow; writes motion.json and residual_NN.flo")
    ap.add_argument("--motion-thresh", default=None, metavar="T", help="with --motion: the inlier threshold in pixels (default 1)")
    ap.add_argument("--epipolar", default=None, metavar="T",
                    help="also fit the epipolar geometry of each pair's checked sparse field (Sampson threshold T pixels); writes epipolar.json")
    ap.add_argument("--epipolar-gate", action="store_true", help="with --epipolar: drop the vectors that disagree from the sparse field")
    ap.add_argument("--pose", default=None, metavar="FOCAL",
                    help="with --epipolar: the camera's motion and the depths under the focal length FOCAL pixels; writes depth_NN.npy")
    mod("bcdstats").add_cli_options(ap, "--bcd-stats")
    mod("labelconf").add_cli_options(ap, with_threshold=True)
    ap.add_argument("--pyramid", type=int, default=1, metavar="L", help="coarse to fine with L levels (1: the plain pass)")
    ap.add_argument("--coarse-bcd-times", type=int, default=None, metavar="N", help="with --pyramid: sweeps of the coarse levels (default: --bcd-times)")
    ap.add_argument("--fine-window", type=int, default=None, metavar="W", help="with --pyramid: kNN window (0..2) of the full-size level")
    return ap


EVAL_ROW = ("n", "n_out_abs", "n_out_kitti", "n_nonfinite", "n_gt_valid", "n_test_valid", "sum_err", "max_err", "mean_epe",
            "outliers_pct", "kitti_fl_pct")
PHOTO_ROW = ("n", "n_outside", "n_unknown", "n_above", "sum_err", "max_err", "mean_err", "above_pct")


def checked(needs, got, read):
    """read()'s value; a ValueError in it exits with status 2 and "<needs>, got <got>"."""
    try:
        return read()
    except ValueError:
        parser().error("%s, got %r" % (needs, got))


def segments_arg(tokens):
    """--segments MIN T -> (MIN, T); exits with status 2 unless MIN is an integer >= 0 and T finite and >= 0."""
    try:
        return cli.segments(tokens)
    except ValueError as e:
        parser().error(str(e))


def wmedian_arg(token):
    """--wmedian R -> R; exits with status 2 unless R is an integer in 1..8."""
    return checked("--wmedian needs R (an integer in 1..8)", token, lambda: cli.integer(token, 1, 8))


def wmedian_reject_arg(tokens):
    """--wmedian-reject R T -> (R, T); exits with status 2 unless R is an integer in 1..8 and T finite and >= 0."""
    return checked("--wmedian-reject needs R (an integer in 1..8) and T (finite, >= 0)", tokens,
                 lambda: (cli.integer(tokens[0], 1, 8), cli.real(tokens[1], False)))


def motion_args(a):
    """--motion MODEL and --motion-thresh T -> (MODEL or None, T); exits with status 2 for an unknown model, a threshold that is
    not finite and > 0, or a threshold without --motion."""
    if a.motion is None and a.motion_thresh is not None:
        parser().error("--motion-thresh needs --motion")
    if a.motion is not None and a.motion not in ("affine", "homography"):
        parser().error("--motion needs MODEL (affine or homography), got %r" % (a.motion,))
    if a.motion_thresh is None:
        return a.motion, 1.0
    return a.motion, checked("--motion-thresh needs T (finite, > 0)", a.motion_thresh, lambda: cli.real(a.motion_thresh, True))


def epipolar_arg(a):
    """--epipolar T -> T or None; exits with status 2 for a threshold that is not finite and > 0, or --epipolar-gate or --pose
    without it."""
    if a.epipolar is None:
        if a.epipolar_gate:
            parser().error("--epipolar-gate needs --epipolar")
        if getattr(a, "pose", None) is not None:
            parser().error("--pose needs --epipolar")
        return None
    return checked("--epipolar needs T (finite, > 0)", a.epipolar, lambda: cli.real(a.epipolar, True))


def pose_arg(a):
    """--pose FOCAL -> FOCAL or None; exits with status 2 for a focal length that is not finite and > 0."""
    if a.pose is None:
        return None
    return checked("--pose needs FOCAL (finite, > 0)", a.pose, lambda: cli.real(a.pose, True))


def pose_pair(s, pair, sparse_dev, model, cls):
    """--pose: the camera motion of one pair from its fit (model and classes still on the device), depth_<pair>.npy, the printed
    line; returns the "pose" entry of the pair's row."""
    a, pipeline = s.a, mod("pipeline")
    pose, depth, counts = pipeline.two_view(sparse_dev, model, focal=a.pose, part=cls, depth=True, counts=True)
    counts = dict(zip(pipeline.TWO_VIEW_COUNTS[:7], counts.cpu().tolist()))
    info = pipeline.two_view_pose(pose.cpu().numpy())
    np.save(os.path.join(a.out, "depth_%02d.npy" % pair), depth.cpu().numpy())
    if info["candidate"] < 0:
        print("pair %d: pose: none (%d voters)" % (pair, counts["voters"]))
    else:
        print("pair %d: pose: rotation %.4f deg, t (%s), %d of %d voters in front of both cameras"
              % (pair, info["angle_deg"], " ".join("%.4f" % v for v in info["t"]), counts["votes"], counts["voters"]))
    return dict(focal=a.pose, R=info["R"].tolist(), t=info["t"].tolist(), angle_deg=info["angle_deg"],
                axis=None if info["axis"] is None else info["axis"].tolist(), singular=info["singular"].tolist(), **counts)


def epipolar_pair(s, pair, sparse_dev):
    """--epipolar: the fit of one pair's checked sparse field, its row of epipolar.json and its printed line; returns the field,
    without the vectors that disagree under --epipolar-gate (the others keep their bits)."""
    import torch
    a, pipeline = s.a, mod("pipeline")
    model, cls, counts = pipeline.epipolar_fit(sparse_dev, thresh=a.epipolar, classes=True, counts=True)
    posed = pose_pair(s, pair, sparse_dev, model, cls) if a.pose is not None else None
    counts = dict(zip(pipeline.EPIPOLAR_FIT_COUNTS[:7], counts.cpu().tolist()))
    model = model.cpu().numpy()
    geo = pipeline.epipolar_geometry(model, s.H, s.W)
    s.epipolar_rows.append(dict(pair=pair, model=model.tolist(), F=geo["F"].tolist(), e1=geo["e1"].tolist(), e2=geo["e2"].tolist(),
                                foe=geo["foe"], **counts))
    if posed is not None:
        s.epipolar_rows[-1]["pose"] = posed
    print("pair %d: epipolar geometry: %d of %d checked vectors within %g px (%.2f%%)%s"
          % (pair, counts["inliers"], counts["scored"], a.epipolar, 100.0 * counts["inliers"] / max(counts["scored"], 1),
             "" if counts["best_slot"] >= 0 else "; no model was found"))
    if a.epipolar_gate:
        sparse_dev = torch.where((cls == 2)[..., None], torch.zeros_like(sparse_dev), sparse_dev)
    return sparse_dev


def midframe_args(a):
    """--mid-fill-rounds and --mid-occl-thresh with their defaults; exits with status 2 if one is given without --midframe or lies
    outside its range."""
    if not a.midframe and (a.mid_fill_rounds is not None or a.mid_occl_thresh is not None):
        parser().error("--mid-fill-rounds and --mid-occl-thresh need --midframe")
    rounds = 8 if a.mid_fill_rounds is None else a.mid_fill_rounds
    occl = 30.0 if a.mid_occl_thresh is None else a.mid_occl_thresh
    for name, value, read in (("--mid-fill-rounds", rounds, lambda: cli.integer(rounds, 0, 64)),
                              ("--mid-occl-thresh", occl, lambda: cli.real(occl, False))):
        try:
            read()
        except ValueError as e:
            parser().error("%s %s, got %r" % (name, e, value))
    return rounds, occl


def psnr(a, b, mask):
    """10 log10(255^2 / MSE) of two uint8 pictures over the pixels of mask (all channels); None when nothing is compared, inf
    when they are equal there."""
    d = a[mask].astype(np.float64) - b[mask].astype(np.float64)
    if d.size == 0:
        return None
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def midframe_pair(s, pair, fwd, bwd, rows):
    """--midframe of one pair: mid_<pair>.png, its printed line and its row."""
    pipeline, synth, flowio = mod("pipeline"), mod("synth"), mod("flowio")
    seed = synth.pair_seed(pair, 0)
    if pair in s.images:                        # this rank's own pair: already on the device
        on_dev = s.images[pair]
        img1, img2 = (x.cpu().numpy() for x in on_dev)
    else:
        on_dev = img1, img2 = synth.make_pair(s.H, s.W, seed=seed)[:2]
    frame, counts = pipeline.frame_interp(on_dev[0], on_dev[1], fwd, bwd, t=0.5, fill_rounds=s.a.mid_fill_rounds,
                                          occl_thresh=s.a.mid_occl_thresh, counts=True)
    frame, counts = frame.cpu().numpy(), counts.cpu().tolist()
    flowio.write_png8(os.path.join(s.a.out, "mid_%02d.png" % pair), frame)
    truth, mask = synth.make_mid(s.H, s.W, seed=seed, t=0.5)
    half = np.float32(0.5)
    blend = np.floor(half * img1.astype(np.float32) + half * img2.astype(np.float32) + half).astype(np.uint8)
    row = dict(pair=pair, counts=dict(zip(pipeline.FRAME_INTERP_COUNTS, counts)), n=int(mask.sum()),
               psnr=psnr(frame, truth, mask), psnr_blend=psnr(blend, truth, mask))
    rows.append(row)
    print("pair %d: middle frame %s; PSNR %.2f dB, plain blend %.2f dB, over %d px"
          % (pair, " ".join("%s=%d" % kv for kv in row["counts"].items()), row["psnr"], row["psnr_blend"], row["n"]))


def stats_row(st, fields):
    """A dict of pipeline.eval_stats or photo_stats as a JSON object: the given fields, a NaN (nothing compared) as null."""
    return {k: (None if st[k] != st[k] else st[k]) for k in fields}


# what --eval and --photo differ in: the words of the statistics struct, pipeline's reader of it, the fields of a JSON row, the
# printed line and the fields it shows
EVAL = (8, "eval_stats", EVAL_ROW, "%s EPE %.3f px, %.2f%% > 3 px, Fl %.2f%% over %d px", ("mean_epe", "outliers_pct", "kitti_fl_pct", "n"))
PHOTO = (6, "photo_stats", PHOTO_ROW, "%s photometric error %.3f, %.2f%% > 10, over %d px (%d targets outside)",
         ("mean_err", "above_pct", "n", "n_outside"))


def tally(spec, pair, fields, run, rows, totals, dev):
    """--eval or --photo of one pair.  Per (kind, field): run(field) for the pair's own statistics, then run(field, stats=...)
    adds the field to the device total of its kind (created when the kind is first met).  Appends the pair's row to rows and
    prints its line."""
    import torch
    nwords, reader, row_fields, fmt, shown = spec
    read = getattr(mod("pipeline"), reader)
    row, line = {"pair": pair}, []
    for kind, field in fields:
        if kind not in totals:
            totals[kind] = torch.zeros(nwords, dtype=torch.int64, device=dev)
        st = read(run(field))                   # the pair's own row
        run(field, stats=totals[kind])          # and into the kind's total, on the device
        row[kind] = stats_row(st, row_fields)
        line.append(fmt % ((kind,) + tuple(st[k] for k in shown)))
    rows.append(row)
    print("pair %d: %s" % (pair, "; ".join(line)))


def write_tally(path, header, spec, rows, totals):
    """eval.json / photo.json: the header, the per-pair rows and, per kind, the totals read back from the device."""
    import json
    read = getattr(mod("pipeline"), spec[1])
    with open(path, "w") as f:
        json.dump(dict(header, pairs=rows, totals={kind: stats_row(read(t), spec[2]) for kind, t in totals.items()}), f, indent=1)


def setup(a):
    """The device and process group of this rank, the images of its passes on the device and its DiscreteFlow objects."""
    import torch
    import torch.distributed as dist
    pipeline, sharding, synth = mod("pipeline"), mod("sharding"), mod("synth")
    s = argparse.Namespace(a=a, stop=mod("bcdstats").stop_from_args(a), histories={})   # histories: pass index -> per-sweep history
    s.H, s.W = (int(v) for v in a.size.lower().split("x"))
    s.rank, s.world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    s.dev = torch.device("cuda", local)
    if s.world > 1:
        dist.init_process_group("nccl", device_id=s.dev)
    s.passes = [(pair, backward) for pair in range(a.pairs) for backward in (0, 1)]
    # this rank's pairs are generated and uploaded BEFORE the passes run: the compute functions are GPU work only
    mine = sharding.assign_passes(len(s.passes), s.world, s.rank)
    s.images = {}
    for pair in sorted({s.passes[i][0] for i in mine}):
        img1, img2, _ = synth.make_pair(s.H, s.W, seed=synth.pair_seed(pair, 0))
        s.images[pair] = (torch.from_numpy(img1).to(s.dev), torch.from_numpy(img2).to(s.dev))
    # the passes of a rank (forward and backward runs, several pairs) are independent: their front ends run one after the
    # other, their BCD sweeps as batched launches (dflow_bcd_sweep_batch), `group` passes at a time
    s.group = max(1, min(a.group, len(mine)))
    flags = mod("_lib").FLAG_DESCR_F16 if a.fp16_descriptors else 0
    ch, cw = (int(v) for v in a.cell.lower().split("x")) if a.cell else (None, None)
    # per pass of a group its DiscreteFlow objects, level 0 first; a plain run has the one level, and its object is built with
    # the cells as given (PyramidFlow clips them to the image), so the library still refuses what it refused
    if a.pyramid > 1:
        s.levels = [pipeline.PyramidFlow(s.H, s.W, a.pyramid, ch, cw, device=s.dev, seed=s.rank, fine_window=a.fine_window, flags=flags).levels
                    for _ in range(s.group)]
    else:
        s.levels = [[pipeline.DiscreteFlow(s.H, s.W, ch, cw, device=s.dev, seed=s.rank, flags=flags)] for _ in range(s.group)]
    s.dfs = [stack[0] for stack in s.levels]
    s.front = [torch.cuda.Stream(device=s.dev) for _ in range(min(3, s.group))]     # front ends of a group's passes side by side
    return s


def compute_many(s, descs):
    """The flows of this rank's passes `descs`, group by group: per group, the levels from the coarsest to level 0 (a plain run
    has only that one) for all its passes.  A level's front ends (at the coarsest level after the image pyramid, at the others
    with the prior step) run on the front streams, its sweeps as one batch on the main stream, where its flows are then
    upsampled into the next level's priors.  With a stop rule the histories of level 0 go to s.histories."""
    import torch
    pipeline = mod("pipeline")
    flows = []
    main = torch.cuda.current_stream(s.dev)
    coarse_times = s.a.bcd_times if s.a.coarse_bcd_times is None else s.a.coarse_bcd_times
    for g0 in range(0, len(descs), s.group):
        part = descs[g0:g0 + s.group]
        stacks = s.levels[:len(part)]
        pyramids, priors = [None] * len(part), [None] * len(part)
        for level in range(len(stacks[0]) - 1, -1, -1):
            start = torch.cuda.Event()
            start.record(main)                               # the previous group's read-out, or the next coarser level, is done
            done = []
            for j, (stack, (pair, backward)) in enumerate(zip(stacks, part)):
                st = s.front[j % len(s.front)]
                with torch.cuda.stream(st):
                    st.wait_event(start)
                    if pyramids[j] is None:
                        pyramids[j] = pipeline.image_pyramid(stack, *(s.images[pair][::-1] if backward else s.images[pair]))
                    if priors[j] is not None:
                        priors[j].record_stream(st)          # made on the main stream
                    stack[level].front_end(*pyramids[j][level], prior=priors[j], pack=True)
                    e = torch.cuda.Event()
                    e.record(st)
                    done.append(e)
            for e in done:
                main.wait_event(e)
            dfs = [stack[level] for stack in stacks]
            hist = pipeline.ceoBCD_batch(dfs, s.a.bcd_times if level == 0 else coarse_times, stop=s.stop if level == 0 else None)
            if level > 0:
                priors = [pipeline.flow_upsample(df.vratiKonacniFlow(), (stack[level - 1].p.pich, stack[level - 1].p.picw))
                          for df, stack in zip(dfs, stacks)]
        if hist is not None:
            for desc, h in zip(part, hist):
                s.histories[s.passes.index(desc)] = h
        if s.a.confidence is None:
            flows += [df.vratiKonacniFlow().clone() for df in dfs]
        else:                                                # [dy, dx, margin]: one tensor per pass to gather
            flows += [torch.cat([df.vratiKonacniFlow(), df.confidence(mode=s.a.conf_mode, min_sep=s.a.conf_sep)[..., None]], dim=2)
                      for df in dfs]
    return flows


def run_passes(s):
    """Every pass on its rank and the flows gathered on rank 0 (with --time twice, the second run timed); the histories of
    a stop rule are gathered into s.histories."""
    import torch
    import torch.distributed as dist
    a, H, W = s.a, s.H, s.W

    like = s.dfs[0].flow if a.confidence is None else torch.empty((H, W, 3), dtype=torch.float32, device=s.dev)

    def run():
        return mod("sharding").run_passes(s.passes, None, s.world, s.rank, like, compute_many=lambda descs: compute_many(s, descs))

    def settle():
        torch.cuda.synchronize()
        if s.world > 1:
            dist.barrier()
    flows = run()
    if a.time:
        import time
        settle()
        t0 = time.perf_counter()
        flows = run()
        settle()
        dt = time.perf_counter() - t0
        if s.rank == 0:
            n = len(s.passes)
            print("%d passes (%d pairs, forward + backward) of %dx%d, bcd_times=%d on %d GPU(s): %.1f ms = %.2f ms per pass = %.1f Mpix/s"
                  % (n, a.pairs, W, H, a.bcd_times, s.world, dt * 1e3, dt * 1e3 / n, n * H * W / dt / 1e6))
    if s.stop is not None and s.world > 1:
        gathered = [None] * s.world
        dist.all_gather_object(gathered, s.histories)
        s.histories = {k: v for g in gathered for k, v in g.items()}
    return flows


def write_pair(s, pair, fwd, bwd, margin=None):
    """The flow, sparse-field, edge and Epic files of one pair and its printed line; returns the sparse field on the device,
    the final dense flow (None without --epic) and the pair's images (None unless a stage asked for them).  margin: the
    forward pass's margin plane under --confidence."""
    a = s.a
    pipeline, synth, flowio = mod("pipeline"), mod("synth"), mod("flowio")
    sparse_dev = pipeline.flow_consistency(fwd, bwd, a.thresh) if a.check == "natural" else pipeline.fb_consistency(fwd, bwd, a.thresh)
    if a.segments is not None:
        sparse_dev, seg_counts = pipeline.segment_filter(sparse_dev, a.segments[1], a.segments[0], counts=True)
        print("pair %d: %d segments, %d removed; %d consistent pixels, %d removed" % ((pair,) + tuple(seg_counts.cpu().tolist())))
    img1 = img2 = epic = None
    if a.edges or a.epic or a.photo or a.wmedian is not None or a.wmedian_reject is not None:
        img1, img2 = s.images[pair] if pair in s.images else synth.make_pair(s.H, s.W, seed=synth.pair_seed(pair, 0))[:2]
    if a.wmedian_reject is not None:
        sparse_dev, wm_counts = pipeline.flow_wmedian(sparse_dev, img1, radius=a.wmedian_reject[0], reject=a.wmedian_reject[1], counts=True)
        print("pair %d: weighted median rejection: %s" % (pair, " ".join("%s=%d" % kv for kv in zip(pipeline.FLOW_WMEDIAN_COUNTS,
                                                                                                     wm_counts.cpu().tolist()))))
    if margin is not None:
        sparse_dev, gate_counts = pipeline.flow_gate(sparse_dev, margin, lo=a.confidence, counts=True)
        print("pair %d: confidence gate at margin >= %g: %d of %d checked vectors stay" % ((pair, a.confidence) + tuple(gate_counts.cpu().tolist()[::-1])))
        np.save(os.path.join(a.out, "margin_%02d.npy" % pair), margin.cpu().numpy())
    if a.epipolar is not None:
        sparse_dev = epipolar_pair(s, pair, sparse_dev)
    sparse_raw = sparse_dev                     # --prefilter hands a filtered copy to the interpolation
    sparse = sparse_dev.cpu().numpy()
    for backward, f in ((0, fwd), (1, bwd)):
        np.save(os.path.join(a.out, flowio.flow_name(pair, backward, a.bcd_times)), f.cpu().numpy().astype(np.float64))
    flowio.write_flo(os.path.join(a.out, flowio.flow_name(pair, 0, a.bcd_times)[:-4] + ".flo"), fwd.cpu().numpy())
    np.save(os.path.join(a.out, "sparse_field_%02d.npy" % pair), sparse)
    mod("evaluate").parovi(sparse, os.path.join(a.out, "parovi_%02d.txt" % pair))
    if a.edges or a.epic:
        if a.edge_kind == "pb":
            ivice = pipeline.pb_edges(img1)               # e itself for the GPU steps, 1 - e in the file
        else:
            _, ivice = pipeline.canny_edges(img1)
    if a.edges and a.edge_kind == "pb":
        mod("edge").write_pb_ivice(ivice, os.path.join(a.out, "ivice_%02d.bin" % pair))
    elif a.edges:
        ivice.cpu().numpy().tofile(os.path.join(a.out, "ivice_%02d.bin" % pair))
    if a.epic:
        if a.prefilter:
            sparse_dev = pipeline.epic_prefilter(sparse_dev, ivice, img1)
        epic = pipeline.epic_interpolate(sparse_dev, ivice)
        if a.epic_refine:
            epic = pipeline.variational_refine(img1, img2, epic)
        flowio.write_flo(os.path.join(a.out, "epic_%02d.flo" % pair), epic.cpu().numpy())
    print("pair %d: %.1f%% of the forward flow survives the consistency check" % (pair, 100.0 * sparse[..., 2].mean()))
    return sparse_raw, epic, img1, img2


def write_out(s, flows):
    """Rank 0: every file of DIR and every printed line after the passes."""
    import torch
    a, H, W = s.a, s.H, s.W
    pipeline, synth, flowio, evaluate, bcdstats = mod("pipeline"), mod("synth"), mod("flowio"), mod("evaluate"), mod("bcdstats")
    os.makedirs(a.out, exist_ok=True)
    if s.stop is not None:
        named = [("pair %d backward=%d" % s.passes[i], s.histories[i]) for i in sorted(s.histories)]
        bcdstats.write_history_json(os.path.join(a.out, "bcd_stats.json"), named, s.dfs[0].p.lamda, a.bcd_times, s.stop, (H, W),
                                    extra={"pyramid": a.pyramid} if a.pyramid > 1 else None)
        for name, h in named:
            print("%s: %d sweeps, E %.3f -> %.3f, last sweep changed %d labels"
                  % (name, len(h) - 1, h[0]["energy"], h[-1]["energy"], h[-1]["n_changed"]))
    eval_rows, eval_totals = [], {}
    photo_rows, photo_totals = [], {}
    mid_rows = []
    motion_rows = []
    s.epipolar_rows = []
    for pair in range(a.pairs):
        fwd, bwd, margin = flows[2 * pair], flows[2 * pair + 1], None
        if a.confidence is not None:            # [dy, dx, margin] per pass
            fwd, bwd, margin = fwd[..., :2].contiguous(), bwd[..., :2].contiguous(), fwd[..., 2].contiguous()
        if a.motion is not None:
            matrix, residual, counts = pipeline.motion_fit(fwd, model=a.motion, thresh=a.motion_thresh, residual=True, counts=True)
            flowio.write_field(os.path.join(a.out, "residual_%02d.flo" % pair), residual.cpu().numpy())
            counts = counts.cpu().tolist()
            motion_rows.append(dict(pair=pair, matrix=matrix.cpu().numpy().tolist(), scored=counts[0], inliers=counts[1]))
            print("pair %d: %s motion: %d of %d vectors within %g px (%.2f%%)"
                  % (pair, a.motion, counts[1], counts[0], a.motion_thresh, 100.0 * counts[1] / max(counts[0], 1)))
        sparse_raw, epic, img1, img2 = write_pair(s, pair, fwd, bwd, margin)
        dense = [("epic", epic)] if a.epic else []
        if a.wmedian is not None:
            filtered = pipeline.flow_wmedian(fwd, img1, radius=a.wmedian)
            flowio.write_field(os.path.join(a.out, "wmedian_%02d.flo" % pair), filtered.cpu().numpy())
            dense = [("filtered", filtered)] + dense
        if a.eval:
            gt = synth.make_pair(H, W, seed=synth.pair_seed(pair, 0))[2]
            gt = torch.from_numpy(evaluate.to_uv_valid(gt) if gt.shape[2] == 2 else np.asarray(gt, np.float32)).to(s.dev)
            confident = [("confident", pipeline.flow_gate(fwd, margin, lo=a.confidence))] if margin is not None else []
            tally(EVAL, pair, [("fwd", fwd), ("sparse", sparse_raw)] + confident + dense, lambda field, **kw: pipeline.flow_eval(field, gt, **kw),
                  eval_rows, eval_totals, s.dev)
        if a.pictures:
            for name, field in [("flowcolor", fwd)] + [("flowcolor_" + kind, f) for kind, f in dense]:
                flowio.write_png8(os.path.join(a.out, "%s_%02d.png" % (name, pair)), pipeline.flow_color(field).cpu().numpy())
        if a.photo:
            tally(PHOTO, pair, [("fwd", fwd)] + dense, lambda field, **kw: pipeline.warp_eval(img1, img2, field, **kw),
                  photo_rows, photo_totals, s.dev)
        if a.midframe:
            midframe_pair(s, pair, fwd, bwd, mid_rows)
    head = {"size": [H, W], "bcd_times": a.bcd_times}
    if a.pyramid > 1:
        head["pyramid"] = a.pyramid
    if a.motion is not None:
        import json
        with open(os.path.join(a.out, "motion.json"), "w") as f:
            json.dump(dict(head, model=a.motion, thresh=a.motion_thresh, pairs=motion_rows), f, indent=1)
    if a.epipolar is not None:
        import json
        if a.motion == "homography":            # both fits' counts side by side, nothing more: the homography is fitted to the forward flow
            for row, m in zip(s.epipolar_rows, motion_rows):
                row["homography"] = dict(scored=m["scored"], inliers=m["inliers"], thresh=a.motion_thresh)
        with open(os.path.join(a.out, "epipolar.json"), "w") as f:
            json.dump(dict(head, thresh=a.epipolar, gate=bool(a.epipolar_gate), pairs=s.epipolar_rows), f, indent=1)
    if a.midframe:
        import json
        with open(os.path.join(a.out, "midframe.json"), "w") as f:
            json.dump(dict(head, t=0.5, fill_rounds=a.mid_fill_rounds, occl_thresh=a.mid_occl_thresh, pairs=mid_rows), f, indent=1)
    if a.photo:
        write_tally(os.path.join(a.out, "photo.json"), dict(head, err_thresh=10.0, err_max=30.0), PHOTO, photo_rows, photo_totals)
    if a.eval:
        if a.check != "reference":
            head["check"] = a.check
        if a.segments is not None:
            head["segments"] = [a.segments[0], a.segments[1]]
        if a.wmedian is not None:
            head["wmedian"] = a.wmedian
        if a.wmedian_reject is not None:
            head["wmedian_reject"] = [a.wmedian_reject[0], a.wmedian_reject[1]]
        if a.confidence is not None:
            head["confidence"] = [a.confidence, a.conf_mode, a.conf_sep]
        write_tally(os.path.join(a.out, "eval.json"), dict(head, abs_thresh=3.0), EVAL, eval_rows, eval_totals)


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    a.conf_mode, a.conf_sep = mod("labelconf").from_args(ap, a)
    if a.confidence is not None:
        a.confidence = mod("labelconf").threshold(a.confidence, ap.error)
    a.epic = a.epic or a.epic_refine or a.prefilter
    if a.segments is not None:
        a.segments = segments_arg(a.segments)
    if a.wmedian is not None:
        a.wmedian = wmedian_arg(a.wmedian)
    if a.wmedian_reject is not None:
        a.wmedian_reject = wmedian_reject_arg(a.wmedian_reject)
    a.mid_fill_rounds, a.mid_occl_thresh = midframe_args(a)
    a.motion, a.motion_thresh = motion_args(a)
    a.epipolar = epipolar_arg(a)
    a.pose = pose_arg(a)
    if a.pyramid < 1 or (a.pyramid == 1 and (a.coarse_bcd_times is not None or a.fine_window is not None)):
        raise SystemExit("run_batch: --pyramid L needs L >= 1, and --coarse-bcd-times and --fine-window need L > 1")
    s = setup(a)
    flows = run_passes(s)
    if s.rank == 0:
        write_out(s, flows)
    if s.world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
