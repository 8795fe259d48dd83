#!/usr/bin/env python3
"""Drop-in for the reference's first CLI (README.md:6-12, daisy i flann.py:16-27):

    python "daisy i flann.py" <idx <= 99> <backward 0|1> <dopython 0|1> [options]

Same positional arguments, same image naming (../data_scene_flow/training/image_2/0001{idx}_1{0|1}.png), same
output files in the current directory: the WTA flow/labels "posle 00", proposals_nakon_gausa,
lcosts_nakon_gausa, nprop -- in the reference's dtypes -- plus a Middlebury .flo next to every flow .npy.
The compat bit matrices (packedksets; with dopython=0 the four 'pakovani za c' copies) exist for users of the reference's own
BCD scripts (its `python bcd.py:76` cannot start without packedksets.npy); the GPU BCD of this package builds its own compact
lists in HBM and never reads them.  They are written by default while the file stays below PACKEDKSETS_DEFAULT_LIMIT bytes
(256 MiB: frames up to about 47 000 pixels); for larger frames (KITTI: 2.6 GB) one line says so and names the flag,
--packedksets writes them regardless of size, --no-packedksets never.
All computation runs in libdflow.so on the GPU; there is no CPU fallback.

Options for inputs the reference cannot handle: --image1/--image2 PATH, --cell HxW, --synthetic HxW
(synthetic pair with seed 1000*idx+backward), --seed N (neighbour-sampler key), --device cuda:N,
--fp16-descriptors (BASELINE configs[4]: DAISY values rounded to binary16).

Starting from a flow somebody already has (DESIGN.md "Prior proposals"): --prior FILE, a .npy of shape (H,W,2) [dy,dx] or
(H,W,3) [U,V,valid], or a Middlebury .flo.  Its vectors are appended to the pixels' label sets after nasumicni, so
proposals_nakon_gausa, lcosts_nakon_gausa and nprop hold them; "posle 00" stays the kNN winner, and the labelling that starts on
the prior goes to "Daisy output slike <idx> backward=<b> labels_prior.npy", which `python bcd.py --labels` takes.  maxnprop stays
150 here, so the prior fills free slots only (maxnprop - nprop per pixel); one printed line gives how many candidates were
appended, found, met a full row or were skipped.  --prior-stride N (default 2; 0: the pixel's own vector only) also offers the
vectors of the four pixels N away; --prior-advance carries every vector to the pixel it points at first (the previous pair's
flow as a constant-velocity prior), --prior-inverse does the same and negates it (the other direction's flow as a prior);
--no-prior-seed leaves the starting labels alone (labels_prior then equals "posle 00").
Seed only a prior you believe: started on a wrong but smooth flow the sweeps stay on it (the control run).

Coarse to fine (DESIGN.md "Coarse to fine"): --pyramid L runs L - 1 coarser levels of the pair to completion in this process
(pipeline.PyramidFlow: half the size per level, the same cells in pixels, --coarse-bcd-times N sweeps each, default 4) and uses
the upsampled flow of level 1 where --prior FILE would stand: the files are those of --prior, labels_prior included, and
--prior-stride and --no-prior-seed apply.  --fine-window W (0..2) narrows the kNN search of the full-size level to +-W cells.
--pyramid together with --prior is refused.  --gate T (pixels of the level it is applied at; needs --pyramid L > 1): every coarse
level runs in both directions and its two flows go through the forward/backward check in image coordinates
(pipeline.flow_consistency, DESIGN.md "Forward/backward check in image coordinates") before they are upsampled, so a coarse vector
that fails the check is no prior for the next level.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))


PACKEDKSETS_DEFAULT_LIMIT = 256 << 20


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("picindex"); ap.add_argument("backward", choices=("0", "1")); ap.add_argument("dopython", choices=("0", "1"))
    ap.add_argument("--image1"); ap.add_argument("--image2"); ap.add_argument("--cell"); ap.add_argument("--synthetic")
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--packedksets", action="store_true", help="write the reference's compat-matrix file(s) whatever their size")
    ap.add_argument("--no-packedksets", action="store_true", help="never write them")
    ap.add_argument("--fp16-descriptors", action="store_true", help="round the DAISY values to binary16 (DFLOW_FLAG_DESCR_F16)")
    ap.add_argument("--prior", metavar="FILE", help=".npy (H,W,2) [dy,dx] or (H,W,3) [U,V,valid], or .flo: a flow to start from; "
                    "maxnprop stays 150, so it fills free label slots only")
    ap.add_argument("--prior-stride", type=int, default=2, metavar="N", help="also offer the prior of the four pixels N away (0: own pixel only)")
    ap.add_argument("--prior-advance", action="store_true", help="carry the prior's vectors to the pixels they point at first")
    ap.add_argument("--prior-inverse", action="store_true", help="the same, negated: the other direction's flow as a prior")
    ap.add_argument("--no-prior-seed", action="store_true", help="append the prior's labels but do not start the labelling on them")
    ap.add_argument("--pyramid", type=int, default=1, metavar="L", help="coarse to fine: L levels, the coarser ones produce the prior")
    ap.add_argument("--coarse-bcd-times", type=int, default=None, metavar="N", help="BCD sweeps of every coarse level of --pyramid (default 4)")
    ap.add_argument("--fine-window", type=int, default=None, metavar="W", help="with --pyramid: the kNN window of the full-size level")
    ap.add_argument("--gate", type=float, default=None, metavar="T", help="with --pyramid: coarse levels run both ways, vectors failing the "
                    "forward/backward check by more than T px are no prior")
    a = ap.parse_args(argv)
    if a.gate is not None and (a.pyramid <= 1 or not (np.isfinite(a.gate) and a.gate >= 0)):
        ap.error("--gate T needs --pyramid L with L > 1 and a finite T >= 0")
    if a.pyramid < 1:
        ap.error("--pyramid L needs L >= 1")
    if a.pyramid > 1 and a.prior is not None:
        ap.error("--pyramid produces the prior itself: it excludes --prior FILE")
    if a.pyramid == 1 and (a.fine_window is not None or a.coarse_bcd_times is not None):
        ap.error("--coarse-bcd-times and --fine-window need --pyramid L with L > 1")
    if a.prior is None and (a.prior_advance or a.prior_inverse):
        ap.error("--prior-advance and --prior-inverse need --prior FILE")
    if a.prior is None and a.pyramid == 1 and (a.no_prior_seed or a.prior_stride != 2):
        ap.error("--prior-stride and --no-prior-seed need --prior FILE or --pyramid L")
    if a.prior_advance and a.prior_inverse:
        ap.error("--prior-advance and --prior-inverse exclude each other")
    pipeline = importlib.import_module(PKG + ".pipeline")
    flowio = importlib.import_module(PKG + ".flowio")
    synth = importlib.import_module(PKG + ".synth")
    idx = a.picindex if len(a.picindex) > 1 else "0" + a.picindex            # daisy i flann.py:24-25
    if a.synthetic:
        h, w = (int(v) for v in a.synthetic.lower().split("x"))
        pic1, pic2, _ = synth.make_pair(h, w, seed=synth.pair_seed(int(idx), 0))
        if a.backward == "1":
            pic1, pic2 = pic2, pic1
    else:
        other = "1" if a.backward == "0" else "0"                           # :19-22
        base = "../data_scene_flow/training/image_2/0001" + idx + "_1"
        pic1 = flowio.read_bgr(a.image1 or base + a.backward + ".png")
        pic2 = flowio.read_bgr(a.image2 or base + other + ".png")
        if not (a.image1 or a.image2):                                      # :34-35,52-53 KITTI crop
            pic1, pic2 = pic1[:375, :1241], pic2[:375, :1241]
    pich, picw = pic1.shape[:2]
    cellh, cellw = (int(v) for v in a.cell.lower().split("x")) if a.cell else pipeline.default_cells(pich, picw)
    flags = importlib.import_module(PKG + "._lib").FLAG_DESCR_F16 if a.fp16_descriptors else 0
    prior = None
    if a.pyramid > 1:
        pf = pipeline.PyramidFlow(pich, picw, a.pyramid, cellh, cellw, device=a.device, seed=a.seed, fine_window=a.fine_window, flags=flags)
        df = pf.levels[0]
        prior = pf.coarse_prior(pf.image_pyramid(np.ascontiguousarray(pic1), np.ascontiguousarray(pic2)),
                                4 if a.coarse_bcd_times is None else a.coarse_bcd_times,
                                a.prior_stride, not a.no_prior_seed, **(dict(gate=a.gate, pair=True) if a.gate is not None else {}))
        if a.gate is not None:
            prior = prior[0]                                                # the direction of this run
    else:
        df = pipeline.DiscreteFlow(pich, picw, cellh, cellw, device=a.device, seed=a.seed, flags=flags)
    df.load_pair(np.ascontiguousarray(pic1), np.ascontiguousarray(pic2))    # :406-407
    df.generisi()                                                           # :409-412
    flow0 = df.vratiKonacniFlow().cpu().numpy().astype(np.float64)
    st0 = df.host_state()
    np.save(flowio.flow_name(idx, a.backward, 0), flow0)                    # sacuvajPodatke0 :200-202
    np.save(flowio.labels_name(idx, a.backward, 0), st0["bestlabels"])
    flowio.write_flo(flowio.flow_name(idx, a.backward, 0)[:-4] + ".flo", flow0)
    df.nasumicni()                                                          # :418
    if a.prior is not None:
        prior = flowio.read_flo(a.prior)[..., ::-1] if a.prior.lower().endswith(".flo") else np.load(a.prior)
        prior = np.ascontiguousarray(prior, dtype=np.float32)
        if a.prior_advance or a.prior_inverse:
            prior = pipeline.flow_advance(prior, negate=a.prior_inverse)
    if prior is not None:
        counts = df.prior_proposals(prior, stride=a.prior_stride, seed_labels=not a.no_prior_seed, counts=True).cpu().tolist()
        np.save(flowio.stage_name(idx, a.backward, "labels_prior"), df.bestlabels.cpu().numpy().astype(np.int64))
        source = os.path.basename(a.prior) if a.prior else "of %d pyramid levels" % a.pyramid
        print("daisy i flann: prior %s: appended %d, found %d, full %d, skipped %d" % ((source,) + tuple(counts)))
    st = df.host_state()
    np.save(flowio.stage_name(idx, a.backward, "proposals_nakon_gausa"), st["proposals"])   # sacuvajPodatke1 :249-253
    np.save(flowio.stage_name(idx, a.backward, "lcosts_nakon_gausa"), st["lcosts"])
    np.save(flowio.stage_name(idx, a.backward, "nprop"), st["nprop"])
    pk_bytes = pich * picw * 2 * (df.p.maxnprop * df.p.maxnprop // 8 + 1)
    if not a.packedksets and not a.no_packedksets and pk_bytes > PACKEDKSETS_DEFAULT_LIMIT:
        print("daisy i flann: packedksets (%.2f GB) not written: this package's `python bcd.py` builds its own lists on the GPU; "
              "pass --packedksets if the reference's own `python bcd.py` is to read these files" % (pk_bytes / 1e9))
    if a.packedksets or (not a.no_packedksets and pk_bytes <= PACKEDKSETS_DEFAULT_LIMIT):   # pakovanje :308 / pakovanjeZaC :394-397
        compat = importlib.import_module(PKG + ".compat")
        pk = compat.packedksets(df)
        if a.dopython == "1":
            np.save(flowio.stage_name(idx, a.backward, "packedksets"), pk)
        else:
            for k, arr in enumerate(compat.pakovani_za_c(pk)):
                np.save(flowio.stage_name(idx, a.backward, "pakovani za c %d" % k), arr)
    print("daisy i flann: %dx%d, cells %dx%d, nprop %d..%d" % (picw, pich, cellw, cellh, st["nprop"].min(), st["nprop"].max()))


if __name__ == "__main__":
    main()
