#!/usr/bin/env python3
"""Drop-in for the reference's second CLI (README.md:15-21, python bcd.py:13-17):

    python "python bcd.py" <idx <= 99> <backward 0|1> <bcd_times> [--device cuda:N] [--confidence [--conf-mode M] [--conf-sep S]]

Loads the files the first CLI wrote (ucitajSvePodatkeDoBCD, python bcd.py:67-81; always the "posle 00"
labels), runs bcd_times BCD sweeps on the GPU and, after every sweep, writes the reference's two .npy files
(python bcd.py:282-283) plus a Middlebury .flo of the same flow.  packedksets.npy is neither needed nor read.

--stats prints one line per sweep (sweep, changed labels, data sum, smoothness sum, image energy E = lamda * data + smooth;
sweep 0 is the labelling that was loaded) and writes "Daisy output slike <idx> backward=<b> bcd_stats.json" (DESIGN.md "BCD
statistics and the stop rule").  --stop-changed F ends the run after the sweep that changed at most the fraction F of the
labels, --stop-energy R after the sweep that lowered E by at most the fraction R (a rise of E included); bcd_times stays the
upper bound, and the files of the sweeps not run are not written.  Each of the three costs one read-back of 48 bytes per
sweep; without them the run issues exactly the launches it always did.

--labels FILE starts from the labels in that .npy instead of "posle 00": the labels_prior file `daisy i flann.py --prior` (or --pyramid) writes,
or any (H,W) integer labelling with 0 <= label < nprop.

--confidence writes, next to the flow of the last sweep that ran, "Margin slike <idx> backward=<b> posle <w> BCD.npy"
(flowio.margin_name): the (H,W) float32 margin plane of the final labelling (DiscreteFlow.confidence, DESIGN.md "Label
confidence"), +Inf where no label competes.  --conf-mode local|data picks the energy (default local), --conf-sep S the L1 distance
up to which a label counts as the chosen motion itself (0..1024, default 1).  Without it nothing is launched that was not
launched before.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.basename(os.path.dirname(os.path.abspath(__file__)))


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("picindex"); ap.add_argument("backward", choices=("0", "1")); ap.add_argument("bcd_times", type=int)
    ap.add_argument("--cell"); ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--labels", metavar="FILE", help="start from these labels (an (H,W) integer .npy) instead of \"posle 00\"")
    importlib.import_module(PKG + ".bcdstats").add_cli_options(ap, "--stats")
    importlib.import_module(PKG + ".labelconf").add_cli_options(ap, with_threshold=False)
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    conf_mode, conf_sep = importlib.import_module(PKG + ".labelconf").from_args(ap, a)
    bcdstats = importlib.import_module(PKG + ".bcdstats")
    stop = bcdstats.stop_from_args(a)
    pipeline = importlib.import_module(PKG + ".pipeline")
    flowio = importlib.import_module(PKG + ".flowio")
    idx = a.picindex if len(a.picindex) > 1 else "0" + a.picindex
    proposals = np.load(flowio.stage_name(idx, a.backward, "proposals_nakon_gausa"))
    lcosts = np.load(flowio.stage_name(idx, a.backward, "lcosts_nakon_gausa"))
    nprop = np.load(flowio.stage_name(idx, a.backward, "nprop"))
    bestlabels = np.load(a.labels if a.labels is not None else flowio.labels_name(idx, a.backward, 0))
    pich, picw = nprop.shape
    if a.labels is not None and not (bestlabels.shape == nprop.shape and np.issubdtype(bestlabels.dtype, np.integer)
                                     and (bestlabels >= 0).all() and (bestlabels < nprop).all()):
        raise SystemExit("python bcd: --labels %s is not an (%d,%d) integer labelling with 0 <= label < nprop" % (a.labels, pich, picw))
    cellh, cellw = (int(v) for v in a.cell.lower().split("x")) if a.cell else pipeline.default_cells(pich, picw)
    df = pipeline.DiscreteFlow(pich, picw, cellh, cellw, device=a.device)
    df.set_host_state(proposals, lcosts, nprop, bestlabels)

    def save(w):
        flow = df.vratiKonacniFlow().cpu().numpy().astype(np.float64)
        np.save(flowio.flow_name(idx, a.backward, w), flow)
        np.save(flowio.labels_name(idx, a.backward, w), df.bestlabels.cpu().numpy().astype(np.int64))
        flowio.write_flo(flowio.flow_name(idx, a.backward, w)[:-4] + ".flo", flow)
        print("uradjen bcd broj", w)

    history = df.ceoBCD(a.bcd_times, on_sweep=save, stop=stop)
    if a.confidence:
        last = a.bcd_times if history is None else len(history) - 1
        np.save(flowio.margin_name(idx, a.backward, last), df.confidence(mode=conf_mode, min_sep=conf_sep).cpu().numpy())
    if history is not None:
        for h in history:
            print(bcdstats.format_row(h))
        bcdstats.write_history_json(flowio.stage_name(idx, a.backward, "bcd_stats")[:-4] + ".json",
                                    [("backward=%s" % a.backward, history)], df.p.lamda, a.bcd_times, stop, (pich, picw))


if __name__ == "__main__":
    main()
