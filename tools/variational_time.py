#!/usr/bin/env python3
"""Times dflow_var_refine: median of 20 calls between HIP events at 1024x436 and 1242x375, the defaults and the kitti
preset, fused and unfused solver.  One line per configuration, then one JSON line.  --size and --preset restrict
the run.  Per-kernel times (profiles/var_kernel_stats.csv):
`rocprofv3 --kernel-trace --stats -d DIR -o s --output-format csv -- python3 tools/variational_time.py --size 1024x436 --preset default --calls 10`."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", default=None, help="WxH: only this size")
    ap.add_argument("--preset", default=None, choices=("default", "kitti"), help="only this parameter set")
    a = ap.parse_args()
    import torch
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    L = importlib.import_module(PKG + "._lib")
    dev = torch.device("cuda", 0)
    rows = []
    for H, W in ((436, 1024), (375, 1242)):
        if a.size not in (None, "%dx%d" % (W, H)):
            continue
        img1, img2, gt = synth.make_pair(H, W, seed=9, amp_x=6, amp_y=4)
        t1, t2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
        flow = torch.from_numpy((gt + 0.5).astype(np.float32)).to(dev)
        for preset in (None, "kitti"):
            if a.preset not in (None, preset or "default"):
                continue
            for name, flags in (("fused", 0), ("unfused", L.VAR_FLAG_SOR_UNFUSED)):
                ms = []
                for i in range(a.calls + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pipeline.variational_refine(t1, t2, flow, preset=preset, flags=flags)
                    e1.record()
                    e1.synchronize()
                    if i >= 2:
                        ms.append(e0.elapsed_time(e1))
                row = dict(size="%dx%d" % (W, H), preset=preset or "default", solver=name, median_ms=float(np.median(ms)),
                           min_ms=float(np.min(ms)), calls=a.calls)
                rows.append(row)
                print("%(size)s %(preset)-8s %(solver)-8s median %(median_ms).3f ms  min %(min_ms).3f ms" % row, flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
