"""Coarse to fine, measured: python tools/pyramid_time.py.  1024x436, the bench frame and its synthetic pairs.
Kernels: dflow_pyr_down (one image, a pair) and dflow_flow_upsample (both layouts, with and without counts) on preallocated
buffers, HIP events, 7 calls each, with the bytes they must move and the rate at the fastest call.  Passes: the whole run
(PyramidFlow.run, 4 sweeps at every level, device images) for 1 level -- the plain pass, the yardstick -- and for 2 and 3 levels
with fine_window 2, 1 and 0; 7 calls, median and minimum.  Quality: for pairs 0 and 1 and the same configurations, seeded and
unseeded, the mean end-point error of the full-size level after 0, 1, 2 and 4 sweeps and the counts of its prior step and of
the upsampling.  The same (times and quality) for a configuration whose single level cannot reach the motion: window 1 and
14x32 cells on every level.  Prints JSON lines, the last one everything."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
pipeline = importlib.import_module(PKG + ".pipeline")
synth = importlib.import_module(PKG + ".synth")
L = importlib.import_module(PKG + "._lib")

H, W = 436, 1024
HC, WC = (H + 1) // 2, (W + 1) // 2
SWEEPS = (1, 2, 4)
out = {}


def timed(fn, reps=7):
    fn()                                                  # warm-up: code objects, the allocator's blocks
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "ms": ms}


def rate(t, nbytes):
    return dict(t, bytes=nbytes, GBps_at_min=nbytes / (t["min_ms"] * 1e-3) / 1e9)


def epe(flow, gt):
    return float((flow - gt).norm(dim=-1).mean())


pairs = []
for k in (0, 1):
    img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(k, 0))
    pairs.append((torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda(),
                  torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).cuda()))

# ---- the two kernels
dev = torch.device("cuda", torch.cuda.current_device())
s = L.stream(dev)
a1, a2, gt_d = pairs[0]
o1, o2 = (torch.empty((HC, WC, 3), dtype=torch.uint8, device=dev) for _ in range(2))
k = {}
k["pyr_down_one"] = rate(timed(lambda: L.call("dflow_pyr_down", H, W, a1.data_ptr(), None, o1.data_ptr(), None, s)), 3 * H * W + 3 * HC * WC)
k["pyr_down_pair"] = rate(timed(lambda: L.call("dflow_pyr_down", H, W, a1.data_ptr(), a2.data_ptr(), o1.data_ptr(), o2.data_ptr(), s)),
                          2 * (3 * H * W + 3 * HC * WC))
coarse_dydx = torch.round(torch.randn((HC, WC, 2), device=dev) * 10)
coarse_uvv = torch.cat([coarse_dydx.flip(-1), (torch.rand((HC, WC, 1), device=dev) > 0.1).float()], dim=-1).contiguous()
up, cnt = torch.empty((H, W, 3), dtype=torch.float32, device=dev), torch.empty(3, dtype=torch.int32, device=dev)
for name, c, lay, per in (("dydx", coarse_dydx, L.EVAL_DYDX, 8), ("uvv", coarse_uvv, L.EVAL_UVV, 12)):
    for with_counts in (False, True):
        t = timed(lambda: L.call("dflow_flow_upsample", H, W, c.data_ptr(), lay, up.data_ptr(), cnt.data_ptr() if with_counts else None, s))
        k["flow_upsample_%s%s" % (name, "_counts" if with_counts else "")] = rate(t, HC * WC * per + H * W * 12)
out["kernels"] = k
print("kernels", json.dumps(k), flush=True)


# ---- whole passes and their quality
def configs(base):
    yield "1 level", 1, None
    for levels in (2, 3):
        for fw in ((2, 1, 0) if base.get("window", 2) == 2 else (None,)):
            yield "%d levels, fine window %s" % (levels, base.get("window") if fw is None else fw), levels, fw


def quality(pf, img1, img2, gt, seed_labels):
    """Level 0's mean EPE after 0, 1, 2, 4 sweeps; the coarse levels run 4 sweeps."""
    pyr = pf.image_pyramid(img1, img2)
    prior = pf.coarse_prior(pyr, 4, 2, seed_labels, counts=True)
    df = pf.levels[0]
    df.load_pair(*pyr[0])
    df.generisi()
    df.nasumicni()
    r = {"epe": {}}
    if prior is not None:
        r["coarse_epe_in_fine_px"] = epe(prior[..., :2].flip(-1), gt)
        r["upsample_counts"] = pf.counts[-1][1].cpu().tolist()
        r["prior_counts"] = df.prior_proposals(prior, stride=2, seed_labels=seed_labels, counts=True).cpu().tolist()
    r["epe"][0] = epe(df.vratiKonacniFlow(), gt)
    done = 0
    for n in SWEEPS:
        df.ceoBCD(n - done)
        done = n
        r["epe"][n] = epe(df.vratiKonacniFlow(), gt)
    return r


for title, base in (("default", {}), ("short reach", {"window": 1, "cellh": 14, "cellw": 32})):
    res = {}
    for name, levels, fw in configs(base):
        pf = pipeline.PyramidFlow(H, W, levels, fine_window=fw, **base)
        row = {"pass": timed(lambda: pf.run(a1, a2, 4))}
        for pi, (img1, img2, gt) in enumerate(pairs):
            for seeded in ((True, False) if levels > 1 else (True,)):
                row["pair%d%s" % (pi, "" if levels == 1 else "_seeded" if seeded else "_unseeded")] = quality(pf, img1, img2, gt, seeded)
        res[name] = row
        print(title, "|", name, json.dumps(row), flush=True)
        del pf
    out[title] = res
print(json.dumps(out))
