"""Superpixels and per-segment models, measured: python tools/superpixel_time.py [reps].  1024x436, the bench
frame and its synthetic pairs.  Times: dflow_superpixels on preallocated planes, HIP events around the C call, for S = 8, 16 and
32 at 10 iterations and at 1 (the difference over 9 is one iteration: an assignment and a division) on a dense and on a
low-texture frame; dflow_segment_fit at R = 3 and R = 1 (half the difference is one round) on the BCD flow of pair 0 over the
S = 16 segments.  Quality, through dflow_flow_eval against synth's ground truth, pairs 0 and 1: the plain BCD flow after 4
sweeps, the models' flow fitted to it, the forward/backward-checked sparse field (10 px) and the models' flow fitted to that, on
all pixels and on the holes alone.  Prints JSON lines, the last one everything."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
pipeline, synth, L = (importlib.import_module(PKG + "." + m) for m in ("pipeline", "synth", "_lib"))

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
H, W = 436, 1024
dev = torch.device("cuda", torch.cuda.current_device())
s = L.stream(dev)
out = {"size": "%dx%d" % (W, H), "reps": reps}


def timed(fn):
    fn()                                                  # warm-up: code objects
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4)}


def i32(*shape):
    return torch.empty(shape, dtype=torch.int32, device=dev)


# ---- dflow_superpixels
label, slic, comp, size, fin, scan, cnt = i32(H, W), i32(H, W), i32(H, W), i32(H, W), i32(H, W), i32(-(-(H * W) // 256) + 1), i32(8)
res = {}
for style in synth.STYLES:
    img = torch.from_numpy(synth.make_pair(H, W, seed=synth.pair_seed(0, 0), style=style)[0]).to(dev)
    for S in (8, 16, 32):
        K = pipeline.superpixel_grid(H, W, S)[2]
        centers, sums = i32(K, 8), i32(K, 8)

        def call(iters):
            L.call("dflow_superpixels", H, W, img.data_ptr(), S, 10, iters, S * S // 4, 0, label.data_ptr(), centers.data_ptr(),
                   slic.data_ptr(), cnt.data_ptr(), sums.data_ptr(), comp.data_ptr(), size.data_ptr(), fin.data_ptr(), scan.data_ptr(), s)
        t10, t1 = timed(lambda: call(10)), timed(lambda: call(1))
        call(10)
        row = {"K": K, "iters10": t10, "iters1": t1, "per_iteration_ms": round((t10["median_ms"] - t1["median_ms"]) / 9, 4),
               "counts": dict(zip(pipeline.SUPERPIXEL_COUNTS[:7], cnt.cpu().tolist()))}
        res["%s S=%d" % (style, S)] = row
        print("superpixels", style, S, json.dumps(row), flush=True)
out["superpixels"] = res


# ---- the flows of the bench pairs
def gt3(gt):
    return torch.from_numpy(np.ascontiguousarray(np.stack([gt[..., 1], gt[..., 0], np.ones(gt.shape[:2])], axis=2), dtype=np.float32)).to(dev)


def epe(flow, gt):
    st = pipeline.eval_stats(pipeline.flow_eval(flow, gt))
    return {"n": st["n"], "mean_epe": round(st["mean_epe"], 4), "outliers_pct": round(st["outliers_pct"], 3)}


pairs = []
for k in (0, 1):
    img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(k, 0))
    df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
    fwd = df.run(img1, img2, 4).clone()
    bwd = df.run(img2, img1, 4).clone()
    pairs.append((torch.from_numpy(img1).to(dev), fwd, pipeline.flow_consistency(fwd, bwd, 10.0), gt3(gt)))
    del df

# ---- dflow_segment_fit
img, fwd, sparse, gt = pairs[0]
lab, c = pipeline.superpixels(img, step=16, counts=True)
n_seg = int(c[5].item())
models, segc = torch.empty((n_seg, 6), device=dev), i32(n_seg, 4)
acc, o, cls, fcnt = torch.empty((n_seg, 12), dtype=torch.int64, device=dev), torch.empty((H, W, 3), device=dev), \
    torch.empty((H, W), dtype=torch.uint8, device=dev), i32(8)
res = {"n_seg": n_seg}
for name, f in (("bcd_dydx", fwd), ("checked_uvv", sparse)):
    def fit(R):
        L.call("dflow_segment_fit", H, W, f.data_ptr(), L.EVAL_UVV if f.shape[2] == 3 else L.EVAL_DYDX, lab.data_ptr(), n_seg, 1.0, R, 0,
               models.data_ptr(), segc.data_ptr(), o.data_ptr(), cls.data_ptr(), fcnt.data_ptr(), acc.data_ptr(), s)
    t3, t1 = timed(lambda: fit(3)), timed(lambda: fit(1))
    fit(3)
    nbytes = H * W * (4 * f.shape[2] + 4)
    res[name] = {"rounds3": t3, "rounds1": t1, "per_round_ms": round((t3["median_ms"] - t1["median_ms"]) / 2, 4), "acc_bytes": nbytes,
                 "counts": dict(zip(pipeline.SEGMENT_FIT_COUNTS[:7], fcnt.cpu().tolist()))}
out["segment_fit"] = res
print("segment_fit", json.dumps(res), flush=True)

# ---- quality
res = {}
for k, (img, fwd, sparse, gt) in enumerate(pairs):
    holes = sparse[..., 2] == 0
    row = {"bcd": epe(fwd, gt), "checked": epe(sparse, gt), "holes": int(holes.sum().item())}
    for S in (8, 16, 32):
        for R in (1, 3, 6):
            for name, f in (("bcd", fwd), ("checked", sparse)):
                r = pipeline.superpixel_flow(img, f, step=S, thresh=1.0, rounds=R, counts=True)
                fit_flow, fc = r[3], r[4].cpu().tolist()
                e = {"n_seg": int(r[1].shape[0]), "all": epe(fit_flow, gt), "agree_pct": round(100.0 * fc[1] / max(fc[0], 1), 2),
                     "affine": fc[3], "translation": fc[4], "no_model_px": int((fit_flow[..., 2] == 0).sum().item())}
                if name == "checked":
                    at_holes = fit_flow.clone()
                    at_holes[~holes] = 0
                    e["at_the_holes"] = epe(at_holes, gt)
                    bcd_at_holes = torch.cat([fwd.flip(-1), holes[..., None].float()], dim=-1).contiguous()
                    row.setdefault("bcd_at_the_holes", epe(bcd_at_holes, gt))
                row["fit of %s, S=%d R=%d" % (name, S, R)] = e
    res["pair%d" % k] = row
    print("quality pair", k, json.dumps(row), flush=True)
out["quality"] = res
print(json.dumps(out))
