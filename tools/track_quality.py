"""What chaining buys on the two bench pairs: python tools/track_quality.py [sweeps]
1024x436.  For run_batch's pairs 0 and 1 the true frames at t = 0, 1/4, 1/2, 3/4, 1 (synth.make_mid), a forward and a backward
pass of `sweeps` sweeps (default 4) per consecutive pair of them, tracks seeded at frame 0 with step 1 and carried through the four
flows with the forward/backward test (pipeline.TrackSet, rel 0.01, abs 0.5); the displacement of the tracks that survive,
TrackSet.flow(0, 4), is evaluated against synth.forward_gt (pipeline.flow_eval): density, mean EPE, outliers above 3 px.  Beside
it the direct pass 0 -> 4: unchecked, after pipeline.flow_consistency(bilinear=True) at 1 px, and at the threshold on that
check's error plane that keeps as many vectors as the chain does, where one exists.  A measurement, no product code.  Prints one
JSON line."""
import importlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
synth, pipeline, evaluate = (importlib.import_module(PKG + "." + m) for m in ("synth", "pipeline", "evaluate"))
sweeps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
dev = torch.device("cuda", 0)
H, W = 436, 1024
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)


def stats(flow, gt):
    st = pipeline.eval_stats(pipeline.flow_eval(flow, gt))
    return {"density": round(st["n"] / (H * W), 4), "mean_epe": round(st["mean_epe"], 4), "outliers_pct": round(st["outliers_pct"], 3)}


res = {"size": "%dx%d" % (W, H), "sweeps": sweeps, "pairs": []}
for pair in (0, 1):
    seed = synth.pair_seed(pair, 0)
    frames = [synth.make_mid(H, W, seed=seed, t=t)[0] for t in (0.0, 0.25, 0.5, 0.75, 1.0)]
    gt = torch.from_numpy(evaluate.to_uv_valid(synth.forward_gt(H, W, seed))).to(dev)
    ts = pipeline.TrackSet(H, W, cap=H * W, step=1).seed()
    per_frame = []
    for a, b in zip(frames[:-1], frames[1:]):
        fwd = df.run(a, b, sweeps).clone()
        bwd = df.run(b, a, sweeps).clone()
        ts.advance(fwd, bwd)
        per_frame.append(dict(zip(pipeline.TRACK_ADVANCE_COUNTS, ts.counts()["advance"].cpu().tolist())))
    chained = ts.flow(0, 4)
    row = {"pair": pair, "advance_counts": per_frame, "chained": stats(chained, gt)}
    fwd = df.run(frames[0], frames[4], sweeps).clone()
    bwd = df.run(frames[4], frames[0], sweeps).clone()
    row["direct_unchecked"] = stats(fwd, gt)
    checked, err = pipeline.flow_consistency(fwd, bwd, 1.0, bilinear=True, err=True)
    row["direct_checked_1px"] = stats(checked, gt)
    formed = torch.sort(err[err >= 0])[0]
    want = int((chained[..., 2] > 0.5).sum())
    if 0 < want <= formed.numel():
        t = float(formed[want - 1])
        row["direct_at_chained_density"] = dict(stats(pipeline.flow_gate(fwd, err, lo=0.0, hi=t), gt), thresh=round(t, 4))
    else:
        row["direct_at_chained_density"] = None         # the check forms an error at fewer pixels than the chain keeps
    res["pairs"].append(row)
print(json.dumps(res))
