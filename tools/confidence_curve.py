"""The sparsification curve of the label margin on one synthetic pair: python tools/confidence_curve.py [pair] [mode] [min_sep] [sweeps]
1024x436, run_batch's pair `pair` (default 0), forward and backward pass of `sweeps` sweeps (default 4).  The forward flow is gated
at the deciles of three score planes and every gated field evaluated against the true flow (pipeline.flow_gate, then
pipeline.flow_eval): the margin of DiscreteFlow.confidence(mode, min_sep) (default local, 1; kept: margin >= its quantile), the
oracle (the true end-point error plane; kept: error <= its quantile) and the forward/backward error of
pipeline.flow_consistency(err=True) (kept: error <= its quantile, among the pixels where an error was formed).  Each row gives the
density (kept / pixels compared with the truth at full density), the mean EPE and the outliers above 3 px of what is kept.  A
measurement, no product code.  Prints one JSON line."""
import importlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
synth, pipeline, evaluate = (importlib.import_module(PKG + "." + m) for m in ("synth", "pipeline", "evaluate"))
pair = int(sys.argv[1]) if len(sys.argv) > 1 else 0
mode = sys.argv[2] if len(sys.argv) > 2 else "local"
min_sep = int(sys.argv[3]) if len(sys.argv) > 3 else 1
sweeps = int(sys.argv[4]) if len(sys.argv) > 4 else 4
dev = torch.device("cuda", 0)
H, W = 436, 1024
img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(pair, 0))
gt = torch.from_numpy(evaluate.to_uv_valid(gt) if gt.shape[2] == 2 else np.asarray(gt, np.float32)).to(dev)
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
fwd = df.run(img1, img2, sweeps).clone()
margin, counts = df.confidence(mode=mode, min_sep=min_sep, counts=True)
bwd = df.run(img2, img1, sweeps).clone()
full, err_true = pipeline.flow_eval(fwd, gt, err=True)
full = pipeline.eval_stats(full)
_, err_fb = pipeline.flow_consistency(fwd, bwd, 1e30, err=True)
INF = float("inf")


def curve(score, keep_high, usable):
    """Rows at the deciles of `score` over the pixels `usable`: keep_high keeps score >= quantile, else score <= quantile."""
    v = torch.sort(score[usable])[0]
    rows = []
    for d in (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1):
        k = min(v.numel() - 1, max(0, int(round((1.0 - d) * v.numel())) if keep_high else int(round(d * v.numel())) - 1))
        t = float(v[k])
        lo, hi = (t, INF) if keep_high else (0.0, t)
        st = pipeline.eval_stats(pipeline.flow_eval(pipeline.flow_gate(fwd, score, lo=lo, hi=hi), gt))
        rows.append({"quantile": d, "thresh": None if t != t or abs(t) == INF else round(t, 5) if abs(t) < 1e30 else t,
                     "density": round(st["n"] / max(full["n"], 1), 4), "mean_epe": round(st["mean_epe"], 4),
                     "outliers_pct": round(st["outliers_pct"], 3)})
    return rows


res = {"size": "%dx%d" % (W, H), "pair": pair, "mode": mode, "min_sep": min_sep, "sweeps": sweeps,
       "counts": dict(zip(pipeline.LABEL_CONF_COUNTS, counts.cpu().tolist())),
       "full": {"n": full["n"], "mean_epe": round(full["mean_epe"], 4), "outliers_pct": round(full["outliers_pct"], 3)},
       "margin": curve(margin, True, torch.ones_like(margin, dtype=torch.bool)),
       "oracle": curve(err_true, False, err_true >= 0),
       "consistency": curve(err_fb, False, err_fb >= 0),
       "consistency_formed_fraction": round(float((err_fb >= 0).float().mean()), 4)}
# Spearman-free summary: the mean true error of the pixels in each margin decile, lowest margins first
order = torch.argsort(margin.reshape(-1))
e = err_true.reshape(-1)[order]
ok = e >= 0
res["mean_true_error_by_margin_decile"] = [round(float(c[o].mean()), 4) if o.any() else None
                                           for c, o in zip(torch.chunk(e, 10), torch.chunk(ok, 10))]
print(json.dumps(res))
