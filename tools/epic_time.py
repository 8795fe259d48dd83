"""dflow_epic_interpolate alone, per-stage HIP-event times and Voronoi rounds: python tools/epic_time.py [reps]
Sizes 1024x436 (the bench frame) and 1242x375 (KITTI).  Seeds: the forward/backward consistency output of a synthetic pass
(what the reference feeds EpicFlow: every valid pixel), and its 1-in-16 grid subsample; edges: the Canny ivice map of the
first image, as spremiZaEpic.py writes it.  LA, nn=100, k=0.8.  Prints one JSON line: median and minimum ms per call
(host wall time, the call synchronises) and the median of each stage.  For the consistency output also the match pre-filter
(dflow_epic_prefilter, its defaults, with the first image): its time and stages, the share of seeds each stage drops, and the
interpolation again on the filtered seeds."""
import importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
pipeline = importlib.import_module("lk-s-2022-estimacija-pokreta_amd.pipeline")
synth = importlib.import_module("lk-s-2022-estimacija-pokreta_amd.synth")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
out = {}
for (H, W) in ((436, 1024), (375, 1242)):
    img1, img2, _ = synth.make_pair(H, W, seed=1)
    flows = []
    for a, b in ((img1, img2), (img2, img1)):
        df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
        flows.append(df.run(a, b, 4).clone())
    sparse = pipeline.fb_consistency(flows[0], flows[1], 10)           # con_tresh of the reference README.md:65
    _, ivice = pipeline.canny_edges(img1)
    sub = torch.zeros_like(sparse)
    sub[::4, ::4] = sparse[::4, ::4]
    dimg1 = torch.from_numpy(img1).to(dev)

    def timed(call, stats):
        """median and minimum wall ms of call(), the last first value of stats() and the median of its stage times"""
        for _ in range(3):
            call()
        wall, stages, first = [], [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            first, ms = stats()
            stages.append(ms)
        wall.sort()
        return first, {"median_ms": round(wall[len(wall) // 2], 3), "min_ms": round(wall[0], 3),
                       "stage_median_ms": {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]}}

    def interpolation(sp):
        rounds, res = timed(lambda: pipeline.epic_interpolate(sp, ivice), pipeline.epic_last_stats)
        return dict(seeds_pct=round(100.0 * float((sp[..., 2] > 0.5).float().mean()), 1), rounds=rounds, **res)
    for name, sp in (("consistency", sparse), ("grid16", sub)):
        out["%dx%d_%s" % (W, H, name)] = interpolation(sp)
    counts, res = timed(lambda: pipeline.epic_prefilter(sparse, ivice, dimg1), pipeline.epic_prefilter_last_stats)
    out["%dx%d_prefilter" % (W, H)] = dict(
        dropped_saliency_pct=round(100.0 * counts["dropped_saliency"] / max(1, counts["seeds"]), 2),
        dropped_consistency_pct=round(100.0 * counts["dropped_consistency"] / max(1, counts["seeds"]), 2), **counts, **res)
    out["%dx%d_consistency_filtered" % (W, H)] = interpolation(pipeline.epic_prefilter(sparse, ivice, dimg1))
print(json.dumps(out))
