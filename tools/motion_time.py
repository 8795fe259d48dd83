"""dflow_motion_fit alone, timed with HIP events on the current stream: python tools/motion_time.py [reps]
1024x436 (the bench frame), on the forward flow of a run_batch synthetic pair (4 sweeps, [dy,dx], every pixel good).  For n_hyp
256, 1024 and 4096 and both models: the whole call with the defaults of pipeline.motion_fit (one local round, two polish steps,
every pixel scored); the search alone (lo_rounds 0, polish 0) with every pixel scored and with step 64, which scores 1/4096 of
them and launches the same kernels: the difference of the two is the time of the score kernel.  Median and minimum milliseconds
of `reps` calls (default 20) after a warm-up call.  Next to them the host round trip the call replaces: the flow copied to the
host and the numpy restatement's own fit (tests/motion_ref.py) at 256 hypotheses, timed once.  Then the quality run on the two
bench pairs: the inlier fraction of an affine and of a homography fit at thresh 1 and 3 and the mean |residual| inside and
outside class 1.  Prints one JSON line."""
import importlib, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
import motion_ref
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
H, W = 436, 1024
s = _lib.stream(dev)
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
fwds = []
for pair in (0, 1):
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(pair, 0))
    fwds.append(df.run(img1, img2, 4).clone())
fwd = fwds[0]
model = torch.empty(9, dtype=torch.float32, device=dev)
state = torch.empty(32, dtype=torch.int64, device=dev)
cnt = torch.empty(8, dtype=torch.int32, device=dev)


def timed(kind, n_hyp, lo_rounds, polish, step):
    models = torch.empty(n_hyp * 9, dtype=torch.float32, device=dev)
    hyp_counts = torch.empty(n_hyp, dtype=torch.int32, device=dev)
    ms = []
    for i in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("dflow_motion_fit", H, W, fwd.data_ptr(), _lib.EVAL_DYDX, None, kind, 1.0, n_hyp, lo_rounds, polish, step, 0, 0,
                  model.data_ptr(), models.data_ptr(), hyp_counts.data_ptr(), state.data_ptr(), None, None, None, cnt.data_ptr(), s)
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "counts": cnt.cpu().tolist()}


res = {"size": "%dx%d" % (W, H), "reps": reps, "pairs_per_call": {}}
for name, kind in (("affine", _lib.MOTION_AFFINE), ("homography", _lib.MOTION_HOMOGRAPHY)):
    for n_hyp in (256, 1024, 4096):
        whole = timed(kind, n_hyp, 1, 2, 1)
        search, sparse = timed(kind, n_hyp, 0, 0, 1), timed(kind, n_hyp, 0, 0, 64)
        res["%s_%d" % (name, n_hyp)] = {"whole_call": whole, "search_step1": search, "search_step64": sparse,
                                        "score_kernel_ms": round(search["median_ms"] - sparse["median_ms"], 4)}
        res["pairs_per_call"][str(n_hyp)] = n_hyp * H * W

# the host round trip: the copy, then the restatement's fit
torch.cuda.synchronize()
t0 = time.perf_counter()
host = fwd.cpu().numpy()
t1 = time.perf_counter()
got = motion_ref.fit(host, motion_ref.AFFINE, n_hyp=256, lo_rounds=1, polish=2)
t2 = time.perf_counter()
res["host_round_trip"] = {"copy_ms": round((t1 - t0) * 1e3, 3), "numpy_fit_256_ms": round((t2 - t1) * 1e3, 1), "counts": got["counts"]}

quality = []
for pair, f in enumerate(fwds):
    for name in ("affine", "homography"):
        for thresh in (1.0, 3.0):
            m, cls, r, c = pipeline.motion_fit(f, model=name, thresh=thresh, classes=True, residual=True, counts=True)
            c = c.cpu().tolist()
            mag = torch.sqrt(r[..., 0] ** 2 + r[..., 1] ** 2)
            inside, outside = cls == 1, cls == 2
            quality.append({"pair": pair, "model": name, "thresh": thresh, "inlier_fraction": round(c[1] / max(c[0], 1), 4),
                            "mean_residual_inside": round(float(mag[inside].mean()), 3) if inside.any() else None,
                            "mean_residual_outside": round(float(mag[outside].mean()), 3) if outside.any() else None,
                            "matrix": [round(float(v), 6) for v in m.reshape(-1).cpu().tolist()]})
res["quality"] = quality
print(json.dumps(res))
