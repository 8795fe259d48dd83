"""dflow_flow_eval alone, timed with HIP events on the current stream: python tools/eval_time.py [reps]
1024x436 (the bench frame): a dense [dy,dx] flow of small integers against a smooth true flow, statistics only and with
both optional outputs (error plane and picture), 2 launches per call; next to it today's host path on the same field, the
wall time of .cpu() of the field plus evaluate.error_metrics.  Prints one JSON line with the median and the minimum
milliseconds per call."""
import importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, evaluate, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "evaluate", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L = _lib.lib()
dev = torch.device("cuda", 0)
H, W = 436, 1024
gt_host = evaluate.to_uv_valid(synth.forward_gt(H, W, seed=1))
gt = torch.from_numpy(gt_host).to(dev)
flow = torch.from_numpy(np.rint(synth.forward_gt(H, W, seed=1) + np.random.default_rng(1).normal(0, 1.5, (H, W, 2))).astype(np.float32)).to(dev)
s = _lib.stream(dev)
wsb = L.dflow_eval_workspace_bytes(H, W)
ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
stats = torch.zeros(8, dtype=torch.int64, device=dev)
err = torch.empty((H, W), dtype=torch.float32, device=dev)
img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


def timed(call):
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    return spread(a.elapsed_time(b) for a, b in ev)


def gpu(e, i):
    return lambda: _lib.check(L.dflow_flow_eval(H, W, flow.data_ptr(), _lib.EVAL_DYDX, gt.data_ptr(), 3.0, 0, stats.data_ptr(), e, i,
                                                ws.data_ptr(), wsb, s), "dflow_flow_eval")


out = {"size": "%dx%d" % (W, H), "reps": reps,
       "bytes_stats_only": H * W * 20, "bytes_both_outputs": H * W * 27,
       "gpu_stats_only": timed(gpu(None, None)), "gpu_both_outputs": timed(gpu(err.data_ptr(), img.data_ptr()))}
st = pipeline.eval_stats(stats)
host = []
for _ in range(5 + reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = evaluate.error_metrics(evaluate.to_uv_valid(flow.cpu().numpy()), gt_host)
    host.append((time.perf_counter() - t0) * 1e3)
out["host_cpu_copy_plus_error_metrics"] = spread(host[5:])
out["mean_epe_gpu"], out["mean_epe_host"], out["n"] = st["mean_epe"], m[0], st["n"]
assert (m[2], m[1]) == (st["n"], st["outliers_pct"])
print(json.dumps(out))
