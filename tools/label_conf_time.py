"""dflow_label_confidence and dflow_flow_gate alone, timed with HIP events on the current stream: python tools/label_conf_time.py [reps]
1024x436 (the bench frame), on the state a run_batch synthetic pair leaves after 4 sweeps (label_pitch 160, maxnprop 150).  Both
modes, min_sep 1, with the margin alone and with all four outputs; then the gate of the forward flow by that margin.  Median and
minimum milliseconds of `reps` calls (default 20) after a warm-up call, all in one process, with the bytes the call has to read
at least (the two label planes, 2 * 4 * label_pitch bytes per pixel) and the rate that makes.  Prints one JSON line."""
import ctypes as C
import importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
H, W = 436, 1024
s = _lib.stream(dev)
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
fwd = df.run(img1, img2, 4).clone()
margin = torch.empty((H, W), dtype=torch.float32, device=dev)
alt = torch.empty((H, W), dtype=torch.int32, device=dev)
sparse = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
cnt = torch.empty(6, dtype=torch.int32, device=dev)
gated, cnt2 = torch.empty((H, W, 3), dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)


def timed(call):
    ms = []
    for i in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


def conf(mode, every):
    _lib.call("dflow_label_confidence", C.byref(df.p), df.proposals.data_ptr(), df.lcosts.data_ptr(), df.nprop.data_ptr(),
              df.bestlabels.data_ptr(), mode, 1, 0.0, margin.data_ptr(), alt.data_ptr() if every else None,
              sparse.data_ptr() if every else None, cnt.data_ptr() if every else None, s)


label_bytes = 2 * 4 * df.p.label_pitch * H * W
used_bytes = int(2 * 4 * ((df.nprop.clamp(max=df.p.label_pitch) + 63) // 64 * 64).clamp(max=df.p.label_pitch).sum().item())
res = {"size": "%dx%d" % (W, H), "reps": reps, "label_pitch": df.p.label_pitch, "label_plane_bytes": label_bytes,
       "bytes_of_the_64_slot_steps_read": used_bytes, "mean_nprop": round(float(df.nprop.float().mean()), 2)}
for name, mode in (("local", _lib.CONF_LOCAL), ("data", _lib.CONF_DATA)):
    for every in (False, True):
        r = timed(lambda: conf(mode, every))
        r["GBps_of_label_planes"] = round(label_bytes / r["median_ms"] / 1e6, 1)
        res["%s_%s" % (name, "all_outputs" if every else "margin_only")] = r
    res["%s_counts" % name] = dict(zip(pipeline.LABEL_CONF_COUNTS, cnt.cpu().tolist()))
r = timed(lambda: _lib.call("dflow_flow_gate", H, W, fwd.data_ptr(), _lib.EVAL_DYDX, margin.data_ptr(), 0.0, float("inf"), gated.data_ptr(),
                            cnt2.data_ptr(), s))
r["bytes"] = H * W * (8 + 4 + 12)
r["GBps"] = round(r["bytes"] / r["median_ms"] / 1e6, 1)
res["flow_gate_dydx"] = r
print(json.dumps(res))
