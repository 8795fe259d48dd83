"""dflow_flow_color and dflow_warp_eval alone, timed with HIP events on the current stream: python tools/flowpic_time.py [reps]
1024x436 (the bench frame): the synthetic pair of the bench and its true flow plus noise as a dense [dy,dx] field.  Prints one
JSON line with the median and the minimum milliseconds per call and the bytes each call has to move (flow read, images read,
planes written; the gathered reads of the second image counted once per pixel and channel tap)."""
import importlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L = _lib.lib()
dev = torch.device("cuda", 0)
H, W = 436, 1024
N = H * W
img1, img2, gt = synth.make_pair(H, W, seed=1)
flow = torch.from_numpy((gt + np.random.default_rng(1).normal(0, 1.5, (H, W, 2))).astype(np.float32)).to(dev)
i1, i2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
s = _lib.stream(dev)
wsb_c, wsb_w = L.dflow_flow_color_workspace_bytes(H, W), L.dflow_warp_eval_workspace_bytes(H, W)
ws = torch.empty(max(wsb_c, wsb_w), dtype=torch.uint8, device=dev)
stats = torch.zeros(6, dtype=torch.int64, device=dev)
err = torch.empty((H, W), dtype=torch.float32, device=dev)
pic, warped = (torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2))


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


def color(max_flow):
    return lambda: _lib.check(L.dflow_flow_color(H, W, flow.data_ptr(), _lib.EVAL_DYDX, max_flow, pic.data_ptr(), None, ws.data_ptr(),
                                                 wsb_c, s), "dflow_flow_color")


def warp(w, e, p):
    return lambda: _lib.check(L.dflow_warp_eval(H, W, i1.data_ptr(), i2.data_ptr(), flow.data_ptr(), _lib.EVAL_DYDX, 10.0, 30.0, 0,
                                                stats.data_ptr(), w, e, p, ws.data_ptr(), wsb_w, s), "dflow_warp_eval")


print(json.dumps({"size": "%dx%d" % (W, H), "reps": reps,
                  "color_fixed_radius": dict(timed(color(40.0)), launches=1, bytes=N * (8 + 3)),
                  "color_auto_radius": dict(timed(color(0.0)), launches=3, bytes=N * (8 + 8 + 3)),
                  "warp_stats_only": dict(timed(warp(None, None, None)), launches=2, bytes=N * (8 + 3 + 12)),
                  "warp_all_outputs": dict(timed(warp(warped.data_ptr(), err.data_ptr(), pic.data_ptr())), launches=2,
                                           bytes=N * (8 + 3 + 12 + 3 + 4 + 3))}))
