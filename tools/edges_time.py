"""dflow_canny_edges alone, timed with HIP events on the current stream: python tools/edges_time.py [reps]
Sizes 1242x375 (KITTI) and 1024x436 (the bench frame), dense and low_texture synthetic first images; prints one JSON line
with the median and the minimum milliseconds per call (4 launches, edges + ivice written)."""
import ctypes as C, importlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
_lib = importlib.import_module("lk-s-2022-estimacija-pokreta_amd._lib")
synth = importlib.import_module("lk-s-2022-estimacija-pokreta_amd.synth")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
L = _lib.lib()
dev = torch.device("cuda", 0)
out = {}
for (H, W) in ((375, 1242), (436, 1024)):
    for style in ("dense", "low_texture"):
        img = torch.from_numpy(synth.make_pair(H, W, seed=1, style=style)[0]).to(dev)
        wsb = L.dflow_canny_workspace_bytes(H, W)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        e = torch.empty((H, W), dtype=torch.uint8, device=dev)
        iv = torch.empty((H, W), dtype=torch.float32, device=dev)
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def call():
            _lib.check(L.dflow_canny_edges(H, W, img.data_ptr(), 100.0, 200.0, e.data_ptr(), iv.data_ptr(), ws.data_ptr(), wsb, s),
                       "dflow_canny_edges")
        for _ in range(5):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(); call(); b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        out["%dx%d_%s" % (W, H, style)] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4),
                                           "edge_px": int((e > 0).sum().item())}
print(json.dumps(out))
