"""dflow_pb_edges alone, timed with HIP events on the current stream: python tools/pb_time.py [reps]
Sizes 1024x436 (the bench frame) and 1242x375 (KITTI), dense synthetic first images, radius 3, 5 and 7, both outputs
written (2 launches); dflow_canny_edges on the same frames in the same run for scale.  Prints one JSON line with the median
and the minimum milliseconds per call."""
import ctypes as C, importlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
_lib = importlib.import_module("lk-s-2022-estimacija-pokreta_amd._lib")
synth = importlib.import_module("lk-s-2022-estimacija-pokreta_amd.synth")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L = _lib.lib()
dev = torch.device("cuda", 0)
out = {}


def timed(call):
    for _ in range(5):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


for (H, W) in ((436, 1024), (375, 1242)):
    img = torch.from_numpy(synth.make_pair(H, W, seed=1, style="dense")[0]).to(dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wsb = max(L.dflow_pb_workspace_bytes(H, W), L.dflow_canny_workspace_bytes(H, W))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    e = torch.empty((H, W), dtype=torch.float32, device=dev)
    m = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
    edges = torch.empty((H, W), dtype=torch.uint8, device=dev)
    for radius in (3, 5, 7):
        def call():
            _lib.check(L.dflow_pb_edges(H, W, img.data_ptr(), radius, e.data_ptr(), m.data_ptr(), ws.data_ptr(), wsb, s),
                       "dflow_pb_edges")
        out["%dx%d_pb_r%d" % (W, H, radius)] = dict(timed(call), mean_e=round(float(e.mean().item()), 4))

    def canny():
        _lib.check(L.dflow_canny_edges(H, W, img.data_ptr(), 100.0, 200.0, edges.data_ptr(), e.data_ptr(), ws.data_ptr(), wsb, s),
                   "dflow_canny_edges")
    out["%dx%d_canny" % (W, H)] = timed(canny)
print(json.dumps(out))
