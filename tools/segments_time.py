"""dflow_segment_filter alone, timed with HIP events on the current stream: python tools/segments_time.py [reps]
1024x436 (the bench frame), T = 1, MIN = 100, all four outputs, on three fields: "checked", the forward field of a run_batch
synthetic pair after the forward/backward check in image coordinates at 10 px; "one_segment", one vector over the whole frame;
"serpentine", one segment that snakes through every row (the longest chains of labels a frame of this size can hold).  Next to
each, alternating with it, what the host function offers for the same field: the wall time of .cpu() +
compat.remove_small_segments + the upload.  Prints one JSON line with the median and the minimum milliseconds per call."""
import importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, compat, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "compat", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L = _lib.lib()
dev = torch.device("cuda", 0)
H, W = 436, 1024
T, MIN = 1.0, 100
s = _lib.stream(dev)
wsb = L.dflow_segment_filter_workspace_bytes(H, W)
ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
seg, size = (torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(2))
cnt = torch.empty(4, dtype=torch.int32, device=dev)


def checked():
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
    df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
    fwd = df.run(img1, img2, 4).clone()
    bwd = df.run(img2, img1, 4).clone()
    return pipeline.flow_consistency(fwd, bwd, 10.0)


def one_segment():
    f = torch.ones((H, W, 3), dtype=torch.float32, device=dev)
    f[..., 0] = 3.0
    return f


def serpentine():
    f = one_segment()
    f[1::2, :, 2] = 0.0
    f[1::4, W - 1, 2] = 1.0
    f[3::4, 0, 2] = 1.0
    return f


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


def both(field):
    """The device call (HIP events) and the host path (wall time), one after the other `reps` times after 3 warm-up rounds."""
    gpu, host = [], []
    for i in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("dflow_segment_filter", H, W, field.data_ptr(), _lib.EVAL_UVV, T, MIN, 0, out.data_ptr(), seg.data_ptr(), size.data_ptr(),
                  cnt.data_ptr(), ws.data_ptr(), wsb, s)
        b.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = torch.from_numpy(compat.remove_small_segments(field.cpu().numpy(), T, MIN)).to(dev)
        torch.cuda.synchronize()
        if i >= 3:
            gpu.append(a.elapsed_time(b))
            host.append((time.perf_counter() - t0) * 1e3)
    c = cnt.cpu().tolist()
    return {"gpu": spread(gpu), "host_copy_fill_upload": spread(host), "counts": c,
            "valid_after_gpu": int(out[..., 2].sum().item()), "valid_after_host": int(back[..., 2].sum().item())}


res = {"size": "%dx%d" % (W, H), "reps": reps, "thresh": T, "min_size": MIN}
for name, make in (("checked", checked), ("one_segment", one_segment), ("serpentine", serpentine)):
    res[name] = both(make().contiguous())
print(json.dumps(res))
