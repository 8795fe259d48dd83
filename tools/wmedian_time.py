"""dflow_flow_wmedian alone, timed with HIP events on the current stream: python tools/wmedian_time.py [reps]
1024x436 (the bench frame), radius 1, 3, 5 and 8, guided (the first image, sigma_color 10, no space table) and unguided, on the
forward flow of a run_batch synthetic pair (4 sweeps, [dy,dx], every pixel good) and on the output of the natural
forward/backward check at 2 px ([U,V,valid], with holes).  Prints one JSON line with the median and the minimum milliseconds of
`reps` calls (default 20) after a warm-up call, and the four counts of each case."""
import importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
H, W = 436, 1024
s = _lib.stream(dev)
img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
fwd = df.run(img1, img2, 4).clone()
bwd = df.run(img2, img1, 4).clone()
checked = pipeline.flow_consistency(fwd, bwd, 2.0)
img = torch.from_numpy(img1).to(dev)
color = torch.from_numpy(pipeline.wmedian_tables(3, None, 10.0)[1]).to(dev)
out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
cnt = torch.empty(4, dtype=torch.int32, device=dev)

res = {"size": "%dx%d" % (W, H), "reps": reps, "launches": "1, and the memset of the counts"}
for fname, field, layout in (("bcd_forward", fwd, _lib.EVAL_DYDX), ("checked", checked, _lib.EVAL_UVV)):
    for guided in (False, True):
        for radius in (1, 3, 5, 8):
            ms = []
            for i in range(1 + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.call("dflow_flow_wmedian", H, W, field.data_ptr(), layout, img.data_ptr() if guided else None, radius, None,
                          color.data_ptr() if guided else None, 0.0, 0, out.data_ptr(), cnt.data_ptr(), s)
                b.record()
                torch.cuda.synchronize()
                if i >= 1:
                    ms.append(a.elapsed_time(b))
            ms.sort()
            res["%s_%s_r%d" % (fname, "guided" if guided else "unguided", radius)] = {
                "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "counts": cnt.cpu().tolist()}
print(json.dumps(res))
