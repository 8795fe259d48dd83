"""dflow_frame_interp alone, timed with HIP events on the current stream: python tools/frame_interp_time.py [reps]
1024x436 (the bench frame), t = 0.5, occl_thresh 30, the source plane and the counts asked for, on the forward and backward flows
of a run_batch synthetic pair (4 sweeps): forward only and two-sided, fill_rounds 0 and 8.  Prints one JSON line with the median
and the minimum milliseconds per call after a warm-up call, the bytes the call has to move at least, and that as GB/s."""
import importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda", 0)
H, W = 436, 1024
N = H * W
s = _lib.stream(dev)
img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
fwd = df.run(img1, img2, 4).clone()
bwd = df.run(img2, img1, 4).clone()
img1, img2 = (torch.from_numpy(a).to(dev) for a in (img1, img2))
out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
keys = torch.empty((H, W), dtype=torch.int64, device=dev)
mot, tmp = (torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
src = torch.empty((H, W), dtype=torch.uint8, device=dev)
cnt = torch.empty(8, dtype=torch.int32, device=dev)


def least_bytes(sides, rounds):
    """What must move when every plane is read and written once per launch that needs it, every gather a hit in its own line:
    memset of the keys 8; claim: flow 8 and own pixel 3 per side, four corners of the other frame counted once as 3, the key
    atomic 8; resolve: key 8, winner's vector 8, motion out 12; a fill round 12 + 12; render: motion 12, key 8, both frames 3 + 3,
    frame out 3, source out 1."""
    per_pixel = 8 + sides * (8 + 3 + 3 + 8) + (8 + 8 + 12) + rounds * 24 + (12 + 8 + 6 + 3 + 1)
    return N * per_pixel


res = {"size": "%dx%d" % (W, H), "reps": reps, "flow_layout": "dydx", "launches": "3 + fill_rounds, and two memsets"}
for sides, back in ((1, None), (2, bwd)):
    for rounds in (0, 8):
        ms = []
        for i in range(1 + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.call("dflow_frame_interp", H, W, img1.data_ptr(), img2.data_ptr(), fwd.data_ptr(), _lib.EVAL_DYDX,
                      None if back is None else back.data_ptr(), _lib.EVAL_DYDX, 0.5, rounds, 30.0, 0, out.data_ptr(), keys.data_ptr(),
                      mot.data_ptr(), tmp.data_ptr(), src.data_ptr(), cnt.data_ptr(), s)
            b.record()
            torch.cuda.synchronize()
            if i >= 1:
                ms.append(a.elapsed_time(b))
        ms.sort()
        nbytes = least_bytes(sides, rounds)
        res["%s_fill%d" % ("forward_only" if sides == 1 else "two_sided", rounds)] = {
            "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "least_bytes": nbytes,
            "gb_per_s_at_median": round(nbytes / (ms[len(ms) // 2] * 1e-3) / 1e9, 1), "counts": cnt.cpu().tolist()}
print(json.dumps(res))
