"""dflow_klt_pyramid, dflow_corners and dflow_klt_track alone, timed with HIP events on the current stream:
python tools/klt_time.py [reps]
1024x436 (the bench frame), on a run_batch synthetic pair; 3 levels, r 7, 20 iterations, eps 0.01, min_eig 1, fb 0.5 and, next to
it, fb 0 (the forward pass alone).  The track call on three sets: the corners of the first image (rc 2, min_dist 4, quality
0.01), grid seeds at step 2 (111 616 tracks) and at step 1 (446 464 tracks).  Median and minimum milliseconds of `reps` calls
(default 20) after a warm-up call; a call is timed in a window of `batch` back-to-back calls so that the window is not a single
short launch.  Next to each track time the counts the call returned.  A third run per set has eps 1e-30, min_eig 0 and fb 0, so
that every iteration of every level runs and the window samples can be counted: its time over the instruction bound of the sample loop (95 instructions per
sample in the gfx950 code of klt_track_kernel's iteration loop, address arithmetic and loads included) is the kernel's ratio to
that bound.  Prints one JSON line."""
import importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
H, W, LEVELS, R, ITERS = 436, 1024, 3, 7, 20
SAMPLE_INSTRUCTIONS = 95
s = _lib.stream(dev)
img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
d1, d2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
nbytes = pipeline.klt_pyramid_len(H, W, LEVELS)
pyr1, pyr2 = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
resp = torch.empty((H, W), dtype=torch.float32, device=dev)
mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
rmax = torch.empty(1, dtype=torch.int32, device=dev)
ccnt = torch.empty(4, dtype=torch.int32, device=dev)


def timed(call, batch):
    ms = []
    for i in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            call()
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b) / batch)
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "batch": batch}


def pyramid(img, pyr):
    _lib.call("dflow_klt_pyramid", H, W, LEVELS, img.data_ptr(), pyr.data_ptr(), s)


def corners():
    _lib.call("dflow_corners", H, W, pyr1.data_ptr(), 2, 4, 4, 0.01, 0.0, 0, None, None, None, resp.data_ptr(), mask.data_ptr(), None,
              rmax.data_ptr(), ccnt.data_ptr(), s)


pyramid(d1, pyr1)
pyramid(d2, pyr2)
res = {"size": "%dx%d" % (W, H), "reps": reps, "levels": LEVELS, "r": R, "iters": ITERS,
       "pyramid": timed(lambda: pyramid(d1, pyr1), 20), "corners": timed(corners, 20)}
res["corners"]["counts"] = ccnt.cpu().tolist()


def track_set(step):
    """The set: the corners (step None) or a grid."""
    if step is None:
        ts = pipeline.TrackSet(H, W, cap=H * W // 16, step=1, device=dev)
        ts.seed(mask)
    else:
        ts = pipeline.TrackSet(H, W, cap=-(-H // step) * -(-W // step), step=step, device=dev)
        ts.seed()
    n = int(ts.n.cpu()[0])
    return ts.pos[:n].clone(), ts.state[:n].clone()


for name, step in (("corner_set", None), ("grid_step2", 2), ("grid_step1", 1)):
    pos, state = track_set(step)
    cap = pos.shape[0]
    pos_out, state_out = torch.empty_like(pos), torch.empty_like(state)
    cnt = torch.empty(8, dtype=torch.int32, device=dev)
    entry = {"tracks": cap}
    for key, fb, eps, min_eig in (("fb_0.5", 0.5, 0.01, 1.0), ("fb_0", 0.0, 0.01, 1.0), ("every_iteration", 0.0, 1e-30, 0.0)):
        def track():
            _lib.call("dflow_klt_track", H, W, LEVELS, pyr1.data_ptr(), pyr2.data_ptr(), cap, pos.data_ptr(), state.data_ptr(), R, ITERS, eps,
                      min_eig, 0.0, fb, 0, pos_out.data_ptr(), state_out.data_ptr(), None, None, cnt.data_ptr(), s)
        t = timed(track, 20 if cap < 50000 else 2)
        t["counts"] = cnt.cpu().tolist()
        t["tracks_per_ms"] = round(cap / t["median_ms"], 1)
        if key == "every_iteration":
            # no step is below eps and no level is flat: a track that ends live has sampled iters windows at every level, the
            # template and the residual once.  The bound: SAMPLE_INSTRUCTIONS wave instructions per 64 samples, one per 2 cycles
            # and SIMD, 1024 SIMDs at 2.4 GHz.
            samples = t["counts"][0] * (LEVELS * ((2 * R + 3) ** 2 + ITERS * (2 * R + 1) ** 2) + (2 * R + 1) ** 2)
            bound_ms = samples / 64 * SAMPLE_INSTRUCTIONS * 2 / (1024 * 2.4e9) * 1e3
            t.update(samples=samples, bound_ms=round(bound_ms, 4), time_over_bound=round(t["median_ms"] / bound_ms, 2))
        entry[key] = t
    res[name] = entry
print(json.dumps(res))
