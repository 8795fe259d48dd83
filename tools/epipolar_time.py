"""dflow_epipolar_fit alone, timed with HIP events on the current stream: python tools/epipolar_time.py [reps]
1024x436 (the bench frame), on a planted rigid scene (synth.rigid_flow: translation + rotation, a rectangle that moves on its own,
0.1 px noise, every pixel good).  For n_hyp 256, 1024 and 4096: the whole call with the defaults of pipeline.epipolar_fit (one
local round, every pixel scored); the search alone (lo_rounds 0) with every pixel scored and with step 64, which scores 1/4096 of
them and launches the same kernels: the difference of the two is the time of ep_score_kernel.  Next to them dflow_motion_fit's
homography on the same field at the same n_hyp, the same three ways (polish does not apply to it).  Median and minimum
milliseconds of `reps` calls (default 20) after a warm-up call.  The VALU bound of the score kernel is counted as DESIGN 5.17
counts it: vector instructions per pixel of the inner loop's disassembly (159 per 8 pixels) x live slots x scored pixels / 64
lanes / (1024 SIMDs x 2.4 GHz / 4 cycles per wave instruction).  Then the quality run: the three planted motions at 1024x436
(the share of static and of moving pixels in class 1, the distance of the focus of expansion from the planted one) and, as a
negative control, the forward flow of the two bench pairs, which obey no epipolar geometry.  Prints one JSON line."""
import importlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
H, W = 436, 1024
VALU_PER_PIXEL = 159 / 8.0
WAVE_INSTRUCTIONS_PER_S = 1024 * 2.4e9 / 4
s = _lib.stream(dev)
MOTIONS = {"sideways": ((0.4, 0.0, 0.0), (0.0, 0.0, 0.0)), "forward": ((0.0, 0.0, 0.9), (0.0, 0.0, 0.0)),
           "mixed": ((0.3, -0.1, 0.6), (0.004, -0.006, 0.003))}
RECT = (H // 4, W // 2, H // 4 + H // 3, W // 2 + W // 4, 3.0, -4.0)


def planted(name, seed=0):
    f, mask = synth.rigid_flow(H, W, seed, MOTIONS[name][0], MOTIONS[name][1], objects=(RECT,))
    f[..., :2] += 0.1 * np.random.default_rng(seed + 1).standard_normal((H, W, 2))
    return torch.from_numpy(f.astype(np.float32)).to(dev), torch.from_numpy(mask).to(dev)


field, _ = planted("mixed")
model = torch.empty(9, dtype=torch.float32, device=dev)
state = torch.empty(32, dtype=torch.int64, device=dev)
cnt = torch.empty(8, dtype=torch.int32, device=dev)


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
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "counts": cnt.cpu().tolist()}


def epipolar(n_hyp, lo_rounds, step):
    models = torch.empty(3 * n_hyp * 9, dtype=torch.float32, device=dev)
    hyp_counts = torch.empty(3 * n_hyp, dtype=torch.int32, device=dev)
    return timed(lambda: _lib.call("dflow_epipolar_fit", H, W, field.data_ptr(), _lib.EVAL_UVV, None, 1.0, n_hyp, lo_rounds, step, 0, 0,
                                   model.data_ptr(), models.data_ptr(), hyp_counts.data_ptr(), state.data_ptr(), None, None,
                                   cnt.data_ptr(), s))


def homography(n_hyp, lo_rounds, step):
    models = torch.empty(n_hyp * 9, dtype=torch.float32, device=dev)
    hyp_counts = torch.empty(n_hyp, dtype=torch.int32, device=dev)
    return timed(lambda: _lib.call("dflow_motion_fit", H, W, field.data_ptr(), _lib.EVAL_UVV, None, _lib.MOTION_HOMOGRAPHY, 1.0, n_hyp,
                                   lo_rounds, 0, step, 0, 0, model.data_ptr(), models.data_ptr(), hyp_counts.data_ptr(), state.data_ptr(),
                                   None, None, None, cnt.data_ptr(), s))


res = {"size": "%dx%d" % (W, H), "reps": reps}
for n_hyp in (256, 1024, 4096):
    for name, fn in (("epipolar", epipolar), ("homography", homography)):
        whole, search, sparse = fn(n_hyp, 1, 1), fn(n_hyp, 0, 1), fn(n_hyp, 0, 64)
        row = {"whole_call": whole, "search_step1": search, "search_step64": sparse,
               "score_kernel_ms": round(search["median_ms"] - sparse["median_ms"], 4)}
        if name == "epipolar":
            live = 3 * n_hyp - search["counts"][2]                    # lo_rounds 0: the degenerate slots are round 0's
            row["slots"], row["live_slots"], row["pairs_live"] = 3 * n_hyp, live, live * H * W
            row["valu_bound_ms"] = round(VALU_PER_PIXEL * live * H * W / 64 / WAVE_INSTRUCTIONS_PER_S * 1e3, 4)
        res["%s_%d" % (name, n_hyp)] = row

quality = []
for name in MOTIONS:
    f, mask = planted(name)
    for thresh in (0.5, 1.0):
        m, cls, r, c = pipeline.epipolar_fit(f, thresh=thresh, classes=True, residual=True, counts=True)
        c = c.cpu().tolist()
        geo = pipeline.epipolar_geometry(m.cpu().numpy(), H, W)
        hm, hcls, hc = pipeline.motion_fit(f, model="homography", thresh=thresh, classes=True, counts=True)
        quality.append({"scene": name, "thresh": thresh, "static_in_class1": round(float((cls[~mask] == 1).float().mean()), 4),
                        "moving_in_class1": round(float((cls[mask] == 1).float().mean()), 4),
                        "median_residual_static": round(float(r[~mask].median()), 4), "median_residual_moving": round(float(r[mask].median()), 4),
                        "foe": geo["foe"], "planted_foe": [(W - 1) * 0.5, (H - 1) * 0.5] if name == "forward" else None, "counts": c,
                        "homography_static_in_class1": round(float((hcls[~mask] == 1).float().mean()), 4)})
res["planted"] = quality

df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
control = []
for pair in (0, 1):
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(pair, 0))
    fwd = df.run(img1, img2, 4).clone()
    for thresh in (1.0, 3.0):
        m, r, c = pipeline.epipolar_fit(fwd, thresh=thresh, residual=True, counts=True)
        c = c.cpu().tolist()
        control.append({"pair": pair, "thresh": thresh, "inlier_fraction": round(c[1] / max(c[0], 1), 4),
                        "median_residual": round(float(r.median()), 3), "counts": c})
res["bench_pairs"] = control
print(json.dumps(res))
