"""The two-view reconstruction, measured: python tools/two_view_time.py [reps].  Times: dflow_two_view on
preallocated planes, HIP events around the C call, median of `reps` (default 20) after a warm-up, at 1024x436 (the bench frame)
and at 4096x2048, for step 1, 2, 4 and 64, with every output and with the pose alone; the call at step 1 minus the call at step
64 is the vote kernel over every pixel (at step 64 it has a handful of lanes), which is set against its float64 issue bound.
And dflow_epipolar_fit followed by dflow_two_view, the chain twoview.py runs.  Quality, on synth.rigid_flow's scene with
rigid_depth as the truth, a rectangle that moves against the epipolar direction, Gaussian noise of 0, 0.1 and 0.5 px on every
vector: the rotation error, the translation error, the relative depth error over the pixels of class 1 outside the rectangle,
and how much of the rectangle is class 2.  Prints JSON lines, the last one everything."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
pipeline, synth, L = (importlib.import_module(PKG + "." + m) for m in ("pipeline", "synth", "_lib"))

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", torch.cuda.current_device())
s = L.stream(dev)
out = {"reps": reps}
T_TRUE, ROT_TRUE = (0.3, -0.1, 0.6), (0.004, -0.006, 0.003)
# float64 VALU instructions of tv_vote_kernel per voting pixel in the gfx950 disassembly, 4 cycles each per wave
VOTE_F64_INSTRUCTIONS = 155


def timed(fn):
    fn()                                                  # warm-up: code objects
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4)}


def rotation(rot):
    rx, ry, rz = rot
    th = float(np.sqrt(rx * rx + ry * ry + rz * rz))
    K = np.array([[0.0, -rz, ry], [rz, 0.0, -rx], [-ry, rx, 0.0]])
    return np.eye(3) if th == 0.0 else np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


# ---- times
for H, W in ((436, 1024), (2048, 4096)):
    flow = torch.from_numpy(synth.rigid_flow(H, W, 0, T_TRUE, ROT_TRUE)[0].astype(np.float32)).to(dev)
    n_hyp = 512
    model, models = torch.empty(9, device=dev), torch.empty(3 * n_hyp * 9, device=dev)
    hc, st = torch.empty(3 * n_hyp, dtype=torch.int32, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    fit_cls = torch.empty((H, W), dtype=torch.uint8, device=dev)
    pose, st2 = torch.empty(16, dtype=torch.float64, device=dev), torch.empty(32, dtype=torch.int64, device=dev)
    depth, err = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
    cls, cnt = torch.empty((H, W), dtype=torch.uint8, device=dev), torch.empty(8, dtype=torch.int32, device=dev)

    def fit():
        L.call("dflow_epipolar_fit", H, W, flow.data_ptr(), L.EVAL_UVV, None, 1.0, n_hyp, 1, 4, 0, 0, model.data_ptr(), models.data_ptr(),
               hc.data_ptr(), st.data_ptr(), fit_cls.data_ptr(), None, None, s)

    def view(step, outputs=True, part=True):
        o = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
        L.call("dflow_two_view", H, W, flow.data_ptr(), L.EVAL_UVV, model.data_ptr(), fit_cls.data_ptr() if part else None, float(max(H, W)),
               float(max(H, W)), (W - 1) * 0.5, (H - 1) * 0.5, step, 0, pose.data_ptr(), st2.data_ptr(), o(depth), o(cls), o(err), o(cnt), s)
    fit()
    res = {}
    for step in (1, 2, 4, 64):
        res["step %d, every output" % step] = timed(lambda: view(step))
        res["step %d, the pose alone" % step] = timed(lambda: view(step, outputs=False))
    res["fit (512 samples, step 4) then two_view (step 1)"] = timed(lambda: (fit(), view(1)))
    view(1)
    res["counts"] = dict(zip(pipeline.TWO_VIEW_COUNTS[:7], cnt.cpu().tolist()))
    vote_ms = res["step 1, the pose alone"]["median_ms"] - res["step 64, the pose alone"]["median_ms"]
    res["vote kernel over every pixel, by difference, ms"] = round(vote_ms, 4)
    if VOTE_F64_INSTRUCTIONS:
        # a wave64 float64 instruction issues in 4 cycles on one of 4 SIMDs of 256 CUs at 2.4 GHz
        bound_ms = (H * W / 64.0) * VOTE_F64_INSTRUCTIONS * 4 / (256 * 4 * 2.4e9) * 1e3
        res["vote kernel's float64 issue bound, ms"] = round(bound_ms, 4)
    out["%dx%d" % (W, H)] = res
    print("times", "%dx%d" % (W, H), json.dumps(res), flush=True)

# ---- quality
H, W = 436, 1024
Z, K = synth.rigid_depth(H, W, 0)
box = (H // 4, W // 2, H // 4 + H // 3, W // 2 + W // 4)
SIDEWAYS = (0.1, 0.0, 0.0)
res = {}
for name, t_true, rot_true, objects in (("moving camera", T_TRUE, ROT_TRUE, ()), ("sideways, a rectangle against it", SIDEWAYS, (0.0, 0.0, 0.0),
                                                                                (box + (-30.0, 0.0),))):
    R_true, t_len = rotation(rot_true), float(np.linalg.norm(t_true))
    for noise in (0.0, 0.1, 0.5):
        f, mask = synth.rigid_flow(H, W, 0, t_true, rot_true, objects=objects)
        f[..., :2] += noise * np.random.RandomState(7).standard_normal((H, W, 2))
        flow = torch.from_numpy(f.astype(np.float32)).to(dev)
        m, fit_cls, fit_cnt = pipeline.epipolar_fit(flow, thresh=max(1.0, 3 * noise), n_hyp=512, step=4, classes=True, counts=True)
        pose, depth, cls, err, cnt = pipeline.two_view(flow, m, part=fit_cls, depth=True, classes=True, err=True, counts=True)
        info = pipeline.two_view_pose(pose.cpu().numpy())
        depth, cls, err, fit_cls = depth.cpu().numpy(), cls.cpu().numpy(), err.cpu().numpy(), fit_cls.cpu().numpy()
        D = info["R"] @ R_true.T
        sk = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
        ok = (cls == 1) & ~mask
        rel = np.abs(depth[ok].astype(np.float64) * t_len / Z[ok] - 1.0) if ok.any() else np.array([np.nan])
        row = {"fit_inliers_of_scored": fit_cnt.cpu().tolist()[:2][::-1], "candidate": info["candidate"],
               "rotation_error_deg": float(np.degrees(np.arctan2(sk, 0.5 * (np.trace(D) - 1.0)))),
               "translation_error": float(np.linalg.norm(info["t"] - np.array(t_true) / t_len)),
               "depth_rel_error_median": float(np.median(rel)), "depth_rel_error_p95": float(np.percentile(rel, 95)),
               "reprojection_px_median": float(np.median(err[ok])) if ok.any() else None,
               "class2_pct_outside": round(100.0 * float((cls[~mask] == 2).mean()), 3),
               "counts": dict(zip(pipeline.TWO_VIEW_COUNTS[:7], cnt.cpu().tolist()))}
        if objects:
            row["class2_pct_in_rectangle"] = round(100.0 * float((cls[mask] == 2).mean()), 2)
            row["fit_outlier_pct_in_rectangle"] = round(100.0 * float((fit_cls[mask] == 2).mean()), 2)
        res["%s, noise %.1f px" % (name, noise)] = row
        print("quality", name, noise, json.dumps(row), flush=True)
out["quality"] = res
print(json.dumps(out))
