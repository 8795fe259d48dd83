"""dflow_prior_proposals beside dflow_neighbour_proposals, and what a prior does to the flow: python tools/prior_time.py
1024x436 (the bench frame and its first synthetic pair).  Times: HIP events around each stage, 7 calls each from the same
restored state, one process: the neighbour stage (its two launches), the prior step at stride 0 and 2 with the pair's true flow
(with the counts, the bytes it has to move and the rate at the fastest call), a repeat call (everything found, no descriptor
read) and dflow_flow_advance.  Quality: mean end-point error after 0, 1, 2 and 4 sweeps without a prior, with the true flow,
with the negated advance of the backward pass's 4-sweep flow, and, as a control, with the previous pair's flow on the next,
unrelated pair; maxnprop 150 and 160.  Prints JSON lines, the last one everything."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
pipeline = importlib.import_module(PKG + ".pipeline")
synth = importlib.import_module(PKG + ".synth")
L = importlib.import_module(PKG + "._lib")

H, W = 436, 1024
out = {}


def state(df):
    return [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]


def restore(df, saved):
    for dst, src in zip((df.proposals, df.lcosts, df.nprop, df.bestlabels), saved):
        dst.copy_(src)
    df._bcd_ready = False


def timed(fn, before, reps=7):
    ms = []
    for _ in range(reps):
        before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def front(img1, img2, **over):
    df = pipeline.DiscreteFlow(H, W, **over)
    df.load_pair(img1, img2)
    df.generisi()
    after_knn = state(df)
    df.nasumicni()
    return df, after_knn, state(df)


def epe(flow, gt):
    return float((flow - gt).norm(dim=-1).mean())


img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
gt32 = np.ascontiguousarray(gt, dtype=np.float32)
gt_d = torch.from_numpy(gt32).cuda()

# ---- times
for name, over in (("f32", {}), ("f16", {"flags": L.FLAG_DESCR_F16})):
    df, after_knn, after_nbr = front(img1, img2, **over)
    t_nbr = timed(df.nasumicni, lambda: restore(df, after_knn))
    res = {"neighbour_stage_ms": t_nbr}
    for stride in (0, 2):
        t = timed(lambda: df.prior_proposals(gt_d, stride=stride), lambda: restore(df, after_nbr))
        restore(df, after_nbr)
        npr0 = df.nprop.clone()
        cnt = df.prior_proposals(gt_d, stride=stride, counts=True).cpu().tolist()
        grew = int((df.nprop > npr0).sum())
        row = 144 if name == "f16" else 272
        nbytes = int(npr0.sum()) * 4 + H * W * (5 if stride else 1) * 8 + cnt[0] * (row + 8) + grew * row + H * W * 8
        res["prior_stride%d" % stride] = {"ms": t, "counts": cnt, "bytes": nbytes, "GBps_at_min": nbytes / (min(t) * 1e-3) / 1e9}
    # a repeat call: everything found, no descriptor read
    t = timed(lambda: df.prior_proposals(gt_d, stride=2), lambda: None)
    res["prior_stride2_repeat_ms"] = t
    fa = timed(lambda: pipeline.flow_advance(gt_d), lambda: None)
    res["flow_advance_ms"] = fa
    out["times_" + name] = res
    print(name, json.dumps(res), flush=True)
    del df

# ---- quality
SWEEPS = (1, 2, 4)


def run(img1, img2, gt_d, prior, maxnprop=150, stride=2):
    df, _, _ = front(img1, img2, maxnprop=maxnprop)
    npr0 = df.nprop.clone()
    cnt = None
    if prior is not None:
        cnt = df.prior_proposals(prior, stride=stride, counts=True).cpu().tolist()
    r = {"counts": cnt, "epe": {}}
    r["epe"][0] = epe(df.vratiKonacniFlow(), gt_d)
    done = 0
    for s in SWEEPS:
        df.ceoBCD(s - done)
        done = s
        r["epe"][s] = epe(df.vratiKonacniFlow(), gt_d)
    r["share_final_label_appended_by_prior"] = float((df.bestlabels >= npr0).float().mean())
    if prior is not None:
        p = prior if isinstance(prior, torch.Tensor) else torch.from_numpy(prior).cuda()
        own = torch.round(p[..., :2].flip(-1)) if p.shape[2] == 3 else torch.round(p)
        eq = (df.vratiKonacniFlow() == own).all(dim=-1)
        if p.shape[2] == 3:
            eq &= p[..., 2] > 0.5
        r["share_final_flow_equals_own_prior"] = float(eq.float().mean())
    return r, df.vratiKonacniFlow().clone()


q = {}
q["no_prior"], fwd4 = run(img1, img2, gt_d, None)
print("no_prior", json.dumps(q["no_prior"]), flush=True)
for m in (150, 160):
    q["true_flow_maxnprop%d" % m], _ = run(img1, img2, gt_d, gt_d, maxnprop=m)
    print("true", m, json.dumps(q["true_flow_maxnprop%d" % m]), flush=True)
# the backward pass (images swapped, no prior) and its negated advance as the forward prior
bgt = torch.zeros_like(gt_d)
_, bwd4 = run(img2, img1, bgt, None)
inv = pipeline.flow_advance(bwd4, negate=True)
for m in (150, 160):
    q["inverse_of_backward_maxnprop%d" % m], _ = run(img1, img2, gt_d, inv, maxnprop=m)
    print("inverse", m, json.dumps(q["inverse_of_backward_maxnprop%d" % m]), flush=True)
# control: the previous pair's flow on the next, unrelated pair
img1b, img2b, gtb = synth.make_pair(H, W, seed=synth.pair_seed(1, 0))
gtb_d = torch.from_numpy(np.ascontiguousarray(gtb, dtype=np.float32)).cuda()
q["pair1_no_prior"], _ = run(img1b, img2b, gtb_d, None)
for m in (150, 160):
    q["pair1_prior_pair0_flow_maxnprop%d" % m], _ = run(img1b, img2b, gtb_d, fwd4, maxnprop=m)
    print("control", m, json.dumps(q["pair1_prior_pair0_flow_maxnprop%d" % m]), flush=True)
print("pair1_no_prior", json.dumps(q["pair1_no_prior"]), flush=True)
out["quality"] = q
print(json.dumps(out))
