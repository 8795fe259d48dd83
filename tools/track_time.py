"""dflow_track_advance, dflow_track_seed and dflow_track_flow alone, timed with HIP events on the current stream:
python tools/track_time.py [reps]
1024x436 (the bench frame), 446 464 tracks (one per pixel, step 1) on the forward and backward [dy,dx] flows a run_batch synthetic
pair leaves after 4 sweeps.  track_advance from the seed positions with and without d_bwd (all outputs), track_seed into an empty
set (every cell seeded) and after one advance (only the uncovered cells), track_flow between the two snapshots; in the same
process dflow_flow_consistency with DFLOW_FBC_BILINEAR, which samples one field where the advance samples two.  Median and minimum
milliseconds of `reps` calls (default 20) after a warm-up call, with the bytes each call has to move at least (every plane once,
a flow field once however often its pixels are gathered) and the time the plain-copy rate DESIGN 5.18 cites (6.29 TB/s) would
need for them.  Prints one JSON line."""
import importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
COPY_TBPS = 6.29
dev = torch.device("cuda", 0)
H, W = 436, 1024
N = H * W
s = _lib.stream(dev)
df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
fwd = df.run(img1, img2, 4).clone()
bwd = df.run(img2, img1, 4).clone()
i32 = dict(dtype=torch.int32, device=dev)
cap = 2 * N
pos, state, birth, n = torch.zeros((cap, 2), device=dev), torch.zeros(cap, **i32), torch.zeros(cap, **i32), torch.zeros(1, **i32)
pos1, state1, err = torch.empty((cap, 2), device=dev), torch.empty(cap, **i32), torch.empty(cap, device=dev)
scan = torch.empty(pipeline.track_scan_len(H, W, 1), **i32)
owner, out = torch.empty((H, W), **i32), torch.empty((H, W, 3), device=dev)
c6, c4, c3, c5 = (torch.empty(k, **i32) for k in (6, 4, 3, 5))
fbc_out, fbc_err = torch.empty((H, W, 3), device=dev), torch.empty((H, W), device=dev)


def timed(call, prep=None):
    ms = []
    for i in range(1 + reps):
        if prep:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


def seed(frame):
    _lib.call("dflow_track_seed", H, W, cap, 1, frame, None, pos.data_ptr(), state.data_ptr(), birth.data_ptr(), n.data_ptr(), scan.data_ptr(),
              c4.data_ptr(), s)


def advance(ntracks, back, p_in=pos, s_in=state):
    _lib.call("dflow_track_advance", H, W, fwd.data_ptr(), _lib.EVAL_DYDX, bwd.data_ptr() if back else None, _lib.EVAL_DYDX, ntracks,
              p_in.data_ptr(), s_in.data_ptr(), 0.01, 0.5, 0, pos1.data_ptr(), state1.data_ptr(), err.data_ptr(), c6.data_ptr(), s)


def clear():
    state.zero_()
    n.zero_()


def with_bytes(r, nbytes):
    r["bytes"] = int(nbytes)
    r["copy_rate_ms"] = round(nbytes / COPY_TBPS / 1e9, 4)
    return r


res = {"size": "%dx%d" % (W, H), "reps": reps, "tracks": N, "copy_rate_TBps": COPY_TBPS}
res["seed_empty"] = with_bytes(timed(lambda: seed(0), clear), N * (4 + 4 + 4 + 16) + cap * 4)      # cells: clear, count, emit; a slot; the mark's states
res["seed_empty_counts"] = dict(zip(pipeline.TRACK_SEED_COUNTS, c4.cpu().tolist()))
field = N * 8
for back in (True, False):
    r = with_bytes(timed(lambda: advance(N, back)), N * (12 + 12 + 4) + field * (2 if back else 1))
    res["advance_%s" % ("fb" if back else "forward_only")] = r
    res["advance_%s_counts" % ("fb" if back else "forward_only")] = dict(zip(pipeline.TRACK_ADVANCE_COUNTS, c6.cpu().tolist()))
# the set one frame on, the whole capacity (half of it FREE), then the reseed of the cells the survivors left
advance(cap, True)
torch.cuda.synchronize()
keep_pos, keep_state, n0 = pos1.clone(), state1.clone(), n.clone()
pos_a, state_a = pos.clone(), state.clone()


def restore():
    pos.copy_(keep_pos)
    state.copy_(keep_state)
    n.copy_(n0)


live = int((keep_state[:N] == _lib.TRACK_LIVE).sum())
res["seed_after_advance"] = with_bytes(timed(lambda: seed(1), restore), N * (4 + 4 + 4) + N * 12 + cap * 4 + (N - live) * 16)
res["seed_after_advance_counts"] = dict(zip(pipeline.TRACK_SEED_COUNTS, c4.cpu().tolist()))
r = timed(lambda: _lib.call("dflow_track_flow", H, W, cap, pos_a.data_ptr(), state_a.data_ptr(), keep_pos.data_ptr(), keep_state.data_ptr(),
                            owner.data_ptr(), out.data_ptr(), c3.data_ptr(), s))
res["flow"] = with_bytes(r, N * (4 + 4 + 12) + 2 * cap * 8 + N * (16 + 4) + live * 16)     # owner: set, read; out; the states twice; claims; winners
res["flow_counts"] = dict(zip(pipeline.TRACK_FLOW_COUNTS, c3.cpu().tolist()))
r = timed(lambda: _lib.call("dflow_flow_consistency", H, W, fwd.data_ptr(), _lib.EVAL_DYDX, bwd.data_ptr(), _lib.EVAL_DYDX, 1.0,
                            _lib.FBC_BILINEAR, fbc_out.data_ptr(), None, fbc_err.data_ptr(), None, c5.data_ptr(), s))
res["flow_consistency_bilinear"] = with_bytes(r, 2 * field + N * (12 + 4))
print(json.dumps(res))
