"""dflow_bcd_stats alone, timed with HIP events on the current stream, next to one dflow_bcd_sweep, and the per-sweep history of
the optimiser: python tools/bcd_stats_time.py [reps] [sweeps]
1024x436 (the bench frame), the bench's first pair (synth.pair_seed(0, 0)) in the dense and in the low_texture style, forward
pass.  Per pair: the median and minimum milliseconds of `reps` (20) calls of dflow_bcd_stats (2 launches, with an earlier
labelling and the copy of the labels) and of dflow_bcd_sweep (4 launches; the sweep kernels are the ones the library had
before the statistics existed) on the labels after generisi + nasumicni, their ratio, and then the history of `sweeps` (12)
sweeps: labels changed and the image energy E = lamda * data_sum + smooth_sum after every sweep (ceoBCD with an empty stop
rule).  Prints one JSON line; DESIGN.md "BCD statistics and the stop rule" quotes it."""
import ctypes as C, importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "lk-s-2022-estimacija-pokreta_amd"
_lib, synth, pipeline = (importlib.import_module(PKG + "." + m) for m in ("_lib", "synth", "pipeline"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sweeps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
H, W = 436, 1024
dev = torch.device("cuda", 0)


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}


def timed(call, restore):
    for _ in range(3):
        restore(); call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        restore()
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    return spread(a.elapsed_time(b) for a, b in ev)


out = {"size": "%dx%d" % (W, H), "reps": reps, "sweeps": sweeps, "pairs": {}}
for style in ("dense", "low_texture"):
    kw = {} if style == "dense" else {"style": "low_texture"}
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0), **kw)
    df = pipeline.DiscreteFlow(H, W, device=dev, seed=0)
    df.load_pair(img1, img2); df.generisi(); df.nasumicni(); df.pakovanje()
    wta = df.bestlabels.clone()
    prev = wta.clone()
    stats = torch.zeros(6, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib().dflow_bcd_stats_workspace_bytes(C.byref(df.p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = _lib.stream(dev)
    t_stats = timed(lambda: _lib.call("dflow_bcd_stats", df._pp(), df.proposals.data_ptr(), df.lcosts.data_ptr(), df.nprop.data_ptr(),
                                      df.bestlabels.data_ptr(), prev.data_ptr(), prev.data_ptr(), stats.data_ptr(), ws.data_ptr(), wsb, s),
                    lambda: None)
    # every timed sweep starts from the same labels: the first sweep of a pass, the one that changes most
    t_sweep = timed(lambda: _lib.call("dflow_bcd_sweep", df._pp(), df.proposals.data_ptr(), df.nprop.data_ptr(), df.bestlabels.data_ptr(),
                                      df.ws.data_ptr(), df.ws_bytes, s),
                    lambda: df.bestlabels.copy_(wta))
    df.bestlabels.copy_(wta)
    hist = df.ceoBCD(sweeps, stop={})
    out["pairs"][style] = {"bcd_stats": t_stats, "bcd_sweep": t_sweep, "workspace_bytes": wsb,
                           "stats_over_sweep": round(t_stats["median_ms"] / t_sweep["median_ms"], 5),
                           "history": [{"sweep": h["sweep"], "changed": h["n_changed"], "E": round(h["energy"], 3),
                                        "data_sum": round(h["data_sum"], 3), "smooth_sum": h["smooth_sum"],
                                        "n_pairs_trunc": h["n_pairs_trunc"], "n_data_trunc": h["n_data_trunc"]} for h in hist]}
    del df
print(json.dumps(out))
