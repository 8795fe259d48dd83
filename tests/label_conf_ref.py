"""dflow_label_confidence and dflow_flow_gate as include/dflow.h defines them, in numpy: float64 with the definition's two
operations per e_k, one astype(np.float32) for the margin.  No step depends on an order, so the GPU comparison is bit for bit.

A plain module: no fixtures, no pytest hooks."""
import numpy as np

LOCAL, DATA = 0, 1
COUNTS = ("labelled", "not_labelled", "no_alternative", "negative", "zero", "kept")


def label_conf_ref(flows, costs, nprop, labels, tpsi, lamda, mode=LOCAL, min_sep=1, thresh=-np.inf):
    """flows (H,W,LP,2) integers [dy,dx], costs (H,W,LP), nprop and labels (H,W) -> dict(margin (H,W) float32, alt (H,W) int32,
    sparse (H,W,3) float32, counts: the six of COUNTS as a list, energy (H,W,LP) float64: e_k of every slot)."""
    flows = np.asarray(flows).astype(np.int64)
    H, W, LP, _ = flows.shape
    costs = np.asarray(costs).astype(np.float32).astype(np.float64)     # (double)c_k
    labels = np.asarray(labels).astype(np.int64)
    n_p = np.minimum(np.asarray(nprop).astype(np.int64), LP)
    ok = (labels >= 0) & (labels < n_p)
    chosen = np.take_along_axis(flows, np.clip(labels, 0, LP - 1)[:, :, None, None], axis=2)[:, :, 0, :]       # (H,W,2), where ok
    # s_k: the four neighbours inside the frame that are labelled
    s = np.zeros((H, W, LP), np.int64)
    g = np.zeros((H + 2, W + 2, 2), np.int64)
    gok = np.zeros((H + 2, W + 2), bool)
    g[1:-1, 1:-1], gok[1:-1, 1:-1] = chosen, ok
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        gq, okq = g[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx], gok[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        d = np.abs(flows - gq[:, :, None, :]).sum(-1)
        s += np.minimum(int(tpsi), d) * okq[:, :, None]
    if mode == LOCAL:
        e = np.float64(lamda) * costs + s.astype(np.float64)            # one multiplication, one addition
    else:
        e = costs.copy()
    k = np.arange(LP)[None, None, :]
    in_a = ok[:, :, None] & (k < n_p[:, :, None]) & (np.abs(flows - chosen[:, :, None, :]).sum(-1) > int(min_sep))
    masked = np.where(in_a, e, np.inf)
    alt = np.argmin(masked, axis=2)                                     # the first of the smallest: the smaller index wins a tie
    has = in_a.any(axis=2)
    e_alt = np.take_along_axis(e, alt[:, :, None], axis=2)[:, :, 0]
    e_l = np.take_along_axis(e, np.clip(labels, 0, LP - 1)[:, :, None], axis=2)[:, :, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        margin = (e_alt - e_l).astype(np.float32)                       # a subtraction in double, one rounding
    margin = np.where(has, margin, np.float32(np.inf)).astype(np.float32)
    margin = np.where(ok, margin, np.float32(-np.inf)).astype(np.float32)
    alt = np.where(has, alt, -1).astype(np.int32)
    kept = ok & (margin >= np.float32(thresh))
    sparse = np.zeros((H, W, 3), np.float32)
    sparse[kept, 0], sparse[kept, 1], sparse[kept, 2] = chosen[kept, 1], chosen[kept, 0], 1.0
    counts = [int(ok.sum()), int((~ok).sum()), int((ok & ~has).sum()), int((ok & (margin < 0)).sum()),
              int((ok & (margin == 0)).sum()), int(kept.sum())]
    return dict(margin=margin, alt=alt, sparse=sparse, counts=counts, energy=e)


def flow_gate_ref(flow, score, lo=-np.inf, hi=np.inf):
    """flow (H,W,2) [dy,dx] or (H,W,3) [U,V,valid] float32, score (H,W) float32 -> ((H,W,3) float32, [good, kept])."""
    flow = np.asarray(flow, np.float32)
    uvv = flow if flow.shape[2] == 3 else np.stack([flow[..., 1], flow[..., 0], np.ones(flow.shape[:2], np.float32)], axis=-1)
    good = (uvv[..., 2] > 0.5) & np.isfinite(uvv[..., 0]) & np.isfinite(uvv[..., 1])
    keep = good & (np.asarray(score, np.float32) >= np.float32(lo)) & (np.asarray(score, np.float32) <= np.float32(hi))
    out = np.where(keep[..., None], np.stack([uvv[..., 0], uvv[..., 1], np.ones_like(uvv[..., 0])], axis=-1), np.float32(0)).astype(np.float32)
    return out, [int(good.sum()), int(keep.sum())]


class RandomState:
    """A random labelling problem in the reference's form, as tests/test_gpu_bcd_stats.State draws it: flows in -4..4, nprop in
    1..maxnprop, costs in [0, 3) with a tenth exactly tphi = 2.5 (quantised=True: multiples of 0.25 up to 2.5, so that with lamda
    = 4 every e_k is an integer and ties occur), labels inside nprop but for a share of -1 and of labels >= nprop."""

    def __init__(self, H, W, seed, maxnprop=150, label_pitch=160, quantised=False):
        rng = np.random.default_rng(seed)
        LP = label_pitch
        self.H, self.W, self.maxnprop, self.label_pitch = H, W, maxnprop, LP
        self.flows = rng.integers(-4, 5, (H, W, LP, 2)).astype(np.int64)
        if quantised:
            self.costs = (rng.integers(0, 11, (H, W, LP)) * 0.25).astype(np.float32)
        else:
            self.costs = (rng.random((H, W, LP)) * 3).astype(np.float32)
            self.costs[rng.random((H, W, LP)) < 0.1] = np.float32(2.5)
        self.nprop = rng.integers(1, maxnprop + 1, (H, W)).astype(np.int64)
        # every tenth pixel has few labels: with min_sep = 3 some of them have no alternative
        few = rng.random((H, W)) < 0.1
        self.nprop[few] = rng.integers(1, 3, (H, W))[few]
        self.labels = (rng.random((H, W)) * self.nprop).astype(np.int64)
        # every 11th pixel is -1, every other 11th nprop, nprop + 100 or nprop + 200 (beyond the pitch), in turn
        flat, n = self.labels.reshape(-1), self.nprop.reshape(-1)
        i = np.arange(flat.size)
        flat[i % 11 == 3] = -1
        at = i % 11 == 7
        flat[at] = n[at] + (i[at] // 11 % 3) * 100
        # slots at or beyond nprop hold what the stages leave there, and must never show: the fill values
        free = np.arange(LP)[None, None, :] >= self.nprop[:, :, None]
        self.flows[free] = -1
        self.costs[free] = np.float32(1000.0)

    def packed(self):
        return (self.flows[..., 0].astype(np.int16).view(np.uint16).astype(np.uint32)
                | (self.flows[..., 1].astype(np.int16).view(np.uint16).astype(np.uint32) << 16))

    def ref(self, tpsi, lamda, **kw):
        return label_conf_ref(self.flows, self.costs, self.nprop, self.labels, tpsi, lamda, **kw)


# ---- what tests/test_gpu_label_conf.py runs, and tests/test_label_conf_ref.py checks the inputs of
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (65, 129)]      # missing neighbours per axis; partial tiles, several blocks per axis
# (label_pitch, maxnprop, tpsi, min_sep, mode, lamda, quantised costs): both pitches, tpsi 1 and 8, min_sep 0, 1 and 3, both modes,
# lamda 0, 0.05 and 4 (with the quantised costs, so that e_k is an integer and ties occur)
COMBOS = [(16, 5, 8, 1, LOCAL, 0.05, False), (160, 150, 1, 0, LOCAL, 4.0, True), (160, 150, 8, 3, DATA, 0.05, False),
          (16, 5, 1, 3, LOCAL, 0.0, False), (160, 150, 8, 1, LOCAL, 4.0, True), (16, 5, 8, 0, DATA, 4.0, True)]
THRESH = 0.0
_states = {}


def gpu_state(shape, label_pitch, maxnprop, quantised):
    """The random state of a shape and a combo's lay-out, made once and shared; nobody changes it."""
    H, W = shape
    if label_pitch == 160 and H * W > 4000:
        maxnprop = 40
    key = (H, W, label_pitch, maxnprop, quantised)
    if key not in _states:
        _states[key] = RandomState(H, W, seed=1000 * H + 10 * W + label_pitch + quantised, maxnprop=maxnprop, label_pitch=label_pitch,
                                   quantised=quantised)
    return _states[key]
