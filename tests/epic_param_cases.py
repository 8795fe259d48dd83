"""Inputs shared by test_epic_params_ref.py (CPU: what the reference does with them, and the float32 yardstick) and
test_gpu_epic_params.py (the GPU against the reference): small frames on which every seed's nearest-256 list is full, one
whose seed graph has a row of more than 128 edges, one with special values in the edge map and the valid plane; and the
reference for every nn and k of the sweep from one Dijkstra per seed, by the prefix law of the neighbour lists."""
import functools

import numpy as np

import epic_prefilter_cases as PC
import epic_prefilter_ref as P
import epic_ref as R

NN_MAX = 256
# list lengths around every multiple of 64: a frontier or settled slot j is first written at 64 j + 1 entries
NNS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
KS = (1e-300, 0.05, 0.8, 10.0, 200.0, 1e300)          # every weight exactly 1 ... every weight but the seed's own exactly 0
K_SWEEP_NNS = (3, 65, 256)
K_SWEEP_INPUTS = ("dense32x48", "hub64x96")
PREF_NNS = (1, 2, 63, 64, 127, 128, 129, 191, 192, 255)
PREF_KS = (0.05, 0.8, 10.0, 200.0)
PREF_TH = 4.0
PREF_INPUTS = ("dense32x48", "ties32x48", "hub64x96")
FULL_LIST_INPUTS = ("dense32x48", "ties32x48", "sparse32x48")
INTERP_INPUTS = FULL_LIST_INPUTS + ("hub64x96",)
WIDE_HUB_NNS = (193, 256)                               # hub72x104 runs at these alone
EXCLUSION_CAP = 0.01                                   # share of a case's seeds that may lie within 1 % of TAU
FACTOR = 4                                             # the project's margin over a measured float32 yardstick

EDGE_VALUES = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 0.0005, 0.0015, 0.0025, 0.5, 0.9995, 1.0,
                        np.nextafter(np.float32(1), np.float32(2)), 7.0, np.inf], np.float32)
VALID_VALUES = np.array([0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0, 2.0, -1.0, np.nan, np.inf], np.float32)


def hub(H, W, half):
    """Every pixel a seed but for a square hole of side 2 half + 1 around the centre, with a wall of e = 1 on the hole's
    rim and one seed, the hub, in its middle: the hub's cell is the interior of side 2 half - 1, and its row of the seed
    graph has an edge to every ring seed along the wall, 4 (2 half - 1) of them."""
    cy, cx = H // 2, W // 2
    rng = np.random.default_rng(6)
    sp = np.zeros((H, W, 3), np.float32)
    sp[..., 0], sp[..., 1], sp[..., 2] = rng.normal(0, 4, (H, W)), rng.normal(0, 4, (H, W)), 1.0
    own = sp[cy, cx].copy()
    sp[cy - half:cy + half + 1, cx - half:cx + half + 1] = 0
    sp[cy, cx] = own
    e = np.zeros((H, W), np.float32)
    e[cy - half:cy + half + 1, cx - half:cx + half + 1] = 1.0
    e[cy - half + 1:cy + half, cx - half + 1:cx + half] = 0.0
    return sp, e


# name: (H, W, half).  hub64x96's row of 156 edges fills frontier slots 0 to 2 in one scan of three chunks; hub72x104's row of
# 196 reaches slot 3 in four (on the other inputs no frontier ever holds more than 158 entries)
HUBS = {"hub64x96": (64, 96, 20), "hub72x104": (72, 104, 25)}


def hub_id(name):
    H, W, _ = HUBS[name]
    return (H // 2) * W + W // 2


def edgevalues():
    """24x40, about 30 % seeded: the edge map cycles through EDGE_VALUES, the valid plane of 60 % of the pixels through
    VALID_VALUES (0 elsewhere), and three pixels with valid = 1 carry a NaN or an infinite flow."""
    H, W = 24, 40
    rng = np.random.default_rng(8)
    ys, xs = np.mgrid[0:H, 0:W]
    e = EDGE_VALUES[(ys * W + xs) % len(EDGE_VALUES)]
    m = rng.random((H, W)) < 0.6
    sp = np.zeros((H, W, 3), np.float32)
    sp[..., 0] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 1] = np.where(m, rng.normal(0, 4, (H, W)), 0)
    sp[..., 2] = np.where(m, VALID_VALUES[(xs + 3 * ys) % len(VALID_VALUES)], 0)
    ones = np.argwhere(m & (sp[..., 2] == 1))
    for (y, x), (c, bad) in zip(ones[[3, len(ones) // 2, -4]], ((0, np.nan), (1, np.inf), (0, -np.inf))):
        sp[y, x, c] = bad
    return sp, np.ascontiguousarray(e)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(sparse, edges) of an input; the arrays are shared: do not write to them."""
    if name == "dense32x48":
        return PC.random_field(32, 48, 0.94, seed=5)
    if name == "ties32x48":                                # every cost 1: G ties everywhere, the order is the seed id's
        return inputs("dense32x48")[0], np.zeros((32, 48), np.float32)
    if name == "sparse32x48":
        return PC.random_field(32, 48, 0.3, seed=5)
    return hub(*HUBS[name]) if name in HUBS else {"edgevalues": edgevalues}[name]()


class Ref:
    """The reference of an input up to the lists: S, D, the seed graph, the seed ids in ascending order, and every seed's
    nearest-256 list as (n, 256) arrays ids, G (-1 pads) with its length."""

    def __init__(self, name):
        self.name = name
        self.sparse, self.edges = inputs(name)
        self.H, self.W = self.edges.shape
        self.S, self.D = R.voronoi(self.sparse, self.edges)
        self.graph = R.seed_graph(self.S, self.D, self.edges)
        self.seeds = np.flatnonzero(R.seed_mask(self.sparse).ravel())
        self.lists = {s: R.neighbour_list(self.graph, s, NN_MAX) for s in self.seeds.tolist()}
        self.ids, self.G = R.list_arrays(self.lists, self.seeds.tolist(), NN_MAX)
        self.length = (self.ids >= 0).sum(axis=1)

    def list_planes(self, nn):
        """(H*W, nn) int64 planes as dflow_epic_interpolate writes them: a seed's row is its list, every other row -1."""
        ids = np.full((self.H * self.W, nn), -1, np.int64)
        G = np.full((self.H * self.W, nn), -1, np.int64)
        ids[self.seeds], G[self.seeds] = self.ids[:, :nn], self.G[:, :nn]
        return ids, G


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


@functools.lru_cache(maxsize=None)
def fits(name, k):
    """R.fit_prefixes of the input at every nn of the sweep."""
    r = ref(name)
    return R.fit_prefixes(r.sparse, r.seeds, r.ids, r.G, k, NNS)


@functools.lru_cache(maxsize=None)
def interp_case(name, nn, k, method):
    """What a GPU flow is held to: flow (H,W,2) float64, keep (H,W) bool (False at the pixels of a seed whose lambda_min is
    within 1 % of TAU, for LA; NW has no branch on it), excluded / seeds counts, yard (the float32 evaluation of the
    reference against its float64 one) and tol = FACTOR * max(yard, half a float32 ulp at the largest |flow|)."""
    r = ref(name)
    f = fits(name, k)[nn]
    flow = R.fill_plane(r.S, r.seeds, f[method])
    flow32 = R.fill_plane(r.S, r.seeds, f[method], np.float32)
    near = (np.abs(f["lmin"] - R.TAU) <= 0.01 * R.TAU) if method == "LA" else np.zeros(len(r.seeds), bool)
    keep = ~np.isin(r.S, r.seeds[near])
    yard = float(np.abs(flow32.astype(np.float64) - flow)[keep].max())
    half_ulp = 0.5 * float(np.spacing(np.float32(np.abs(flow[keep]).max())))
    return dict(flow=flow, keep=keep, excluded=int(near.sum()), seeds=len(r.seeds), lmin=f["lmin"], yard=yard,
                tol=FACTOR * max(yard, half_ulp))


@functools.lru_cache(maxsize=None)
def _estimates(name, k):
    """{pref_nn: (n,2) float64}: P.estimate of every seed over the pref_nn entries after its own, the sums grown entry by
    entry in list order; a seed with no other entry gets its own flow."""
    r = ref(name)
    flat = r.sparse.reshape(-1, 3).astype(np.float64)
    n = len(r.seeds)
    sw, su, sv = np.zeros(n), np.zeros(n), np.zeros(n)
    out = {}
    for j in range(1, max(PREF_NNS) + 1):
        live = r.ids[:, j] >= 0
        t = np.where(live, r.ids[:, j], 0)
        with np.errstate(over="ignore"):
            w = np.where(live, np.exp(-(k * r.G[:, j].astype(np.float64)) / 2000.0), 0.0)
        sw += w; su += w * np.where(live, flat[t, 0], 0.0); sv += w * np.where(live, flat[t, 1], 0.0)
        if j in PREF_NNS:
            with np.errstate(divide="ignore", invalid="ignore"):
                est = np.stack([su / sw, sv / sw], axis=1)
            out[j] = np.where((r.length > 1)[:, None], est, flat[r.seeds, :2])
    return out


def prefilter_case(name, pref_nn, k, pref_th=PREF_TH):
    """P.prefilter(sparse, edges, None, 0, pref_nn, pref_th, k) from the cached lists: with stage A skipped the survivors
    are the seeds themselves, and a seed's pref_nn + 1 nearest are a prefix of its nearest 256."""
    r = ref(name)
    est = _estimates(name, k)[pref_nn]
    uv = r.sparse.reshape(-1, 3).astype(np.float64)[r.seeds, :2]
    du, dv = est[:, 0] - uv[:, 0], est[:, 1] - uv[:, 1]
    drop = du * du + dv * dv > pref_th * pref_th
    reason = np.zeros(r.H * r.W, np.uint8)
    reason[r.seeds] = np.where(drop, P.CONSISTENCY, P.KEPT)
    plane = np.zeros((r.H * r.W, 2))
    plane[r.seeds] = est
    out = r.sparse.copy()
    out[reason.reshape(r.H, r.W) >= P.SALIENCY] = 0
    dist = dict(zip(r.seeds.tolist(), np.sqrt(du * du + dv * dv).tolist()))
    return dict(out=out, reason=reason.reshape(r.H, r.W), saliency=None, mid=r.sparse.copy(),
                estimate=plane.reshape(r.H, r.W, 2), dist=dist)
