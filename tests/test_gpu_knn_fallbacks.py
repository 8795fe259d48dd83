"""The fallbacks of the MFMA-screened kNN search (csrc/knn_mfma.hip) at the sizes that reach them, against the CPU oracle:

* an event list that runs out (a lane with an event in every tile of a cell of more than 2880 points) goes to knn_fix_kernel
  list by list;
* a list of 90 entries per lane (the most a cell of 2880 points gives) goes through knn_resolve_heavy_kernel in several batches
  of 64 entries;
* (query, cell) pairs beyond the capacity of the heavy kernel's item list stay in knn_resolve_kernel;
* low-texture content on binary16 planes (knn_resolve_kernel<true>, knn_resolve_heavy_kernel<true>).

Every case runs on both descriptor storages, compares proposals, costs, counts and WTA labels bit for bit with the oracle (on
the descriptors rounded to binary16 where the planes hold binary16) and with the brute-force kernel, and checks through
dflow_knn_screen_stats that the path it is meant for was taken.  The outputs and the workspace are filled with garbage before
each screened pass: a slot that no kernel writes, or a statistic read from a list the screen did not write, shows.
Run with `pytest -m gpu`."""
import json

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

# knn_mfma.hip: candidates per LDS chunk (cells are padded to whole chunks of 32-row tiles), list capacity cap, queries per
# list, list entries above which a (query, cell) pair goes to the heavy kernel, capacity of the heavy kernel's item list
KM_CHUNK, KM_EVROWS_MAX, KM_QPW, KM_HEAVY_ENTRIES, KM_HEAVY_CAP = 192, 96, 64, 32, 1 << 20
STORAGES = ("f32", "f16")
OUTPUTS = ("proposals", "lcosts", "nprop", "bestlabels")


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def stored(d, storage):
    """What the descriptor planes hold: binary16 planes round every value (numpy float16 = torch's rounding)."""
    return d.astype(np.float16).astype(np.float32) if storage == "f16" else d


def new_pass(H, W, ch, cw, storage, seed=0):
    L = pkg("_lib")
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed, flags=L.FLAG_DESCR_F16 if storage == "f16" else 0)


def query_descriptors(O, synth, H, W, seed):
    """Real DAISY of a textured pair.  DAISY leaves a few all-zero rows in the bottom corners (reads near the edge are zeroed):
    those would take the all-zero-query shortcut and emit no events, so they get the row of the centre pixel."""
    img1, img2, _ = synth.make_pair(H, W, seed=seed)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    assert d1[H // 2, W // 2].any()
    d1[~d1.any(-1)] = d1[H // 2, W // 2]
    assert d1.any(-1).all()
    return d1, d2


def run(df, d1, d2, exact=False):
    """One generisi on (d1, d2), MFMA-screened or brute force; outputs and workspace poisoned first.  -> (host state, stats)."""
    L = pkg("_lib")
    df.p.flags = (df.p.flags & ~L.FLAG_KNN_EXACT) | (L.FLAG_KNN_EXACT if exact else 0)
    df.set_descriptors(d1, d2)
    df.ws.fill_(1)                              # an event list the screen does not write holds one entry of garbage
    df.proposals.fill_(0x7FFF7FFF)
    df.lcosts.fill_(float("nan"))
    df.nprop.fill_(-1)
    df.bestlabels.fill_(-1)
    df.generisi()
    stats = None if exact else df.knn_stats()
    return df.host_state(), stats


def check_pass(O, df, d1, d2, storage, case):
    """Screened pass against the oracle and the brute-force kernel, bit for bit; returns the screen's statistics."""
    p = O.make_params(df.p.pich, df.p.picw, df.p.cellh, df.p.cellw, seed=df.p.seed)
    st, stats = run(df, d1, d2)
    print(json.dumps({"case": case, "storage": storage, **stats}))
    ref = dict(zip(OUTPUTS, O.knn_proposals(p, stored(d1, storage), stored(d2, storage))))
    for k in OUTPUTS:
        assert np.array_equal(st[k], ref[k]), (case, storage, k)
    ex, _ = run(df, d1, d2, exact=True)
    for k in OUTPUTS:
        assert np.array_equal(ex[k], ref[k]), (case, storage, "exact kernel", k)
    return stats


def ntiles(npts):
    return -(-npts // KM_CHUNK) * KM_CHUNK // 32


def lane_lists(npts):
    """(entries, events) of the two half-lane lists of a query against a cell of npts points when every candidate is an event:
    tile t, row r holds candidate r * ntiles + t (knn_prep_kernel); half-lane h sees rows 4 h + (i & 3) + 8 (i >> 2)."""
    nt = ntiles(npts)
    out = []
    for h in (0, 1):
        rows = np.array([4 * h + (i & 3) + 8 * (i >> 2) for i in range(16)])
        real = rows[:, None] * nt + np.arange(nt)[None, :] < npts          # (row, tile)
        out.append((int(real.any(0).sum()), int(real.sum())))
    return out


def expected_all_events(H, W, ch, cw, window=2):
    """The statistics of a pass in which every candidate of every cell is an event for every query (exact ties)."""
    ncx, ncy = W // cw, H // ch
    xs = [(i * cw, W if i == ncx - 1 else (i + 1) * cw) for i in range(ncx)]
    ys = [(j * ch, H if j == ncy - 1 else (j + 1) * ch) for j in range(ncy)]
    npts = lambda ci, cj: (xs[ci][1] - xs[ci][0]) * (ys[cj][1] - ys[cj][0])
    cap = min(ntiles(npts(ncx - 1, ncy - 1)) + 1, KM_EVROWS_MAX)
    e = dict(lists_exact=0, entries=0, events=0, max_entries_per_lane=0, query_cell_pairs=0, heavy=0, list_capacity=cap)
    for qcj in range(ncy):
        for qci in range(ncx):
            qn = npts(qci, qcj)
            waves = -(-qn // KM_QPW)
            for ci in range(max(0, qci - window), min(ncx - 1, qci + window) + 1):
                for cj in range(max(0, qcj - window), min(ncy - 1, qcj + window) + 1):
                    halves = lane_lists(npts(ci, cj))
                    e["query_cell_pairs"] += qn
                    if any(n >= cap for n, _ in halves):        # a lane's list ran out: the list goes to knn_fix_kernel
                        e["lists_exact"] += waves
                        continue
                    # per list: 2 groups x 32 query columns per half-lane (columns past the cell's queries repeat its last one)
                    e["entries"] += waves * 64 * sum(n for n, _ in halves)
                    e["events"] += waves * 64 * sum(v for _, v in halves)
                    e["max_entries_per_lane"] = max(e["max_entries_per_lane"], *(n for n, _ in halves))
                    if sum(n for n, _ in halves) > KM_HEAVY_ENTRIES:
                        e["heavy"] += qn
    e["heavy_pairs"], e["heavy_pairs_left"] = min(e["heavy"], KM_HEAVY_CAP), max(e["heavy"] - KM_HEAVY_CAP, 0)
    del e["heavy"]
    return e


def assert_stats(stats, expected):
    assert stats["flags"] == 0 and stats["bad_queries"] == 0 and stats["zero_queries"] == 0, stats
    got = {k: stats[k] for k in expected}
    assert got == expected, (got, expected)


# (H, W, cellh, cellw): cells of 2880 points = 90 tiles, capacity 91: the fullest list that cannot run out (90 entries per lane,
# 180 per (query, cell): three batches of the heavy kernel); cells of 3040 points = 96 tiles, capacity 96: every lane's list runs
# out; ragged: cells of 2880 points above a last cell row of 38 x 80 = 3040 points, only the lists against that row run out
FULL, OVERFLOW, RAGGED = (120, 216, 40, 72), (120, 228, 40, 76), (110, 240, 36, 80)


def test_geometries_reach_the_list_capacity_boundary():
    """The numbers the cases below are built on (no GPU needed, but kept next to the cases they describe)."""
    assert lane_lists(2880) == [(90, 1440), (90, 1440)] and ntiles(2880) == 90
    assert lane_lists(3040) == [(96, 1536), (96, 1504)] and ntiles(3040) == 96
    full, ovf, rag = expected_all_events(*FULL), expected_all_events(*OVERFLOW), expected_all_events(*RAGGED)
    assert full["list_capacity"] == 91 and full["max_entries_per_lane"] == 90 and full["lists_exact"] == 0
    assert full["heavy_pairs"] == full["query_cell_pairs"] == 120 * 216 * 9
    assert ovf["list_capacity"] == 96 and ovf["lists_exact"] == 9 * 48 * 9 and ovf["entries"] == ovf["heavy_pairs"] == 0
    # every query cell sees the three cells of the bottom row: 3 x (45 + 45 + 48) query waves x 3 candidate cells
    assert rag["list_capacity"] == 96 and rag["lists_exact"] == 3 * 138 * 3 and rag["max_entries_per_lane"] == 90
    assert rag["heavy_pairs"] == 110 * 240 * 6


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("geom", [FULL, OVERFLOW, RAGGED], ids=["full_2880", "overflow_3040", "ragged"])
def test_tied_cells_at_the_list_capacity(torch_, oracle, synth, geom, storage):
    """Image 2 is ONE descriptor row repeated: every distance in a cell ties, every candidate is an event for every query, and
    the answer is the 5 lowest in-cell indices.  The statistics must be exactly those of that picture: full lists through the
    heavy kernel where the capacity holds them, every list with a lane that ran out through knn_fix_kernel one by one (the
    pass as a whole never handed over)."""
    O = oracle
    H, W, ch, cw = geom
    d1, d2 = query_descriptors(O, synth, H, W, seed=3)
    t = d2[H // 2, W // 2].copy()
    assert t.any()
    d2 = np.broadcast_to(t, d2.shape).copy()
    df = new_pass(H, W, ch, cw, storage)
    O.set_threads(16)
    try:
        stats = check_pass(O, df, d1, d2, storage, "tied_%dx%d_c%dx%d" % (H, W, ch, cw))
    finally:
        O.set_threads(1)
    assert_stats(stats, expected_all_events(H, W, ch, cw))
    assert stats["lists_exact"] < stats["lists"]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("geom", [FULL, OVERFLOW], ids=["full_2880", "overflow_3040"])
def test_perturbed_rows_make_the_end_of_every_list_count(torch_, oracle, synth, geom, storage):
    """Image 2 rows are T + eps u (u seeded, uniform in [-1, 1]^68, eps = 1 % of the mean |T| component): the f32 distances
    differ, so the 5 nearest sit anywhere in the cell and a kernel that lost the last entries of a list (or a list) would
    give other answers.  eps is still so small against the screen's allowance that every lane keeps an event in every tile:
    the lists are exactly as full as in the tied case, which the statistics confirm (all but a few thousand of the 672 M
    (query, candidate) pairs stay events).  On binary16 planes the perturbation survives the rounding."""
    O = oracle
    H, W, ch, cw = geom
    d1, d2 = query_descriptors(O, synth, H, W, seed=3)
    t = d2[H // 2, W // 2].copy()
    u = np.random.default_rng(11).uniform(-1.0, 1.0, d2.shape).astype(np.float32)
    d2 = (t + np.float32(0.01 * np.abs(t).mean()) * u).astype(np.float32)
    cell = stored(d2, storage)[:ch, :cw].reshape(-1, 68)
    assert len(np.unique(cell, axis=0)) == ch * cw                  # no two rows of a cell tie in any storage
    df = new_pass(H, W, ch, cw, storage)
    O.set_threads(16)
    try:
        stats = check_pass(O, df, d1, d2, storage, "perturbed_%dx%d_c%dx%d" % (H, W, ch, cw))
    finally:
        O.set_threads(1)
    expected = expected_all_events(H, W, ch, cw)
    events = expected.pop("events")
    assert_stats(stats, expected)
    assert 0.9999 * events <= stats["events"] <= events, (stats, events)


@pytest.mark.parametrize("storage", STORAGES)
def test_heavy_pairs_beyond_the_cap_stay_in_the_lane_per_query_kernel(torch_, oracle, synth, storage):
    """Bench-like cells of 27 x 64 = 1728 points on 512 x 270: 2.6 M (query, cell) pairs.  Image 2 is made of three DAISY rows
    chosen per pixel at random, so a query's nearest row ties exactly in almost every tile: about 108 list entries per pair,
    every pair heavy.  The heavy kernel's list takes the first 2^20 pairs, the rest are resolved by knn_resolve_kernel."""
    O = oracle
    H, W, ch, cw = 270, 512, 27, 64
    d1, d2 = query_descriptors(O, synth, H, W, seed=5)
    rows = np.stack([d2[H // 4, W // 4], d2[H // 2, W // 2], d2[3 * H // 4, 3 * W // 4]])
    assert rows.any(-1).all() and len(np.unique(stored(rows, storage), axis=0)) == 3
    d2 = rows[np.random.default_rng(7).integers(0, 3, (H, W))]
    df = new_pass(H, W, ch, cw, storage)
    O.set_threads(16)
    try:
        stats = check_pass(O, df, d1, d2, storage, "heavy_cap")
    finally:
        O.set_threads(1)
    assert stats["flags"] == 0 and stats["lists_exact"] == 0 and stats["zero_queries"] == 0, stats
    assert stats["max_entries_per_lane"] < stats["list_capacity"] == ntiles(ch * cw) + 1, stats
    assert stats["heavy_pairs"] == KM_HEAVY_CAP and stats["heavy_pairs_left"] > 0, stats
    assert stats["heavy_pairs"] + stats["heavy_pairs_left"] == stats["query_cell_pairs"], stats


@pytest.mark.parametrize("storage", STORAGES)
def test_low_texture_kitti_frame_matches_oracle(torch_, oracle, synth, storage):
    """The low-texture frame of test_low_texture_kitti_fp16_planes_match_exact_kernel (1242 x 375, cells 54 x 25) against the
    oracle: saturated sky, flat road, blur and a repeated pattern, with hundreds of near-ties per cell in the fringes of the flat
    regions (the heavy kernel) -- on binary16 planes, the variants of the resolve kernels that read them."""
    O = oracle
    H, W = 375, 1242
    img1, img2, _ = synth.make_pair(H, W, seed=3, style="low_texture")
    df = new_pass(H, W, 25, 54, storage, seed=1)
    O.set_threads(16)
    try:
        d1, d2 = O.daisy(img1), O.daisy(img2)
        df.load_pair(img1, img2)
        assert np.array_equal(df.descriptors_f32(0).cpu().numpy().view(np.uint32), stored(d1, storage).view(np.uint32))
        assert np.array_equal(df.descriptors_f32(1).cpu().numpy().view(np.uint32), stored(d2, storage).view(np.uint32))
        stats = check_pass(O, df, d1, d2, storage, "low_texture_kitti")
    finally:
        O.set_threads(1)
    assert stats["flags"] == 0 and stats["lists_exact"] == 0 and stats["zero_queries"] > 0.2 * H * W, stats
    assert 0 < stats["heavy_pairs"] < KM_HEAVY_CAP and stats["heavy_pairs_left"] == 0, stats
