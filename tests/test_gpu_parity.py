"""Parity of the HIP path (through the C-ABI) with the CPU oracle and with the reference's golden vectors.
Everything here needs a real MI355X: run with `pytest -m gpu`."""
import hashlib

import numpy as np
import pytest

from conftest import GOLDEN_NAMES, pkg

pytestmark = pytest.mark.gpu

# (H, W, cellh, cellw): exact tilings, ragged tilings (last cells absorb the remainder), more cells than the window
# thresholds of test_bench_config_four_sweeps_match_oracle_and_epe (set from the measured values, see its docstring)
EPE_REACHABLE_MEAN_MAX = 3.0
EPE_REACHABLE_MEDIAN_MAX = 1.0
EPE_REACHABLE_OUTLIER_PCT_MAX = 7.5

GEOMS = [(40, 48, 5, 6), (36, 40, 9, 8), (45, 70, 7, 9), (96, 128, 12, 16), (64, 200, 10, 12)]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def make(H, W, ch=None, cw=None, seed=0):
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed)


def oracle_params(O, df):
    p = df.p
    return O.make_params(p.pich, p.picw, p.cellh, p.cellw, seed=p.seed)


@pytest.mark.parametrize("shape", [(40, 56), (97, 131), (436, 1024)])
def test_daisy_bit_exact(torch_, oracle, synth, shape):
    H, W = shape
    img, _, _ = synth.make_pair(H, W, seed=H + W)
    df = make(H, W, max(5, H // 8), max(5, W // 8))
    got = df.izracunajDaisy(img).cpu().numpy()
    want = oracle.daisy(img)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("geom", GEOMS)
def test_stages_match_oracle(torch_, oracle, synth, geom):
    """DAISY -> generisi -> nasumicni -> every BCD phase of 2 sweeps, each stage compared bit for bit."""
    H, W, ch, cw = geom
    O = oracle
    img1, img2, _ = synth.make_pair(H, W, seed=H * W, amp_x=0.1 * W, amp_y=0.1 * H)
    df = make(H, W, ch, cw, seed=1234 + H)
    p = oracle_params(O, df)
    df.load_pair(img1, img2)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    assert np.array_equal(df.descrs1.cpu().numpy(), d1) and np.array_equal(df.descrs2.cpu().numpy(), d2)

    df.generisi()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    st = df.host_state()
    assert np.array_equal(st["nprop"], npr)
    assert np.array_equal(st["proposals"], pr), "bit-exact kNN candidate indices"
    assert np.array_equal(st["lcosts"], lc)
    assert np.array_equal(st["bestlabels"], bl)
    assert np.array_equal(df.vratiKonacniFlow().cpu().numpy().astype(np.float64), O.labels_to_flow(p, pr, bl))

    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    st = df.host_state()
    assert np.array_equal(st["nprop"], npr)
    assert np.array_equal(st["proposals"], pr)
    assert np.array_equal(st["lcosts"], lc)

    for sweep in range(2):
        for phase in range(4):
            df.bcd_phase(phase)
            O.bcd_phase(p, pr, lc, npr, bl, phase)
            got = df.bestlabels.cpu().numpy()
            assert np.array_equal(got, bl), "labels differ after sweep %d phase %d" % (sweep, phase)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
@pytest.mark.parametrize("backward", (0, 1))
def test_hip_path_matches_reference_golden(torch_, golden, name, backward):
    """HIP end to end against what the reference's own scripts produced (tests/golden), no oracle in between."""
    g = golden(name)
    df = make(int(g["H"]), int(g["W"]), int(g["cellh"]), int(g["cellw"]), seed=int(g["seed"]))
    k = "b%d_" % backward
    a, b = (g["img1"], g["img2"]) if backward == 0 else (g["img2"], g["img1"])
    df.load_pair(a, b)
    df.generisi()
    assert np.array_equal(df.bestlabels.cpu().numpy(), g[k + "labels00"])
    assert np.array_equal(df.vratiKonacniFlow().cpu().numpy(), g[k + "flow00"])
    df.nasumicni()
    st = df.host_state()
    assert np.array_equal(st["nprop"], g[k + "nprop"])
    assert np.array_equal(st["proposals"][:2], g[k + "proposals_rows"])
    assert np.array_equal(st["lcosts"][:2], g[k + "lcosts_rows"])
    # the reference's packedksets file (pakovanje): GPU bit matrices + host replay of its border scratch reuse
    pk = pkg("compat").packedksets(df)
    assert np.array_equal(pk[1, 1], g[k + "packedksets_px"])
    assert hashlib.sha256(pk.tobytes()).hexdigest() == str(g[k + "packedksets_sha"])
    if name == "a40x48_c5x6" and backward == 0:         # pakovanjeZaC (dopython=0) of the same pass
        ge = golden("extras")
        for j, arr in enumerate(pkg("compat").pakovani_za_c(pk)):
            assert hashlib.sha256(arr.tobytes()).hexdigest() == str(ge["za_c%d_sha" % j])
    for w in range(1, int(g["bcd_times"]) + 1):
        df.ceoBCD(1)
        assert np.array_equal(df.bestlabels.cpu().numpy(), g[k + "labels%02d" % w]), "sweep %d" % w


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_fb_consistency_matches_reference_golden(torch_, golden, name):
    g = golden(name)
    pl = pkg("pipeline")
    flows = []
    for backward in (0, 1):
        df = make(int(g["H"]), int(g["W"]), int(g["cellh"]), int(g["cellw"]), seed=int(g["seed"]))
        a, b = (g["img1"], g["img2"]) if backward == 0 else (g["img2"], g["img1"])
        flows.append(df.run(a, b, int(g["bcd_times"])).clone())
    for t in (1, 3):
        got = pl.fb_consistency(flows[0], flows[1], t).cpu().numpy()
        assert np.array_equal(got, g["sparse_t%d" % t])


def test_bcd_from_uploaded_reference_state(torch_, oracle, synth):
    """ucitajSvePodatkeDoBCD path: state produced on the CPU, uploaded in the reference's dtypes, swept on the GPU."""
    H, W, ch, cw = 48, 64, 8, 8
    O = oracle
    img1, img2, _ = synth.make_pair(H, W, seed=77, amp_x=6, amp_y=4)
    p = O.make_params(H, W, ch, cw, seed=5)
    r = O.full_pass(p, img1, img2, 0)
    df = make(H, W, ch, cw, seed=5)
    df.set_host_state(r["proposals"], r["lcosts"], r["nprop"], r["bestlabels"])
    bl = r["bestlabels"].copy()
    for w in range(3):
        df.ceoBCD(1)
        O.bcd_sweep(p, r["proposals"], r["lcosts"], r["nprop"], bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl)


@pytest.mark.parametrize("geom", [(45, 70, 7, 9), (96, 128, 12, 16)])
def test_batched_sweeps_equal_separate_sweeps(torch_, oracle, synth, geom):
    """dflow_bcd_sweep_batch: the chains of several independent passes (forward and backward run of two pairs) in one
    launch per phase give the labels of separate calls, which are the oracle's."""
    H, W, ch, cw = geom
    O = oracle
    pl = pkg("pipeline")
    passes, refs = [], []
    for k in range(5):                      # 5 passes: forward/backward of pair 0 and 1, forward of pair 2
        img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(k // 2, 0), amp_x=0.08 * W, amp_y=0.08 * H)
        if k % 2:
            img1, img2 = img2, img1
        df = make(H, W, ch, cw, seed=k)
        df.load_pair(img1, img2); df.generisi(); df.nasumicni()
        passes.append(df)
        refs.append(O.full_pass(O.make_params(H, W, ch, cw, seed=k), img1, img2, 3)["bestlabels"])
    pl.ceoBCD_batch(passes, 3)
    for k, df in enumerate(passes):
        assert np.array_equal(df.bestlabels.cpu().numpy(), refs[k]), "pass %d" % k


def test_full_size_sintel_whole_frame_matches_oracle(torch_, oracle, synth):
    """BASELINE config 2 geometry (1024x436, 64x27 cells, ragged last cell row), EVERY pixel against the oracle (16 threads,
    about 10 s): proposals / costs / counts / WTA labels after generisi (446 464 x 125 exact 5-NN indices), the neighbour
    stage, one whole BCD sweep; plus the invariants of the layout."""
    H, W = 436, 1024
    O = oracle
    O.set_threads(16)
    try:
        img1, img2, gt = synth.make_pair(H, W, seed=2022)
        df = make(H, W, seed=99)
        p = oracle_params(O, df)
        assert (p.cellh, p.cellw) == (27, 64)
        df.load_pair(img1, img2)
        d1, d2 = O.daisy(img1), O.daisy(img2)
        assert np.array_equal(df.descrs1.cpu().numpy().view(np.uint32), d1.view(np.uint32))
        assert np.array_equal(df.descrs2.cpu().numpy().view(np.uint32), d2.view(np.uint32))
        df.generisi()
        st = df.host_state()
        pr, lc, npr, bl = O.knn_proposals(p, d1, d2)                          # the whole frame on the CPU
        assert np.array_equal(st["nprop"], npr)
        assert np.array_equal(st["proposals"], pr), "bit-exact kNN candidate indices, every pixel"
        assert np.array_equal(st["lcosts"], lc)
        assert np.array_equal(st["bestlabels"], bl)
        ncx, ncy = W // p.cellw, H // p.cellh
        cy = np.minimum(np.arange(H) // p.cellh, ncy - 1); cx = np.minimum(np.arange(W) // p.cellw, ncx - 1)
        wy = np.minimum(cy + 2, ncy - 1) - np.maximum(cy - 2, 0) + 1
        wx = np.minimum(cx + 2, ncx - 1) - np.maximum(cx - 2, 0) + 1
        assert np.array_equal(npr, 5 * wy[:, None] * wx[None, :])                 # nprop = 5 x window cells
        assert np.all(bl < npr) and np.all(bl >= 0)
        lab = np.arange(p.maxnprop)[None, None, :]
        assert np.all(pr[lab[..., None].repeat(2, -1) >= npr[..., None, None]] == -1)   # -1 fill beyond nprop
        assert np.all(lc[lab >= npr[..., None]] == 1000.0)
        # every proposal lands inside the image and inside the +-2-cell window
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ty = yy[..., None] + pr[..., 0]; tx = xx[..., None] + pr[..., 1]
        valid = lab < npr[..., None]
        assert np.all((ty >= 0) & (ty < H) & (tx >= 0) & (tx < W) | ~valid)
        tcy = np.minimum(ty // p.cellh, ncy - 1); tcx = np.minimum(tx // p.cellw, ncx - 1)
        assert np.all((np.abs(tcy - cy[:, None, None]) <= 2) & (np.abs(tcx - cx[None, :, None]) <= 2) | ~valid)
        # WTA label = first minimum of the costs
        assert np.array_equal(bl, np.argmin(np.where(valid, lc, np.inf), axis=-1))
        # neighbour stage and one full BCD sweep
        df.nasumicni()
        O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
        df.ceoBCD(1)
        O.bcd_sweep(p, pr, lc, npr, bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl)
    finally:
        O.set_threads(1)


def test_low_texture_whole_frame_matches_oracle(torch_, oracle, synth):
    """The reference reads real KITTI frames (daisy i flann.py:26-27) and its DAISY is un-normalised (:66): saturated sky
    and flat road give exactly-zero and near-equal descriptors over large areas, which smoothed noise never does.  The
    "low_texture" style of synth.py has them (31 % saturated, 24 % a +-2 grey level road band, a blurred box, a pattern that
    repeats every 16 px).  Whole 1024x436 frame against the oracle on 16 threads: every kNN index / cost / count / WTA
    label, the neighbour stage, one sweep -- and the screen must have done it itself: no list handed to the brute-force
    kernel, the duplicate zero rows removed, the all-zero queries answered from their cells' lists, event count bounded
    (round 3: this frame sent the WHOLE pass to knn_fix_kernel, 81 ms instead of 0.2)."""
    H, W = 436, 1024
    O = oracle
    O.set_threads(16)
    try:
        img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(0, 0), style="low_texture")
        reg = synth.low_texture_regions(H, W, synth.pair_seed(0, 0))
        assert (reg == 1).mean() > 0.28 and (reg == 2).mean() > 0.2
        df = make(H, W, seed=99)
        p = oracle_params(O, df)
        df.load_pair(img1, img2)
        d1, d2 = O.daisy(img1), O.daisy(img2)
        assert np.array_equal(df.descrs1.cpu().numpy().view(np.uint32), d1.view(np.uint32))
        assert np.array_equal(df.descrs2.cpu().numpy().view(np.uint32), d2.view(np.uint32))
        nzero1, nzero2 = int((~d1.any(-1)).sum()), int((~d2.any(-1)).sum())
        assert nzero1 > 0.2 * H * W and nzero2 > 0.2 * H * W              # the saturated sky really is all-zero DAISY
        df.generisi()
        stats = df.knn_stats()
        st = df.host_state()
        pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
        assert np.array_equal(st["nprop"], npr)
        assert np.array_equal(st["proposals"], pr), "bit-exact kNN candidate indices, every pixel"
        assert np.array_equal(st["lcosts"], lc)
        assert np.array_equal(st["bestlabels"], bl)
        assert stats["flags"] == 0 and stats["lists_exact"] == 0, stats     # nothing went to the brute-force kernel
        assert stats["zero_queries"] == nzero1 and stats["zero_candidates"] == nzero2, stats
        assert stats["zero_candidates_removed"] >= nzero2 - 5 * 256, stats     # at most 5 zero rows stay per cell
        assert stats["max_entries_per_lane"] < stats["list_capacity"], stats
        assert stats["events_per_query_cell"] < 12.0, stats                    # measured 7.65 (dense texture: 5.76)
        # the queries in the fringes of the flat regions (hundreds of near-ties per cell) went to the one-wave-per-query kernel
        assert 0 < stats["heavy_pairs"] < 1 << 20, stats                       # measured 172 825 of 9.5 M (query, cell) pairs
        df.nasumicni()
        O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
        df.ceoBCD(1)
        O.bcd_sweep(p, pr, lc, npr, bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl)
    finally:
        O.set_threads(1)


def test_low_texture_kitti_fp16_planes_match_exact_kernel(torch_, synth):
    """The same frame content at BASELINE configs[4]'s geometry (1242x375, cells 54x25, binary16 planes): MFMA-screened search
    against the brute-force kernel, every pixel, and again no list for the brute-force kernel inside the screened run."""
    torch = torch_
    L = pkg("_lib")
    H, W = 375, 1242
    img1, img2, _ = synth.make_pair(H, W, seed=3, style="low_texture")
    df = pkg("pipeline").DiscreteFlow(H, W, 25, 54, seed=1, flags=L.FLAG_DESCR_F16)
    df.load_pair(img1, img2)
    df.generisi()
    stats = df.knn_stats()
    screened = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
    assert stats["flags"] == 0 and stats["lists_exact"] == 0 and stats["zero_queries"] > 0.2 * H * W, stats
    df.p.flags = L.FLAG_DESCR_F16 | L.FLAG_KNN_EXACT
    df.generisi()
    for a, b, name in zip(screened, (df.proposals, df.lcosts, df.nprop, df.bestlabels), ("proposals", "lcosts", "nprop", "bestlabels")):
        assert torch.equal(a, b), name


def test_knn_lists_with_rows_outside_the_screen_go_to_the_exact_kernel_one_by_one(torch_, synth):
    """A descriptor the f16 rows cannot hold (|64 d|^2 beyond KM_NORM2_MAX, inf, NaN-free) costs the lists it takes part in,
    not the pass: one such query -> the 25 lists of its 64-query wave; one such candidate -> the lists of the query waves
    that have its cell in their window.  Results equal the brute-force kernel's."""
    L = pkg("_lib")
    H, W, ch, cw = 96, 128, 12, 16
    img1, img2, _ = synth.make_pair(H, W, seed=5, amp_x=8, amp_y=6)
    df = make(H, W, ch, cw)
    df.load_pair(img1, img2)
    d1, d2 = df.descrs1.clone(), df.descrs2.clone()

    def both(a, b):
        out = []
        for mode in (0, L.FLAG_KNN_EXACT):
            df.p.flags = mode
            df.set_descriptors(a, b)
            df.generisi()
            if mode == 0:
                stats = df.knn_stats()
            out.append(df.host_state())
        df.p.flags = 0
        for k in out[0]:
            assert np.array_equal(out[0][k], out[1][k]), k
        return stats

    base = both(d1, d2)
    assert base["lists_exact"] == 0 and base["flags"] == 0
    q = d1.clone(); q[H // 2, W // 2, 7] = 2000.0                   # one query far outside the range
    s1 = both(q, d2)
    assert s1["flags"] == 0 and s1["bad_queries"] == 1 and 0 < s1["lists_exact"] <= 25, s1
    c = d2.clone(); c[H // 2 + 1, W // 2 + 3, 11] = float("inf")     # one candidate: every list against its cell
    s2 = both(d1, c)
    waves_per_cell = (ch * cw + 63) // 64
    assert s2["flags"] == 0 and 0 < s2["lists_exact"] <= 25 * waves_per_cell, s2


def test_per_list_fallback_at_bench_size(torch_, synth):
    """The per-LIST fallback at BASELINE size: 40 candidate pixels and 40 query pixels of the bench pair get a value the f16 rows
    cannot hold; the lists they take part in (tens of thousands of the 198 400) go to knn_fix_kernel one by one, the rest
    of the frame is screened as usual, and the whole frame equals the brute-force kernel's result (round 3 would have sent the
    WHOLE pass to the brute-force kernel: one flag for the frame)."""
    torch = torch_
    L = pkg("_lib")
    H, W = 436, 1024
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(1, 0))
    df = make(H, W, seed=0)
    df.load_pair(img1, img2)
    g = torch.Generator(device="cpu").manual_seed(5)
    d1, d2 = df.descrs1.clone(), df.descrs2.clone()
    for d in (d1, d2):
        ys = torch.randint(0, H, (40,), generator=g); xs = torch.randint(0, W, (40,), generator=g); ks = torch.randint(0, 68, (40,), generator=g)
        d[ys, xs, ks] = 3000.0
    out = {}
    for mode in (0, L.FLAG_KNN_EXACT):
        df.p.flags = mode
        df.set_descriptors(d1, d2)
        df.generisi()
        if mode == 0:
            stats = df.knn_stats()
        out[mode] = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
    df.p.flags = 0
    for a, b, name in zip(out[0], out[L.FLAG_KNN_EXACT], ("proposals", "lcosts", "nprop", "bestlabels")):
        assert torch.equal(a, b), name
    assert stats["flags"] == 0 and stats["bad_queries"] == 40, stats
    assert 1000 < stats["lists_exact"] < 0.25 * stats["lists"], stats          # lists, not the pass


def test_descriptor_storage_mode_is_fixed_at_construction(torch_):
    """Flipping DFLOW_FLAG_DESCR_F16 on an existing object would make the kernels use 272-byte rows in 144-byte planes (or
    the reverse): the wrapper refuses."""
    L = pkg("_lib")
    df = make(48, 64, 8, 8)
    df.p.flags = L.FLAG_DESCR_F16
    with pytest.raises(L.DflowError):
        df.generisi()
    df.p.flags = L.FLAG_KNN_EXACT                                      # other flags may change per call
    df._pp()
    dh = pkg("pipeline").DiscreteFlow(48, 64, 8, 8, flags=L.FLAG_DESCR_F16)
    dh.p.flags = 0
    with pytest.raises(L.DflowError):
        dh.generisi()


def _window_mask(gt, ch, cw, window=2):
    """Pixels whose ground-truth target lies inside the image and inside the +-2-cell search window (daisy i flann.py:167-168)."""
    H, W, _ = gt.shape
    ncx, ncy = W // cw, H // ch
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ty = np.rint(yy + gt[..., 0]).astype(np.int64); tx = np.rint(xx + gt[..., 1]).astype(np.int64)
    inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
    cy = np.minimum(yy // ch, ncy - 1); cx = np.minimum(xx // cw, ncx - 1)
    tcy = np.minimum(np.clip(ty, 0, H - 1) // ch, ncy - 1); tcx = np.minimum(np.clip(tx, 0, W - 1) // cw, ncx - 1)
    return inside & (np.abs(tcy - cy) <= window) & (np.abs(tcx - cx) <= window)


def test_full_frame_knn_mfma_equals_exact_at_bench_size(torch_, synth):
    """BASELINE configs[1] geometry, every pixel: the MFMA-screened search and the brute-force kernel (DFLOW_FLAG_KNN_EXACT)
    must agree on all of proposals, lcosts, nprop and bestlabels (446 464 x 125 exact 5-NN indices, bit for bit)."""
    torch = torch_
    H, W = 436, 1024
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))       # the bench's first pair
    df = make(H, W, seed=0)
    df.load_pair(img1, img2)
    out = {}
    for mode in (0, pkg("_lib").FLAG_KNN_EXACT):
        df.p.flags = mode
        df.generisi()
        out[mode] = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
    df.p.flags = 0
    for a, b, name in zip(out[0], out[pkg("_lib").FLAG_KNN_EXACT], ("proposals", "lcosts", "nprop", "bestlabels")):
        assert torch.equal(a, b), name


def test_bench_config_four_sweeps_match_oracle_and_epe(torch_, oracle, synth):
    """BASELINE configs[1] exactly (1024x436, cells 64x27, bcd_times=4): labels after each of the 4 sweeps equal the oracle's
    (run on the GPU's own proposals: the kNN stage has its own full-frame test above), and the end-point error against the
    synthetic ground truth (synth.forward_gt: the true flow of image 1's pixels).  Measured on this pair after 4 sweeps, GPU and
    oracle alike: over the pixels whose ground truth is reachable (target inside the image and the +-2-cell window, 96 % of
    the frame) mean 2.41 px, median 0.81 px, 5.8 % > 3 px (sweep 0, WTA only: 30.4 / 1.06 / 32 %); over all pixels 4.83 /
    0.84 / 8.6 % -- the unreachable border band is a property of the search window.  Thresholds = those values x 1.25.
    (Round 1's "median 2.0 px" compared against the warp field sampled at the source pixel instead of the true forward
    flow, an error of |grad g| |g| = several px in the ground truth itself; see synth.forward_gt.)"""
    H, W = 436, 1024
    O = oracle
    O.set_threads(16)
    try:
        img1, img2, gt = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
        df = make(H, W, seed=0)
        p = oracle_params(O, df)
        df.load_pair(img1, img2)
        df.generisi()
        df.nasumicni()
        st = df.host_state()
        pr, lc, npr, bl = st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"]
        for w in range(4):
            df.ceoBCD(1)
            O.bcd_sweep(p, pr, lc, npr, bl)
            assert np.array_equal(df.bestlabels.cpu().numpy(), bl), "sweep %d" % (w + 1)
        flow = df.vratiKonacniFlow().cpu().numpy().astype(np.float64)
        assert np.array_equal(flow, O.labels_to_flow(p, pr, bl))          # EPE delta vs the oracle is exactly 0
        epe = np.sqrt(((flow - gt) ** 2).sum(-1))
        m = _window_mask(gt, p.cellh, p.cellw)
        print("EPE all: mean %.3f median %.3f >3px %.2f%% | reachable (%.1f%% of px): mean %.3f median %.3f >3px %.2f%%"
              % (epe.mean(), np.median(epe), (epe > 3).mean() * 100, m.mean() * 100, epe[m].mean(), np.median(epe[m]), (epe[m] > 3).mean() * 100))
        assert m.mean() > 0.5
        assert epe[m].mean() < EPE_REACHABLE_MEAN_MAX and (epe[m] > 3).mean() * 100 < EPE_REACHABLE_OUTLIER_PCT_MAX
        assert np.median(epe[m]) < EPE_REACHABLE_MEDIAN_MAX
    finally:
        O.set_threads(1)


def test_kitti_config5_as_stated_matches_oracle(torch_, oracle, synth):
    """BASELINE configs[4] as one configuration: 1242x375, cells 54x25 (discrete_flow.py:22-23,30-31), fp16 DAISY
    descriptors (DFLOW_FLAG_DESCR_F16), MFMA-screened kNN, bcd_times=8.  The oracle runs on its own descriptors rounded by
    numpy's float16 (round to nearest even); every stage of the whole frame is compared: descriptors, proposals / costs /
    counts / labels after generisi and after nasumicni, labels after each of the 8 sweeps."""
    H, W, ch, cw = 375, 1242, 25, 54
    O = oracle
    L = pkg("_lib")
    O.set_threads(16)
    try:
        img1, img2, _ = synth.make_pair(H, W, seed=H + W + 1)
        df = pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=4, flags=L.FLAG_DESCR_F16)
        assert df.descrs1.dtype == torch_.float16 and df.descrs1.shape[-1] == 72          # real half-width descriptor planes
        p = oracle_params(O, df)
        df.load_pair(img1, img2)
        d1 = O.daisy(img1).astype(np.float16).astype(np.float32)
        d2 = O.daisy(img2).astype(np.float16).astype(np.float32)
        assert np.array_equal(df.descriptors_f32(0).cpu().numpy().view(np.uint32), d1.view(np.uint32))
        assert np.array_equal(df.descriptors_f32(1).cpu().numpy().view(np.uint32), d2.view(np.uint32))
        df.generisi()
        pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr)
        assert np.array_equal(st["lcosts"], lc) and np.array_equal(st["bestlabels"], bl)
        df.nasumicni()
        O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
        for w in range(8):
            df.ceoBCD(1)
            O.bcd_sweep(p, pr, lc, npr, bl)
            assert np.array_equal(df.bestlabels.cpu().numpy(), bl), "sweep %d" % (w + 1)
    finally:
        O.set_threads(1)


def test_full_hd_frame_matches_oracle(torch_, oracle, synth):
    """The largest frame the design is sized for (1920x1080 in 18.6 GB of workspace), cells of 30x40 px (the
    bench's 64x27 grid): every stage of the whole frame against the oracle -- proposals / costs / counts / labels after
    generisi and after nasumicni, labels after each of 2 sweeps.  The reference hard-codes 1241x375 (daisy i flann.py:34-35);
    SURVEY Q12 asks the build to generalise, the oracle defines the result."""
    H, W, ch, cw = 1080, 1920, 40, 30
    O = oracle
    O.set_threads(16)
    try:
        img1, img2, _ = synth.make_pair(H, W, seed=1080)
        df = make(H, W, ch, cw, seed=11)
        assert df.ws_bytes < 20 * 2 ** 30
        p = oracle_params(O, df)
        df.load_pair(img1, img2)
        d1, d2 = O.daisy(img1), O.daisy(img2)
        df.generisi()
        pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr)
        assert np.array_equal(st["lcosts"], lc) and np.array_equal(st["bestlabels"], bl)
        df.nasumicni()
        O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
        st = df.host_state()
        assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
        del st
        for w in range(2):
            df.ceoBCD(1)
            O.bcd_sweep(p, pr, lc, npr, bl)
            assert np.array_equal(df.bestlabels.cpu().numpy(), bl), "sweep %d" % (w + 1)
    finally:
        O.set_threads(1)


@pytest.mark.parametrize("geom", [(375, 1241, 25, 73), (375, 1242, 25, 54)])
def test_kitti_geometries_sampled(torch_, oracle, synth, geom):
    """BASELINE configs 1 and 5 geometries (daisy i flann.py:34-43, discrete_flow.py:22-31): invariants, sampled exact
    kNN searches and one full BCD sweep against the oracle."""
    H, W, ch, cw = geom
    O = oracle
    img1, img2, _ = synth.make_pair(H, W, seed=H + W)
    df = make(H, W, ch, cw, seed=3)
    p = oracle_params(O, df)
    df.load_pair(img1, img2)
    d1, d2 = df.descrs1.cpu().numpy(), df.descrs2.cpu().numpy()
    df.generisi()
    st = df.host_state()
    pr, lc, npr, bl = st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"]
    ncx, ncy = W // cw, H // ch
    cy = np.minimum(np.arange(H) // ch, ncy - 1); cx = np.minimum(np.arange(W) // cw, ncx - 1)
    wy = np.minimum(cy + 2, ncy - 1) - np.maximum(cy - 2, 0) + 1
    wx = np.minimum(cx + 2, ncx - 1) - np.maximum(cx - 2, 0) + 1
    assert np.array_equal(npr, 5 * wy[:, None] * wx[None, :])
    valid = np.arange(p.maxnprop)[None, None, :] < npr[..., None]
    assert np.array_equal(bl, np.argmin(np.where(valid, lc, np.inf), axis=-1))
    rng = np.random.default_rng(7)
    for _ in range(12):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        slot = 0
        for ci in range(max(0, cx[x] - 2), min(ncx - 1, cx[x] + 2) + 1):
            for cj in range(max(0, cy[y] - 2), min(ncy - 1, cy[y] + 2) + 1):
                idx, _ = O.knn_cell(p, d1[y, x], d2, ci, cj)
                cwid = (W if ci == ncx - 1 else (ci + 1) * cw) - ci * cw
                want = np.stack([cj * ch + idx // cwid - y, ci * cw + idx % cwid - x], -1)
                assert np.array_equal(pr[y, x, slot:slot + 5], want), (y, x, ci, cj)
                slot += 5
    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    st = df.host_state()
    assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
    df.ceoBCD(1)
    O.bcd_sweep(p, pr, lc, npr, bl)
    assert np.array_equal(df.bestlabels.cpu().numpy(), bl)


def test_knn_mfma_path_equals_exact_kernel(torch_, synth, monkeypatch):
    """The MFMA-screened search and the brute-force VALU kernel (DFLOW_FLAG_KNN_EXACT) give identical outputs, also for
    descriptors DAISY never produces (negative values) and where the screen has to hand the whole pass back to the exact
    fix-up kernel (values outside the f16 range, NaN-free)."""
    H, W, ch, cw = 96, 128, 12, 16
    img1, img2, _ = synth.make_pair(H, W, seed=5, amp_x=8, amp_y=6)
    df = make(H, W, ch, cw)
    df.load_pair(img1, img2)

    def run(mode, d1, d2):
        df.p.flags = pkg("_lib").FLAG_KNN_EXACT if mode else 0
        df.set_descriptors(d1, d2)
        df.generisi()
        return df.host_state()

    d1, d2 = df.descrs1.clone(), df.descrs2.clone()
    a, b = run(None, d1, d2), run("exact", d1, d2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    d1n = d1 - 0.01
    a, b = run(None, d1n, d2), run("exact", d1n, d2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # one value far outside the range of the f16 rows -> the lists of its query wave go to the fix-up kernel
    d1n = d1.clone(); d1n[H // 2, W // 2, 7] = 2000.0
    a, b = run(None, d1n, d2), run("exact", d1n, d2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", ("quantised", "tiny", "offset", "constant", "mixed_scale", "sparse"))
def test_knn_mfma_screen_is_exact_on_hard_descriptors(torch_, synth, monkeypatch, case):
    """The f16 screen must never lose an exact neighbour: descriptor sets that stress its error bound (exact ties, f16
    subnormals, a large common offset, identical rows, 1000:1 scale differences between dimensions, mostly-zero rows)
    against the brute-force kernel, bit for bit."""
    torch = torch_
    H, W, ch, cw = 72, 96, 12, 16
    img1, img2, _ = synth.make_pair(H, W, seed=17, amp_x=6, amp_y=5)
    df = make(H, W, ch, cw)
    df.load_pair(img1, img2)
    d1, d2 = df.descrs1.clone(), df.descrs2.clone()
    g = torch.Generator(device="cpu").manual_seed(3)
    if case == "quantised":              # values on a coarse grid: many exactly equal distances -> index tie-breaks
        d1, d2 = torch.round(d1 * 64) / 64, torch.round(d2 * 64) / 64
    elif case == "tiny":                 # 64 x lands in the f16 subnormal range
        d1, d2 = d1 * 1e-5, d2 * 1e-5
    elif case == "offset":               # large common component, small differences
        d1, d2 = d1 + 3.0, d2 + 3.0
    elif case == "constant":             # all candidates identical: every distance ties
        d2 = d2[:1, :1].expand_as(d2).contiguous()
    elif case == "mixed_scale":
        sc = torch.logspace(-2, 1, 68).to(d1.device)
        d1, d2 = d1 * sc, d2 * sc
    elif case == "sparse":
        m = (torch.rand(d2.shape, generator=g) < 0.1).to(d1.device)
        d1, d2 = d1 * m, d2 * m

    def run(mode):
        df.p.flags = pkg("_lib").FLAG_KNN_EXACT if mode else 0
        df.set_descriptors(d1, d2)
        df.generisi()
        return df.host_state()
    a, b = run(None), run("exact")
    for k in a:
        assert np.array_equal(a[k], b[k]), (case, k)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_knn_mfma_screen_on_mixed_scale_rows(torch_, synth, seed):
    """What low-texture frames do to the screen, exaggerated: per-PIXEL scales from 1e-7 to 2 (rows of a cell that differ by
    seven orders of magnitude: fringes of flat regions next to texture), 15 % all-zero rows in both images, and exact
    duplicates of non-zero rows among the candidates (ties that the index must break).  MFMA-screened search against the
    brute-force kernel, bit for bit, and no list may have gone to the brute-force kernel inside the screened run."""
    torch = torch_
    L = pkg("_lib")
    H, W, ch, cw = 96, 128, 12, 16
    img1, img2, _ = synth.make_pair(H, W, seed=40 + seed, amp_x=8, amp_y=6)
    df = make(H, W, ch, cw)
    df.load_pair(img1, img2)
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = []
    for base in (df.descrs1.clone(), df.descrs2.clone()):
        scale = torch.pow(10.0, torch.rand((H, W, 1), generator=g) * 7.3 - 7.0).to(base.device)
        zero = (torch.rand((H, W, 1), generator=g) < 0.15).to(base.device)
        d.append(torch.where(zero, torch.zeros_like(base), base * scale))
    d1, d2 = d
    # duplicates among the candidates: every fourth pixel repeats its left neighbour's row
    d2[:, 1::4] = d2[:, 0:-1:4][:, :d2[:, 1::4].shape[1]]
    out = []
    for mode in (0, L.FLAG_KNN_EXACT):
        df.p.flags = mode
        df.set_descriptors(d1, d2)
        df.generisi()
        if mode == 0:
            stats = df.knn_stats()
        out.append(df.host_state())
    df.p.flags = 0
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert stats["flags"] == 0 and stats["lists_exact"] == 0, stats
    assert stats["zero_queries"] > 0.1 * H * W and stats["zero_candidates_removed"] > 0, stats


def test_large_frame_invariants(torch_, oracle, synth):
    """1920x1080 (2.07 Mpx, 36 GB workspace): 64-bit offsets everywhere, structural invariants and sampled parity with the
    oracle's exact search; guards against 32-bit index arithmetic that the benchmark sizes cannot reach."""
    torch = torch_
    H, W = 1080, 1920
    img1, img2, _ = synth.make_pair(H, W, seed=31, amp_x=30.0, amp_y=20.0)
    df = make(H, W)
    p = oracle_params(oracle, df)
    df.load_pair(img1, img2)
    df.generisi()
    g = dict(ch=df.p.cellh, cw=df.p.cellw, ncx=W // df.p.cellw, ncy=H // df.p.cellh)

    def labels_of(y, x):         # (150,2) int [dy,dx] of one pixel, without converting the whole 5 GB state
        packed = df.proposals[y, x, :150].cpu().numpy().view(np.uint32)
        return np.stack([(packed & 0xFFFF).astype(np.uint16).view(np.int16), (packed >> 16).astype(np.uint16).view(np.int16)], -1).astype(np.int64)
    cy = np.minimum(np.arange(H) // g["ch"], g["ncy"] - 1); cx = np.minimum(np.arange(W) // g["cw"], g["ncx"] - 1)
    wy = np.minimum(g["ncy"] - 1, cy + 2) - np.maximum(0, cy - 2) + 1
    wx = np.minimum(g["ncx"] - 1, cx + 2) - np.maximum(0, cx - 2) + 1
    assert np.array_equal(df.nprop.cpu().numpy(), 5 * wy[:, None] * wx[None, :])
    # sampled exact searches (bottom-right corner cell included: the largest offsets)
    d1 = df.descrs1.cpu().numpy(); d2 = df.descrs2.cpu().numpy()
    rng = np.random.default_rng(1)
    for (y, x) in [(H - 1, W - 1), (0, 0), (H // 2, W // 2)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(5)]:
        qcj, qci = int(cy[y]), int(cx[x])
        mine = labels_of(y, x)
        slot = 0
        for ci in range(max(0, qci - 2), min(g["ncx"] - 1, qci + 2) + 1):
            for cj in range(max(0, qcj - 2), min(g["ncy"] - 1, qcj + 2) + 1):
                idx, _ = oracle.knn_cell(p, d1[y, x], d2, ci, cj)
                x0, y0 = ci * g["cw"], cj * g["ch"]
                cwid = (W if ci == g["ncx"] - 1 else x0 + g["cw"]) - x0
                exp = np.stack([y0 + idx // cwid - y, x0 + idx % cwid - x], -1)
                assert np.array_equal(mine[slot:slot + 5], exp), (y, x, ci, cj)
                slot += 5
    df.nasumicni()
    df.ceoBCD(1)
    bl = df.bestlabels.cpu().numpy(); npr = df.nprop.cpu().numpy()
    assert (bl >= 0).all() and (bl < npr).all() and npr.max() <= 150
    flow = df.vratiKonacniFlow().cpu().numpy()
    assert np.isfinite(flow).all() and np.abs(flow[..., 0]).max() <= 3 * g["ch"] + 25 and np.abs(flow[..., 1]).max() <= 3 * g["cw"] + 25


@pytest.mark.parametrize("over", [dict(tpsi=5, tphi=1.5, lamda=0.1, ngauss=10, sigma=4.0),
                                  dict(tpsi=1, tphi=0.75, lamda=1.0, ngauss=25, sigma=8.0, maxnprop=160),
                                  dict(tpsi=8, tphi=2.5, lamda=0.05, ngauss=0, window=1),
                                  dict(tpsi=8, tphi=2.5, lamda=0.05, ngauss=25, window=0, maxnprop=40)])
def test_non_default_constants_match_oracle(torch_, oracle, synth, over):
    """The module globals of the reference (tpsi, tphi, lamda, ngauss, sigma, maxnprop, window) are parameters of the ABI:
    other values than the reference's go through the same kernels and must agree with the oracle stage by stage."""
    O = oracle
    H, W, ch, cw = 60, 84, 10, 12
    img1, img2, _ = synth.make_pair(H, W, seed=99, amp_x=7.0, amp_y=5.0)
    df = pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=21, **over)
    p = O.make_params(H, W, ch, cw, seed=21, **over)
    df.load_pair(img1, img2)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    df.generisi()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    st = df.host_state()
    assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
    for sweep in range(2):
        df.ceoBCD(1)
        O.bcd_sweep(p, pr, lc, npr, bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl), (over, sweep)
    with pytest.raises(pkg("_lib").DflowError):
        pkg("pipeline").DiscreteFlow(H, W, ch, cw, tpsi=9)


def _random_geometries(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        ch, cw = int(rng.integers(3, 20)), int(rng.integers(3, 24))
        ncy, ncx = int(rng.integers(1, 8)), int(rng.integers(1, 9))
        H, W = max(24, ch * ncy + int(rng.integers(0, ch))), max(24, cw * ncx + int(rng.integers(0, cw)))
        window, ngauss = int(rng.integers(0, 3)), int(rng.choice([0, 7, 25]))
        out.append((H, W, ch, cw, window, ngauss))
    return out


@pytest.mark.parametrize("geom", _random_geometries(10, 7))
def test_random_geometries_match_oracle(torch_, oracle, synth, geom):
    """Randomly drawn image sizes, cell sizes (down to 3x9 pixels, ragged last cells, single-row cell grids) and windows
    (0..2): kNN proposals, neighbour proposals and one BCD sweep against the oracle, bit for bit (scratch/fuzz_geoms.py (round 3, git history) runs
    more of them)."""
    O = oracle
    H, W, ch, cw, window, ngauss = geom
    over = dict(window=window, ngauss=ngauss, maxnprop=5 * (2 * window + 1) ** 2 + ngauss)
    df = pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=H + W, **over)
    p = O.make_params(H, W, ch, cw, seed=H + W, **over)
    img1, img2, _ = synth.make_pair(H, W, seed=100 + H, amp_x=0.08 * W, amp_y=0.08 * H)
    df.load_pair(img1, img2)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    df.generisi()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    st = df.host_state()
    for k, v in (("nprop", npr), ("proposals", pr), ("lcosts", lc), ("bestlabels", bl)):
        assert np.array_equal(st[k], v), (geom, "knn", k)
    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    st = df.host_state()
    for k, v in (("nprop", npr), ("proposals", pr), ("lcosts", lc)):
        assert np.array_equal(st[k], v), (geom, "neighbour", k)
    df.ceoBCD(1)
    O.bcd_sweep(p, pr, lc, npr, bl)
    assert np.array_equal(df.bestlabels.cpu().numpy(), bl), (geom, "sweep")


def test_cli_end_to_end(torch_, oracle, synth, tmp_path, monkeypatch):
    """The two drop-in CLIs on a synthetic pair: file names, dtypes and contents as the reference writes them."""
    import runpy, sys, os
    from conftest import ROOT, PKG
    O = oracle
    H, W, ch, cw = 48, 64, 8, 8
    monkeypatch.chdir(tmp_path)
    # no --packedksets: like the reference (daisy i flann.py:308,430) the default writes the file (this frame is far below the size limit)
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "6", "0", "1", "--synthetic", "%dx%d" % (H, W), "--cell", "%dx%d" % (ch, cw), "--seed", "11"])
    runpy.run_path(os.path.join(ROOT, PKG, "daisy i flann.py"), run_name="__main__")
    monkeypatch.setattr(sys, "argv", ["python bcd.py", "6", "0", "2", "--cell", "%dx%d" % (ch, cw)])
    runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="__main__")
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(6, 0))
    ref = O.full_pass(O.make_params(H, W, ch, cw, seed=11), img1, img2, 2)
    prop = np.load("Daisy output slike 106 backward=0 proposals_nakon_gausa.npy")
    assert prop.dtype == np.int64 and prop.shape == (H, W, 150, 2) and np.array_equal(prop, ref["proposals"])
    lc = np.load("Daisy output slike 106 backward=0 lcosts_nakon_gausa.npy")
    assert lc.dtype == np.float64 and np.array_equal(lc, ref["lcosts"])
    assert np.array_equal(np.load("Daisy output slike 106 backward=0 nprop.npy"), ref["nprop"])
    pk = np.load("Daisy output slike 106 backward=0 packedksets.npy")
    assert pk.dtype == np.uint8 and np.array_equal(pk, O.pack_compat(O.make_params(H, W, ch, cw, seed=11), ref["proposals"], ref["nprop"]))
    for w in range(3):
        f = np.load("Gotova flow slika 106 backward=0 posle %02d BCD.npy" % w)
        assert f.dtype == np.float64 and np.array_equal(f, ref["flows"][w])
        flo = pkg("flowio").read_flo("Gotova flow slika 106 backward=0 posle %02d BCD.flo" % w)
        assert np.array_equal(flo, f[..., ::-1].astype(np.float32))
    assert np.array_equal(np.load("Bestlabels fajl slike 106 backward=0 posle 02 BCD.npy"), ref["bestlabels"])
    # dopython=0 (daisy i flann.py:423-426): pakovanjeZaC's four scan-order files instead of packedksets
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "6", "0", "0", "--synthetic", "%dx%d" % (H, W), "--cell", "%dx%d" % (ch, cw), "--seed", "11", "--packedksets"])
    runpy.run_path(os.path.join(ROOT, PKG, "daisy i flann.py"), run_name="__main__")
    for k, want in enumerate(pkg("compat").pakovani_za_c(pk)):
        got = np.load("Daisy output slike 106 backward=0 pakovani za c %d.npy" % k)
        assert got.dtype == np.uint8 and np.array_equal(got, want), k


def test_batch_driver_config3(torch_, oracle, synth, tmp_path):
    """BASELINE config 3 through the batch driver on one GPU: forward + backward + consistency, outputs on disk."""
    import os
    rb = pkg("run_batch")
    H, W = 48, 64
    rb.main(["--pairs", "1", "--bcd-times", "2", "--size", "%dx%d" % (H, W), "--thresh", "3", "--out", str(tmp_path)])
    O = oracle
    img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(0, 0))
    ch, cw = pkg("pipeline").default_cells(H, W)
    p = O.make_params(H, W, ch, cw, seed=0)
    fwd = O.full_pass(p, img1, img2, 2)["flows"][-1]
    bwd = O.full_pass(p, img2, img1, 2)["flows"][-1]
    got = np.load(os.path.join(tmp_path, "sparse_field_00.npy"))
    assert np.array_equal(got, O.fb_consistency(fwd, bwd, 3))
    assert np.array_equal(np.load(os.path.join(tmp_path, "Gotova flow slika 100 backward=1 posle 02 BCD.npy")), bwd)
    assert os.path.getsize(os.path.join(tmp_path, "parovi_00.txt")) > 0


def test_bench_contract(torch_, tmp_path):
    """bench.py prints ONE JSON line with the driver's keys, the roofline object (the kernel with the larger measured time per
    step of knn_screen_kernel / bcd_chain_kernel, both carried, + per-stage fractions), the one-pair latency, one-GPU timings of
    BASELINE configs[2] and [4], the CPU baseline (whole bench pair + the configs[0] geometry + the single-thread sample) and the EPE of
    the GPU flow and of the oracle's flow on the bench pair (difference exactly 0), all of which --full adds to the headline; run as
    a child process, as the driver does."""
    import json, os, subprocess, sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=1500, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "epe", "epe_delta_vs_oracle"):
        assert k in d, k
    assert d["metric"].startswith("Mpix/s") and d["unit"] == "Mpix/s" and d["n_gpus"] == 1 and d["steps"] == 3
    assert d["vs_baseline"] is None and d["scaling"] == "weak" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 436 * 1024 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    # the headline object is the kernel with the larger measured time per step; both candidates are carried
    ks = r["kernels"]
    assert set(ks) == {"knn_screen_kernel", "bcd_chain_kernel"}
    assert r["kernel"] == max(ks, key=lambda k: ks[k]["ms_per_step"])
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert r[k] == ks[r["kernel"]][k]
    c, sc = ks["bcd_chain_kernel"], ks["knn_screen_kernel"]
    assert c["bound"] == "hbm" and c["unit"] == "GB/s" and c["peak"] == 8000.0
    assert sc["bound"] == "mfma" and sc["unit"] == "TFLOP/s" and sc["peak"] == 2500.0
    assert 1.0 <= sc["issued_over_algorithmic"] < 1.9 and sc["launch_ms"] > 0
    for k in (c, sc):
        assert abs(k["frac"] - k["achieved"] / k["peak"]) < 1e-12 and 0 < k["frac"] < 1
        assert k["traffic"] is None or k["traffic"] > 0
    assert set(("daisy", "knn", "bcd", "end_to_end")) <= set(r["stages"])
    assert d["latency_ms_single_pair"] == r["stages"]["ms_total"] > d["ms_per_step"] * 0.5
    oc = d["other_configs"]
    assert oc["configs[2]"]["passes"] == 2 and oc["configs[2]"]["ms"] > 0
    assert oc["configs[4] geometry"]["dtype"].startswith("f16 descriptors") and oc["configs[4] geometry"]["ms_per_pass"] > 0
    assert oc["1920x1080"]["passes"] == 2 and oc["1920x1080"]["ms_per_pass"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["unit"] == "Mpix/s" and 0 < c["value"] < d["value"]
    assert len(c["entries"]) == 3 and c["entries"][2]["threads"] == 1 and "1241x375" in c["entries"][1]["config"]
    assert sum(e["seconds"] for e in c["entries"]) < 40
    assert d["epe_delta_vs_oracle"] == 0.0 and d["epe"]["flow_fields_identical"] is True
    assert d["epe"]["gpu"]["all_pixels"] == d["epe"]["oracle"]["all_pixels"]


def test_bench_two_ranks_rehearsal(torch_, tmp_path):
    """`python bench.py --gpus 2` end to end on the one-GPU box: the launcher starts two ranks, both drive device 0
    (--rehearse-on-one-gpu: gloo instead of RCCL, which cannot host two ranks on one device) through the batch engine, the
    flow fields are gathered on rank 0 after every step, rank 0 prints ONE JSON line with n_gpus = 2."""
    import json, os, subprocess, sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                          "--batch", "2", "--front", "2", "--full", "--no-cpu-baseline", "--rehearse-on-one-gpu"],
                         capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    assert abs(d["value"] - 2 * 436 * 1024 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    assert d["config"]["mode"] == "batch" and d["roofline"]["kernel"] in ("bcd_chain_kernel", "knn_screen_kernel")


def test_bench_dump_outputs_is_the_last_timed_step(torch_, oracle, synth, tmp_path):
    """--dump-outputs writes the flow the LAST timed step returned (4 steps in groups of 2: step 3 = resident pair 1, the
    second pass of the second batched group), every pixel equal to the oracle's pass over that pair; --steps alone sets
    the timed steps (no extra long region in the line)."""
    import json, os, subprocess, sys
    from conftest import ROOT
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--batch", "2",
                          "--no-cpu-baseline", "--no-other-configs", "--fixed-batch", "0", "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][0])
    assert d["steps"] == 4 and not any(k.startswith(("ms_per_step_", "value_")) for k in d)
    assert "config" in d and not set(d) & {"roofline", "latency_ms_single_pair", "epe", "fixed_batch"}     # no --full
    assert sorted(os.listdir(dump)) == ["flow.npy"]
    got = np.load(dump / "flow.npy")
    assert got.dtype == np.float32 and got.shape == (436, 1024, 2)
    O = oracle
    O.set_threads(16)
    try:
        img1, img2, _ = synth.make_pair(436, 1024, seed=synth.pair_seed(1, 0))
        ref = O.full_pass(O.make_params(436, 1024, 27, 64, seed=0), img1, img2, 4)
    finally:
        O.set_threads(1)
    assert np.array_equal(got.astype(np.float64), ref["flows"][-1])


def test_cli_kitti_png_branch(torch_, oracle, synth, tmp_path, monkeypatch):
    """The reference's own input path (daisy i flann.py:19-27,34-35,52-53): 8-bit PNGs under
    ../data_scene_flow/training/image_2/0001<idx>_1{0,1}.png, cropped to 1241x375 at (0,0), cells 73x25; backward swaps the
    two frames.  KITTI itself is absent, so the PNGs are a synthetic 1242x375 pair written with PIL; the files the CLI
    writes must equal the oracle's state on the cropped frames (whole frame, 16 threads)."""
    import runpy, sys, os
    from PIL import Image
    from conftest import ROOT, PKG
    O = oracle
    img1, img2, _ = synth.make_pair(375, 1242, seed=synth.pair_seed(6, 0))
    d = tmp_path / "data_scene_flow" / "training" / "image_2"
    d.mkdir(parents=True)
    Image.fromarray(np.ascontiguousarray(img1[..., ::-1])).save(str(d / "000106_10.png"))     # BGR -> RGB on disk
    Image.fromarray(np.ascontiguousarray(img2[..., ::-1])).save(str(d / "000106_11.png"))
    work = tmp_path / "work"
    work.mkdir()
    monkeypatch.chdir(work)
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "6", "1", "1", "--seed", "5"])      # backward run
    runpy.run_path(os.path.join(ROOT, PKG, "daisy i flann.py"), run_name="__main__")
    a, b = img2[:375, :1241], img1[:375, :1241]                                               # backward: pic1 = _11, pic2 = _10
    O.set_threads(16)
    try:
        p = O.make_params(375, 1241, 25, 73, seed=5)
        ref = O.full_pass(p, np.ascontiguousarray(a), np.ascontiguousarray(b), 0)
    finally:
        O.set_threads(1)
    prop = np.load("Daisy output slike 106 backward=1 proposals_nakon_gausa.npy")
    assert prop.shape == (375, 1241, 150, 2) and prop.dtype == np.int64 and np.array_equal(prop, ref["proposals"])
    assert np.array_equal(np.load("Daisy output slike 106 backward=1 lcosts_nakon_gausa.npy"), ref["lcosts"])
    assert np.array_equal(np.load("Daisy output slike 106 backward=1 nprop.npy"), ref["nprop"])
    assert np.array_equal(np.load("Gotova flow slika 106 backward=1 posle 00 BCD.npy"), ref["flows"][0])


def test_integration_stub_runs_as_written(torch_, oracle, synth, tmp_path, monkeypatch):
    """INTEGRATION.md section 2 is the binding a maintainer of the reference would paste next to `daisy i flann.py`: the code
    block is executed here VERBATIM (only the library path is made absolute) with the module globals the reference has at
    that point (pich, picw, cellh, cellw, pic3, pic4, bcd_times, picindex, backward, wstr, con_tresh), and the .npy it saves
    must be the oracle's flow."""
    import os, re
    from conftest import ROOT, PKG
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"```python\n(# dflow_binding.py.*?)```", text, re.S).group(1)
    block = block.replace('C.CDLL("libdflow.so")', 'C.CDLL(%r)' % os.path.join(ROOT, PKG, "csrc", "libdflow.so"))
    H, W, ch, cw = 48, 64, 8, 8
    img1, img2, _ = synth.make_pair(H, W, seed=4, amp_x=6, amp_y=4)
    monkeypatch.chdir(tmp_path)
    zeros = torch_.zeros((H, W, 2), dtype=torch_.float32, device="cuda:0")
    ns = dict(pich=H, picw=W, cellh=ch, cellw=cw, pic3=img1, pic4=img2, bcd_times=2, picindex="06", backward="0", wstr="02",
              con_tresh=10.0, flow_fwd=zeros, flow_bwd=zeros)
    exec(compile(block, "INTEGRATION.md", "exec"), ns)
    torch_.cuda.synchronize()
    got = np.load("Gotova flow slika 106 backward=0 posle 02 BCD.npy")
    ref = oracle.full_pass(oracle.make_params(H, W, ch, cw, seed=0), img1, img2, 2)
    assert got.dtype == np.float64 and np.array_equal(got, ref["flows"][-1])
    assert tuple(ns["sparse"].shape) == (H, W, 3)


def test_baseline_config0_as_one_run(torch_, oracle, synth, tmp_path, monkeypatch):
    """BASELINE configs[0] as the reference's README runs it (README.md:25-37): `daisy i flann.py 6 0 1` then
    `python bcd.py 6 0 1` on the KITTI-layout PNG pair 000106_10/_11 (forward, dopython=1, bcd_times=1), 1241x375 with
    cells 73x25, the second CLI reading the files the first one wrote (python bcd.py:13-17,67-81).  KITTI itself is
    absent: the PNGs are a synthetic 1242x375 pair in the low-texture style (sky, road, blur, pattern).  The `posle 01`
    flow and label files (python bcd.py:282-283) must equal the oracle's whole-frame result (16 threads)."""
    import runpy, sys, os
    from PIL import Image
    from conftest import ROOT, PKG
    O = oracle
    img1, img2, _ = synth.make_pair(375, 1242, seed=synth.pair_seed(6, 0), style="low_texture")
    d = tmp_path / "data_scene_flow" / "training" / "image_2"
    d.mkdir(parents=True)
    Image.fromarray(np.ascontiguousarray(img1[..., ::-1])).save(str(d / "000106_10.png"))     # BGR -> RGB on disk
    Image.fromarray(np.ascontiguousarray(img2[..., ::-1])).save(str(d / "000106_11.png"))
    work = tmp_path / "work"
    work.mkdir()
    monkeypatch.chdir(work)
    monkeypatch.setattr(sys, "argv", ["daisy i flann.py", "6", "0", "1", "--seed", "3"])
    runpy.run_path(os.path.join(ROOT, PKG, "daisy i flann.py"), run_name="__main__")
    monkeypatch.setattr(sys, "argv", ["python bcd.py", "6", "0", "1"])
    runpy.run_path(os.path.join(ROOT, PKG, "python bcd.py"), run_name="__main__")
    a, b = np.ascontiguousarray(img1[:375, :1241]), np.ascontiguousarray(img2[:375, :1241])    # daisy i flann.py:52-53
    O.set_threads(16)
    try:
        ref = O.full_pass(O.make_params(375, 1241, 25, 73, seed=3), a, b, 1)
    finally:
        O.set_threads(1)
    assert np.array_equal(np.load("Daisy output slike 106 backward=0 proposals_nakon_gausa.npy"), ref["proposals"])
    assert np.array_equal(np.load("Daisy output slike 106 backward=0 lcosts_nakon_gausa.npy"), ref["lcosts"])
    assert np.array_equal(np.load("Daisy output slike 106 backward=0 nprop.npy"), ref["nprop"])
    for w in (0, 1):
        f = np.load("Gotova flow slika 106 backward=0 posle %02d BCD.npy" % w)
        assert f.dtype == np.float64 and f.shape == (375, 1241, 2) and np.array_equal(f, ref["flows"][w]), w
        flo = pkg("flowio").read_flo("Gotova flow slika 106 backward=0 posle %02d BCD.flo" % w)
        assert np.array_equal(flo, f[..., ::-1].astype(np.float32))
    lab = np.load("Bestlabels fajl slike 106 backward=0 posle 01 BCD.npy")
    assert lab.dtype == np.int64 and np.array_equal(lab, ref["bestlabels"])


@pytest.mark.parametrize("case", ("all_compatible", "ties", "sparse_labels", "mixed_lengths"))
def test_bcd_adversarial_label_sets_match_oracle(torch_, oracle, case):
    """Hand-made states uploaded in the reference's dtypes (ucitajSvePodatkeDoBCD path) that drive the chain kernel through
    its rare branches: every label compatible with every label of the neighbour (150-member lists: second / third blocks
    and the 160-bit rows for every label), exact cost ties everywhere (first-index rules, Q9-Q11), pixels with very few
    labels next to full ones, and lists of every length 0..40 side by side.  Labels after every phase of two sweeps must
    equal the oracle's."""
    O = oracle
    H, W, ch, cw = 40, 44, 8, 11
    rng = np.random.default_rng({"all_compatible": 1, "ties": 2, "sparse_labels": 3, "mixed_lengths": 4}[case])
    L = 150
    proposals = np.full((H, W, L, 2), -1, np.int64)
    lcosts = np.full((H, W, L), 1000.0, np.float64)
    nprop = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if case == "all_compatible":          # all flows inside a 3x3 box: |d|_1 <= 4 < tpsi for every pair
                n = 150
                f = rng.integers(-1, 2, size=(n, 2))
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            elif case == "ties":                  # few distinct flows and costs: ties in every minimum
                n = int(rng.integers(100, 151))
                f = rng.integers(-6, 7, size=(n, 2)) * np.array([1, 2])
                c = rng.choice(np.array([0.5, 1.0, 2.5], np.float32), n)
            elif case == "sparse_labels":
                n = int(rng.choice([1, 2, 5, 150]))
                f = rng.integers(-30, 31, size=(n, 2))
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            else:                                 # clusters of growing size: list lengths 0..40
                n = 150
                f = np.zeros((n, 2), np.int64)
                k = 0; cl = 0
                while k < n:
                    m = min(n - k, cl % 41 + 1)
                    f[k:k + m] = np.array([40 * (cl % 7) - 120, 30 * (cl // 7) - 60]) + rng.integers(-1, 2, size=(m, 2))
                    k += m; cl += 1
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            proposals[y, x, :n] = f
            lcosts[y, x, :n] = c.astype(np.float64)
            nprop[y, x] = n
    bestlabels = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            bestlabels[y, x] = rng.integers(0, nprop[y, x])
    df = make(H, W, ch, cw, seed=1)
    p = O.make_params(H, W, ch, cw, seed=1)
    df.set_host_state(proposals, lcosts, nprop, bestlabels)
    bl = bestlabels.copy()
    for sweep in range(2):
        for phase in range(4):
            df.bcd_phase(phase)
            O.bcd_phase(p, proposals, lcosts, nprop, bl, phase)
            assert np.array_equal(df.bestlabels.cpu().numpy(), bl), (case, sweep, phase)


def test_fp16_descriptor_mode_matches_oracle(torch_, oracle, synth):
    """BASELINE configs[4] names "fp16 DAISY descriptors": DFLOW_FLAG_DESCR_F16 rounds every descriptor value to binary16
    (values stay in float32 storage).  DAISY must equal the oracle's descriptors rounded the same way (numpy float16, round
    to nearest even), and the rest of the path (MFMA-screened exact kNN, costs, neighbour stage, two sweeps) must equal the
    oracle run on those rounded descriptors."""
    O = oracle
    L = pkg("_lib")
    H, W, ch, cw = 60, 84, 10, 12
    img1, img2, _ = synth.make_pair(H, W, seed=31, amp_x=7.0, amp_y=5.0)
    df = pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=9, flags=L.FLAG_DESCR_F16)
    p = O.make_params(H, W, ch, cw, seed=9)
    df.load_pair(img1, img2)
    d1 = O.daisy(img1).astype(np.float16).astype(np.float32)
    d2 = O.daisy(img2).astype(np.float16).astype(np.float32)
    assert df.descrs1.dtype == torch_.float16 and tuple(df.descrs1.shape) == (H, W, 72)      # half-width storage, 144-byte rows
    assert np.array_equal(df.descrs1[..., :68].cpu().numpy().view(np.uint16), O.daisy(img1).astype(np.float16).view(np.uint16))
    assert not df.descrs1[..., 68:].any() and not df.descrs2[..., 68:].any()
    assert np.array_equal(df.descriptors_f32(0).cpu().numpy().view(np.uint32), d1.view(np.uint32))
    assert np.array_equal(df.descriptors_f32(1).cpu().numpy().view(np.uint32), d2.view(np.uint32))
    # the brute-force kernel reads the same planes: its results must equal the MFMA-screened ones
    df.p.flags = L.FLAG_DESCR_F16 | L.FLAG_KNN_EXACT
    df.generisi()
    exact = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
    df.p.flags = L.FLAG_DESCR_F16
    df.generisi()
    for a_, b_ in zip(exact, (df.proposals, df.lcosts, df.nprop, df.bestlabels)):
        assert torch_.equal(a_, b_)
    assert not np.array_equal(d1, O.daisy(img1))                     # the mode does change the values
    df.generisi()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    st = df.host_state()
    assert np.array_equal(st["nprop"], npr) and np.array_equal(st["proposals"], pr) and np.array_equal(st["lcosts"], lc)
    for sweep in range(2):
        df.ceoBCD(1)
        O.bcd_sweep(p, pr, lc, npr, bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl), sweep
