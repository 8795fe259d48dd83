"""Every stage at the edges of what dflow_check_params (csrc/abi.hip) accepts, against the CPU oracle bit for bit.

The rest of the GPU suite builds its parameters from dflow_default_params with a few overrides: label_pitch 160, frames of 24 px
and more, cells of 9 points and more, a few thousand points per cell, max_attempts 65536, seeds below 2^32.  The cases here run
the values at the other ends of the accepted ranges, where code exists that nothing else reaches:

* frames down to 8 x 8 and cells of 5 points, 1 px wide or tall (DAISY border clamps, tiles with 5 real rows);
* label pitches 16 .. 160 on both sides of the 64- and 128-label groups of the BCD kernels;
* chains of 8192 pixels (75 904 B of LDS per chain workgroup);
* a cell of 65 535 points (the last MFMA-screened size, uint16 candidate indices) and one of 65 536 (the brute-force kernel);
* the sampler's max_attempts bound, a saturated threshold table, a seed with a non-zero high word;
* batches of more than BCD_MAX_BATCH = 8 passes;
* forward-backward consistency on a frame with an edge of 8 px, targets on and just past every border, errors equal to tresh.

Stage by stage means: DAISY (u32 view), kNN proposals / lcosts / nprop / WTA labels, neighbour proposals, compat.packedksets,
the labels after every phase of two sweeps and the final flow.  Before each kNN call the outputs are filled with garbage, and
after kNN and after the neighbour stage the slots nprop..label_pitch of the raw tensors must hold the ABI's fill values
(include/dflow.h: 0xFFFFFFFF, 1000.0f), so that a slot no kernel writes shows up.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "f16")
OUTPUTS = ("proposals", "lcosts", "nprop", "bestlabels")
FILL_PROPOSAL, FILL_COST = 0xFFFFFFFF, np.float32(1000.0)


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture
def O(oracle):
    oracle.set_threads(16)
    try:
        yield oracle
    finally:
        oracle.set_threads(1)


def stored(d, storage):
    """What the descriptor planes hold: binary16 planes round every value (numpy float16 = torch's rounding)."""
    return d.astype(np.float16).astype(np.float32) if storage == "f16" else d


def new_pass(H, W, ch, cw, storage="f32", seed=0, **over):
    L = pkg("_lib")
    flags = L.FLAG_DESCR_F16 if storage == "f16" else 0
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed, flags=flags, **over)


def oracle_params(O, df):
    """The oracle's parameters for a pass: everything but label_pitch and flags, which it does not have."""
    p = df.p
    keys = ("maxnprop", "knn", "window", "ngauss", "tpsi", "max_attempts", "tphi", "sigma", "lamda")
    return O.make_params(p.pich, p.picw, p.cellh, p.cellw, seed=p.seed, **{k: getattr(p, k) for k in keys})


def poison(df):
    """Garbage in every output slot before a kNN call (the workspace is left alone)."""
    df.proposals.fill_(0x7FFF7FFF)
    df.lcosts.fill_(float("nan"))
    df.nprop.fill_(-1)
    df.bestlabels.fill_(-1)


def assert_fill(df, what):
    """include/dflow.h: the slots nprop..label_pitch of proposals and lcosts hold 0xFFFFFFFF and 1000.0f."""
    LP = df.p.label_pitch
    nprop = df.nprop.cpu().numpy()
    assert (nprop >= 0).all() and (nprop <= df.p.maxnprop).all(), what
    unused = np.arange(LP)[None, None, :] >= nprop[..., None]
    prop = df.proposals.cpu().numpy().view(np.uint32)
    lc = df.lcosts.cpu().numpy()
    assert (prop[unused] == FILL_PROPOSAL).all(), (what, "proposals fill")
    assert (lc[unused].view(np.uint32) == FILL_COST.view(np.uint32)).all(), (what, "lcosts fill")


def assert_state(df, ref, keys, what):
    st = df.host_state()
    for k, v in zip(OUTPUTS, ref):
        if k in keys:
            assert np.array_equal(st[k], v), (what, k)


def stages(O, synth, df, sweeps=2, img_seed=0, amp=0.1, pack=True):
    """DAISY -> kNN -> neighbour proposals -> packedksets -> every phase of `sweeps` sweeps -> flow, each against the oracle.
    Returns the oracle's state after the sweeps."""
    H, W = df.p.pich, df.p.picw
    storage = "f16" if df.descr_f16 else "f32"
    p = oracle_params(O, df)
    img1, img2, _ = synth.make_pair(H, W, seed=img_seed, amp_x=amp * W, amp_y=amp * H)
    df.load_pair(img1, img2)
    d1, d2 = stored(O.daisy(img1), storage), stored(O.daisy(img2), storage)
    for i, d in enumerate((d1, d2)):
        assert np.array_equal(df.descriptors_f32(i).cpu().numpy().view(np.uint32), d.view(np.uint32)), ("daisy", i)

    poison(df)
    df.generisi()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    assert_state(df, (pr, lc, npr, bl), OUTPUTS, "knn")
    assert_fill(df, "knn")
    flow0 = df.vratiKonacniFlow().cpu().numpy().astype(np.float64)
    assert np.array_equal(flow0, O.labels_to_flow(p, pr, bl)), "knn flow"

    df.nasumicni()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    assert_state(df, (pr, lc, npr, bl), ("proposals", "lcosts", "nprop"), "neighbour")
    assert_fill(df, "neighbour")

    if pack:
        assert np.array_equal(pkg("compat").packedksets(df), O.pack_compat(p, pr, npr)), "packedksets"

    for sweep in range(sweeps):
        for phase in range(4):
            df.bcd_phase(phase)
            O.bcd_phase(p, pr, lc, npr, bl, phase)
            assert np.array_equal(df.bestlabels.cpu().numpy(), bl), ("bcd", sweep, phase)
    assert np.array_equal(df.vratiKonacniFlow().cpu().numpy().astype(np.float64), O.labels_to_flow(p, pr, bl)), "final flow"
    return pr, lc, npr, bl


# ------------------------------------------------------------------------------------------------ 1. smallest frames

SMALL = [((8, 8, 8, 8), {}, "f32"),
         ((8, 8, 1, 5), {}, "f32"),
         ((9, 13, 5, 1), {}, "f32"),
         ((8, 23, 1, 5), {}, "f32"),
         ((11, 17, 2, 3), {}, "f32"),
         ((11, 17, 2, 3), {}, "f16"),
         ((23, 8, 5, 2), dict(window=1, ngauss=64, maxnprop=109), "f32")]


@pytest.mark.parametrize("geom,over,storage", SMALL, ids=["8x8_c8x8", "8x8_c1x5", "9x13_c5x1", "8x23_c1x5", "11x17_c2x3",
                                                          "11x17_c2x3_f16", "23x8_w1_ng64"])
def test_smallest_frames_and_thinnest_cells(torch_, O, synth, geom, over, storage):
    """Frames at the 8-px floor, where DAISY's 17-point grid (radius 5) and its smoothing stencils are wider than the frame and
    every read goes through the border clamps of daisy.hip; cells of 5 to 9 points, 1 px wide or tall, whose 32-row kNN tiles
    (knn_prep_kernel) hold 5 real rows and whose top 5 is almost the whole cell; ragged last cells that absorb the remainder.
    23 x 8 with window 1, ngauss 64, maxnprop 109: the largest sampler (64 x 128 x 4 = 32 KB of neighbour_kernel's dynamic
    LDS, the most draws of one thread kept there)."""
    H, W, ch, cw = geom
    df = new_pass(H, W, ch, cw, storage, seed=H * W, **over)
    stages(O, synth, df, img_seed=H + 3 * W)


# ------------------------------------------------------------------------------------------------ 2. label pitch

PITCHES = [(0, 0, 5, 16, "f32"), (1, 0, 45, 48, "f32"), (1, 7, 52, 64, "f32"), (1, 25, 70, 80, "f32"),
           (2, 0, 125, 128, "f32"), (2, 7, 132, 144, "f32"), (2, 7, 132, 144, "f16"),
           (1, 0, 45, 160, "f32"), (2, 0, 125, 144, "f32")]


@pytest.mark.parametrize("window,ngauss,maxnprop,lp,storage", PITCHES,
                         ids=["%d_%d_%d_lp%d_%s" % c for c in PITCHES])
def test_label_pitch_on_both_sides_of_the_label_groups(torch_, O, synth, window, ngauss, maxnprop, lp, storage):
    """label_pitch LP below 160: bcd_lists_kernel builds its compat masks in groups of 64 labels and emits the second group only
    for LP > 64 and the fifth (labels 128..159) only for LP > 128 with a pixel above 128 labels; bcd_chain_kernel's threads
    LP..191 are shadow lanes (`owner = tid < LP`); knn_finalize_kernel fills n..LP in steps of 16 lanes; pack_compat_kernel
    reads rows of LP and packs matrices of maxnprop.  The tight pairs sit just above and below 64 and 128 labels, the slack
    ones leave 35 and 19 unused slots per pixel, which the fill checks cover."""
    H, W, ch, cw = 60, 84, 10, 12
    df = new_pass(H, W, ch, cw, storage, seed=21 + lp, window=window, ngauss=ngauss, maxnprop=maxnprop, label_pitch=lp)
    assert tuple(df.proposals.shape) == (H, W, lp)
    stages(O, synth, df, img_seed=99, amp=0.08)


# ------------------------------------------------------------------------------------------------ 3. longest chains

@pytest.mark.parametrize("geom", [(8, 8192, 8, 32), (8192, 8, 32, 8)], ids=["8x8192", "8192x8"])
def test_longest_chains(torch_, O, synth, geom):
    """Chains of 8192 pixels (rows of 8 x 8192 in phases 1 and 3, columns of 8192 x 8 in phases 0 and 2): bcd_chain_kernel's
    dynamic LDS is 8 * len + 16 = 65 552 B (launch_bcd_phase_batch), on top of 10 352 B of static LDS: 75 904 B per workgroup,
    above 64 KiB (gfx950 has 160 KiB per CU).  The traceback walks 256 chunks of BCD_TB_STEPS.  A full pass and two sweeps,
    phase by phase."""
    H, W, ch, cw = geom
    df = new_pass(H, W, ch, cw, seed=77)
    stages(O, synth, df, img_seed=5, amp=0.004)


# ------------------------------------------------------------------------------------------------ 4. largest cells

def screen_stats_rc(df):
    """dflow_knn_screen_stats' return code (DFLOW_EINVAL where the MFMA screen does not run)."""
    import torch
    out = (C.c_int64 * 13)()
    stream = C.c_void_p(torch.cuda.current_stream(df.device).cuda_stream)
    return pkg("_lib").lib().dflow_knn_screen_stats(C.byref(df.p), df.ws.data_ptr(), df.ws_bytes, stream, out)


def check_sampled_queries(O, df, d1, d2, pixels):
    """The 5 proposals of sampled pixels of a one-cell frame against oracle.knn_cell.  Returns the highest index expected."""
    H, W = df.p.pich, df.p.picw
    p = oracle_params(O, df)
    top = 0
    for (y, x) in pixels:
        packed = df.proposals[y, x, :5].cpu().numpy().view(np.uint32)
        got = np.stack([(packed & 0xFFFF).astype(np.uint16).view(np.int16),
                        (packed >> 16).astype(np.uint16).view(np.int16)], -1).astype(np.int64)
        idx, _ = O.knn_cell(p, d1[y, x], d2, 0, 0)
        exp = np.stack([idx // W - y, idx % W - x], -1)
        assert np.array_equal(got, exp), (y, x, got.tolist(), exp.tolist())
        top = max(top, int(idx.max()))
    return top


def sample_pixels(d1, H, W, seed):
    """The last row of pixels, the bottom-right corner (whose nearest neighbours have the highest indices under small motion),
    the first pixel and random ones; all-zero DAISY rows (in the bottom corners) are kept: they take the zero-query path."""
    rng = np.random.default_rng(seed)
    pix = [(H - 1, x) for x in (0, 1, W // 2, W - 3, W - 2, W - 1)]
    pix += [(H - 1 - dy, W - 1 - dx) for dy in (1, 3, 6) for dx in (0, 2, 5)]
    pix += [(0, 0)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(24)]
    return pix


@pytest.mark.parametrize("storage", STORAGES)
def test_largest_mfma_cell(torch_, O, synth, storage):
    """255 x 257 as one cell: 65 535 points = KM_MAXPTS, the last size knn_mfma_supported accepts.  The cell pads to 342 chunks
    = 2 052 tiles; km_event_cand decodes tile rows to indices up to 65 663, which the uint16 lists of knn_resolve_kernel and
    knn_resolve_heavy_kernel would wrap onto real candidates if a padded row ever gave an event.  The screen must run (stats
    flags 0), equal the brute-force kernel on the whole frame and the oracle on sampled queries, the last row of pixels and the
    bottom-right corner included."""
    torch = torch_
    H, W = 255, 257
    L = pkg("_lib")
    img1, img2, _ = synth.make_pair(H, W, seed=41, amp_x=1.5, amp_y=1.0)
    d1, d2 = stored(O.daisy(img1), storage), stored(O.daisy(img2), storage)
    df = new_pass(H, W, H, W, storage, seed=3)
    df.set_descriptors(d1, d2)
    poison(df)
    df.generisi()
    stats = df.knn_stats()
    print(storage, stats)
    assert stats["flags"] == 0 and stats["bad_queries"] == 0, stats
    assert stats["query_cell_pairs"] == H * W, stats
    assert_fill(df, "knn")
    assert (df.nprop == 5).all()
    screened = [t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]
    top = check_sampled_queries(O, df, d1, d2, sample_pixels(d1, H, W, seed=1))
    assert top >= H * W - 2 * W, top                     # the samples reach the last rows of the cell
    df.p.flags |= L.FLAG_KNN_EXACT
    poison(df)
    df.generisi()
    for k, a, b in zip(OUTPUTS, screened, (df.proposals, df.lcosts, df.nprop, df.bestlabels)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_first_cell_beyond_the_mfma_screen(torch_, O, synth):
    """256 x 256 as one cell: 65 536 points, one more than the uint16 indices of the screen hold.  knn_mfma_supported refuses it,
    dflow_knn_proposals runs the brute-force kernel (dflow_knn_screen_stats answers DFLOW_EINVAL: the screen did not run), and
    sampled queries must equal the oracle."""
    H, W = 256, 256
    img1, img2, _ = synth.make_pair(H, W, seed=43, amp_x=1.5, amp_y=1.0)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    df = new_pass(H, W, H, W, seed=4)
    df.set_descriptors(d1, d2)
    poison(df)
    df.generisi()
    assert screen_stats_rc(df) == -1                     # DFLOW_EINVAL
    assert_fill(df, "knn")
    top = check_sampled_queries(O, df, d1, d2, sample_pixels(d1, H, W, seed=2))
    assert top >= H * W - 2 * W, top


# ------------------------------------------------------------------------------------------------ 5. sampler limits

@pytest.mark.parametrize("extra", (0, 3))
def test_sampler_max_attempts_bound(torch_, O, synth, extra):
    """max_attempts = ngauss and ngauss + 3 on 16 x 16 (sigma 3): neighbour_kernel's `att < max_attempts` ends the draws of the
    pixels whose draws leave the frame too often.  The bound must cut some pixels and not all (the oracle's draw counts with
    and without it tell which), one draw more must change the oracle's proposals (an off-by-one in the bound shows), and every
    stage must equal the oracle."""
    H, W, ch, cw = 16, 16, 4, 4
    over = dict(ngauss=25, sigma=3.0, max_attempts=25 + extra)
    df = new_pass(H, W, ch, cw, seed=3, **over)
    stages(O, synth, df, img_seed=5)
    img1, img2, _ = synth.make_pair(H, W, seed=5, amp_x=0.1 * W, amp_y=0.1 * H)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    att, props = [], []
    for ma in (over["max_attempts"], over["max_attempts"] + 1, 1 << 16):
        p = O.make_params(H, W, ch, cw, seed=3, ngauss=25, sigma=3.0, max_attempts=ma)
        pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
        att.append(O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl, want_attempts=True))
        props.append(pr)
    cut = att[2] > over["max_attempts"]
    assert cut.any() and not cut.all(), int(cut.sum())
    assert np.array_equal(att[0], np.minimum(att[2], over["max_attempts"]))
    assert not np.array_equal(props[0], props[1])


def test_sampler_saturated_threshold_table(torch_, O, synth):
    """sigma = 0.25: gauss_thresholds saturates (every threshold below offset -1 is 0, every one above +1 is 2^32 - 1), so
    nearly every draw lands on the pixel itself and is a duplicate of its own WTA label."""
    H, W, ch, cw = 24, 32, 6, 8
    df = new_pass(H, W, ch, cw, seed=17, sigma=0.25)
    thr = O.gauss_thresholds(0.25)
    assert (thr[:62] == 0).all() and (thr[65:] == 0xFFFFFFFF).all()
    p = oracle_params(O, df)
    img1, img2, _ = synth.make_pair(H, W, seed=8, amp_x=0.1 * W, amp_y=0.1 * H)
    pr, lc, npr, bl = O.knn_proposals(p, O.daisy(img1), O.daisy(img2))
    n_knn = npr.copy()
    O.neighbour_proposals(p, O.daisy(img1), O.daisy(img2), pr, lc, npr, bl)
    assert (npr - n_knn).mean() < 1.0 and (npr > n_knn).any()
    stages(O, synth, df, img_seed=8)


def test_sampler_seed_high_word(torch_, O, synth):
    """seed = 0x9E3779B97F4A7C15: the Philox key word k1 = seed >> 32 (launch_neighbour) is non-zero.  Its proposals must equal
    the oracle's and differ from those of 0x7F4A7C15, the same low word with a zero high word."""
    H, W, ch, cw = 24, 32, 6, 8
    seed = 0x9E3779B97F4A7C15
    df = new_pass(H, W, ch, cw, seed=seed)
    assert df.p.seed == seed
    high = stages(O, synth, df, img_seed=12)
    low = new_pass(H, W, ch, cw, seed=seed & 0xFFFFFFFF)
    p = oracle_params(O, low)
    img1, img2, _ = synth.make_pair(H, W, seed=12, amp_x=0.1 * W, amp_y=0.1 * H)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    low.load_pair(img1, img2)
    low.generisi()
    low.nasumicni()
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    assert_state(low, (pr, lc, npr, bl), ("proposals", "lcosts", "nprop"), "neighbour, low word only")
    assert not np.array_equal(high[0], pr)                 # the sweeps leave the proposals as the neighbour stage made them


# ------------------------------------------------------------------------------------------------ 6. batches over 8 passes

@pytest.mark.parametrize("npass", (9, 17))
def test_batches_of_more_than_eight_passes(torch_, O, synth, npass):
    """ceoBCD_batch with 9 and 17 passes: launch_bcd_phase_batch splits them into launches of BCD_MAX_BATCH = 8 (the last one
    ragged: 1 pass), each launch taking the passes from b0 on.  Every pass (pair k // 2, direction k % 2, seed k) must equal its
    own oracle run after two sweeps."""
    H, W, ch, cw = 24, 40, 6, 8
    pl = pkg("pipeline")
    passes, refs = [], []
    for k in range(npass):
        img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(k // 2, 0), amp_x=0.08 * W, amp_y=0.08 * H)
        if k % 2:
            img1, img2 = img2, img1
        df = new_pass(H, W, ch, cw, seed=k)
        df.load_pair(img1, img2); df.generisi(); df.nasumicni()
        passes.append(df)
        refs.append(O.full_pass(oracle_params(O, df), img1, img2, 2))
    pl.ceoBCD_batch(passes, 2)
    for k, (df, ref) in enumerate(zip(passes, refs)):
        assert np.array_equal(df.bestlabels.cpu().numpy(), ref["bestlabels"]), "pass %d" % k
        assert np.array_equal(df.vratiKonacniFlow().cpu().numpy().astype(np.float64), ref["flows"][-1]), "pass %d flow" % k
    assert len({r["bestlabels"].tobytes() for r in refs}) == npass          # every pass has labels of its own


# ------------------------------------------------------------------------------------------------ 7. fb consistency

def test_fb_consistency_on_an_edge_frame(torch_, O):
    """fb_consistency_kernel on 8 x 8192 with integer flows: targets exactly on -1, 0, H-1, H (rows, where the transposed
    indexing of postprocessing.py adds U = dx) and -1, 0, W-1, W (columns), and backward flows that make the error exactly
    tresh = 5 (3-4-5 triangles, 0-5) on some pixels and just above it on others: the test is a strict `>`."""
    torch = torch_
    H, W, tresh = 8, 8192, 5.0
    rng = np.random.default_rng(23)
    u1, v1 = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tr = rng.integers(0, H, (H, W))
    tc = rng.integers(0, W, (H, W))
    edge = rng.random((H, W)) < 0.3
    tr[edge] = rng.choice([-1, 0, H - 1, H], edge.sum())
    edge = rng.random((H, W)) < 0.3
    tc[edge] = rng.choice([-1, 0, W - 1, W], edge.sum())
    fwd = np.zeros((H, W, 2))
    fwd[..., 1] = tr - u1                                   # U = dx moves the row (u1)
    fwd[..., 0] = tc - v1                                   # V = dy moves the column (v1)
    # the backward flow at a target undoes the forward one up to an error vector drawn from these (|e| = 0, 5, 5, 5, sqrt 26, sqrt 34)
    errs = np.array([[0, 0], [3, 4], [-4, 3], [0, -5], [1, 5], [-3, -5]])
    ok = (tr >= 0) & (tr < H) & (tc >= 0) & (tc < W)
    bwd = rng.integers(-6, 7, (H, W, 2)).astype(np.float64)
    e = errs[rng.integers(0, len(errs), (H, W))]
    bwd[tr[ok], tc[ok]] = -fwd[ok] + e[ok]
    # what the error is at every pixel (float64, exact on these integers)
    g = bwd[np.clip(tr, 0, H - 1), np.clip(tc, 0, W - 1)]
    err = np.hypot(fwd[..., 0] + g[..., 0], fwd[..., 1] + g[..., 1])
    assert (ok & (err == tresh)).sum() > 100 and (ok & (err > tresh) & (err < 6)).sum() > 100 and (ok & (err == 0)).any()
    for v in (-1, 0, H - 1, H):
        assert (tr == v).any()
    for v in (-1, 0, W - 1, W):
        assert (tc == v).any()
    ref = O.fb_consistency(fwd, bwd, tresh)
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    got = pkg("pipeline").fb_consistency(dev(fwd), dev(bwd), tresh).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert ref[..., 2][ok & (err == tresh)].all() and not ref[..., 2][~ok].any()
