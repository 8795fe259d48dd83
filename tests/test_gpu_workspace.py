"""Every stage in a workspace of exactly the size the library names for it, between two guards, filled with poison.

include/dflow.h promises that a stage needs the bytes its size function names (dflow_workspace_bytes, the eleven
dflow_*_workspace_bytes, and per main-path stage the need its own DFLOW_ENOSPC message states), writes nothing beyond them and
reads nothing it has not written.  The rest of the suite hands out torch.empty(nbytes): the caching allocator rounds sizes up
and recycles blocks, so an overrun lands in slack and a stale read sees zeros or an earlier test's data.  Here (ws_guard.py) the
workspace is a region of exactly `need` bytes between two 4096-byte guards, filled with 0x00, 0xFF (NaN, -1, UINT_MAX) or 0x7F
(a large finite float, a large positive int) before the call.  The rule of every case:

* the stage runs once per poison, with fresh outputs;
* all outputs, statistics structs and count arrays included, are byte-identical across the three poisons;
* the first run passes the comparison the stage's own test module makes (its reference helper and its tolerance, none added);
* both guards are intact after every run.

Entry points covered (every one of include/dflow.h that takes d_ws):
    dflow_daisy, dflow_daisy_pair, dflow_knn_proposals, dflow_knn_proposals_timed, dflow_knn_screen_stats_n,
    dflow_knn_screen_stats, dflow_neighbour_proposals, dflow_bcd_prepare, dflow_bcd_phase     test_main_path_stage_by_stage
    dflow_bcd_sweep, and all of the above in one buffer of dflow_workspace_bytes     test_whole_pass_in_one_exact_buffer
    dflow_bcd_phase_batch, dflow_bcd_sweep_batch                                     test_sweep_batch_of_nine_...
    dflow_bcd_stats, dflow_bcd_stats_batch                                           test_bcd_stats, test_bcd_stats_batch_of_nine_...
    dflow_canny_edges, dflow_pb_edges, dflow_epic_interpolate, dflow_epic_prefilter, dflow_var_refine, dflow_flow_eval,
    dflow_flow_color, dflow_warp_eval, dflow_flow_advance, dflow_segment_filter      test_<stage>

Image-plane sizes: 1x1 (the smallest workspace, everything a tail) and 37x101 (partial tiles in both axes, four blocks of the
1024-pixel plane kernels); the stages that keep one partial result per block also run 1025x1027, where plane_blocks' cap of 1024
binds and the grid-stride loop and the partial count come apart.

After dflow_bcd_prepare the regions of the workspace that csrc/bcd.hip (BcdPlanes) documents as fully written, lab and blkA,
are byte-identical across the poisons.  The others are named there as unwritten or order-dependent and are left out: back is
the phases' scratch; blkBC holds only the second and third blocks that exist; the 160-bit rows of the "more" labels are
bump-allocated from masks with an atomic cursor, so their order, and the pool bases in blkBC, differ between two runs on the
same poison (measured at 40x48: 152 870 of 12 672 256 bytes, all at or beyond blkBC; 3 112 157 bytes keep the poison).  What
those regions feed is covered by the labels after the four phases.

The header's persistence claims (the records of dflow_bcd_prepare stay valid under dflow_bcd_stats, dflow_bcd_stats_batch,
dflow_labels_to_flow, dflow_pack_compat and dflow_prior_proposals) are checked on a snapshot of the workspace's bytes, the batch
claims (one workspace per pass, npass times the statistics workspace) with regions 4096 bytes apart in one allocation.

Lowest documented alignment: dflow_bcd_stats (8), dflow_flow_advance (4) and dflow_segment_filter (4) also run with d_ws that
many bytes past a 256-byte boundary.  Their kernels touch their regions with nothing wider: BsPartial {double, 6 x uint32} is
stored and loaded as a struct of 8-byte alignment (bcd_stats.hip), the winners are uint32 under atomicMin (prior.hip), labels and
sizes int32 under atomic loads, atomicMin and atomicAdd (segments.hip, union_find.h).  No case was dropped.
Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import ws_guard as G
from conftest import pkg

pytestmark = pytest.mark.gpu

POISONS = G.POISONS
SMALL = [(1, 1), (37, 101)]
BIG = (1025, 1027)
ids = lambda s: "%dx%d" % s if isinstance(s, tuple) and len(s) == 2 else None       # noqa: E731


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same_bytes(outs, what):
    """outs: per poison a list of arrays (None where an output was skipped): every one byte-equal to the first poison's."""
    for k in range(1, len(outs)):
        assert len(outs[k]) == len(outs[0])
        for i, (a, b) in enumerate(zip(outs[0], outs[k])):
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and a.tobytes() == b.tobytes())), \
                "%s: output %d under poison 0x%02X differs from the one under 0x%02X" % (what, i, POISONS[k], POISONS[0])


def three_poisons(torch, run, what, offset=0):
    """run() -> the stage's outputs (tensors, or None) through a pipeline.py wrapper.  Once per poison in exact guarded
    workspaces; the outputs must be byte-identical and the guards intact.  Returns the first run's outputs as arrays.  The
    device tensors of all runs stay alive until the end, so that no run is handed the block a former run's result lies in."""
    outs, keep = [], []
    for poison in POISONS:
        with G.guarded(torch, poison, offset) as handed:
            res = run()
        res = list(res) if isinstance(res, (tuple, list)) else [res]
        keep.append(res)
        torch.cuda.synchronize()
        handed.assert_guards("%s, poison 0x%02X" % (what, poison))
        assert all(g.ptr % 256 == offset for g in handed.all)
        outs.append([None if t is None else host(t) for t in res])
    same_bytes(outs, what)
    return outs[0]


def checked_under_guard(torch, check, what, poison=0xFF):
    """A check helper of another test module that runs the wrapper itself: inside exact guarded workspaces."""
    with G.guarded(torch, poison) as handed:
        ret = check()
    torch.cuda.synchronize()
    handed.assert_guards(what)
    return ret


# ================================================================================================ image-plane stages
@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_canny(torch_, size):
    import canny_ref as CR
    import test_gpu_canny as TC
    pipeline = pkg("pipeline")
    img = TC.noise_image(*size, seed=size[0] + size[1])
    ref = CR.canny(img, 20, 40)
    e, iv = three_poisons(torch_, lambda: pipeline.canny_edges(img, 20, 40), "canny %dx%d" % size)
    assert e.dtype == np.uint8 and np.array_equal(e, ref) and iv.tobytes() == CR.ivice(ref).tobytes()
    if size != (1, 1):
        assert 0 < (ref == 255).mean() < 0.5
    e2, none = three_poisons(torch_, lambda: pipeline.canny_edges(img, 20, 40, ivice=False), "canny %dx%d without ivice" % size)
    assert none is None and np.array_equal(e2, ref)


@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_pb(torch_, size):
    import test_gpu_pb as TP
    pipeline = pkg("pipeline")
    key = "ws%dx%d" % size
    img = TP.random_image(*size, seed=5)
    e64, m64, e32, m32 = TP.reference(key, img, 5)
    e, m = three_poisons(torch_, lambda: pipeline.pb_edges(img, 5, per_orientation=True), "pb %dx%d" % size)
    assert e.tobytes() == e32.tobytes() and m.tobytes() == m32.tobytes()
    assert np.abs(e - e64).max() <= TP.TOL and np.abs(m - m64).max() <= TP.TOL
    e2, = three_poisons(torch_, lambda: pipeline.pb_edges(img, 5), "pb %dx%d without the orientation plane" % size)
    assert e2.tobytes() == e32.tobytes()
    checked_under_guard(torch_, lambda: TP.check(key, img), "pb_ref check %dx%d" % size)


@pytest.mark.parametrize("seeds", ["none", "one", "30%"])
@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_epic(torch_, size, seeds):
    import test_gpu_epic as TE
    pipeline = pkg("pipeline")
    H, W = size
    sp, e = TE.random_field(H, W, 0.3 if seeds == "30%" else 0.0, seed=3 + H, edge_style="sparse")
    if seeds == "one":
        sp[H // 2, W // 3] = (2.0, -1.0, 1.0)
    what = "epic %dx%d %s seeds" % (H, W, seeds)
    nseeds = int((sp[..., 2] > 0.5).sum())
    assert nseeds == {"none": 0, "one": 1}.get(seeds, nseeds) and (seeds != "30%" or size == (1, 1) or nseeds > 1000)
    for method in ("LA", "NW"):
        full = three_poisons(torch_, lambda: pipeline.epic_interpolate(sp, e, 16, 0.8, method, aux=True), "%s %s" % (what, method))
        flow, = three_poisons(torch_, lambda: pipeline.epic_interpolate(sp, e, 16, 0.8, method), "%s %s, flow only" % (what, method))
        assert flow.tobytes() == full[0].tobytes(), "the flow does not depend on the optional outputs"
        if seeds == "none":
            assert not full[0].any() and (full[1] == -1).all()
    # S, D and the lists byte for byte, the flow of both methods within its 1e-3 px: test_gpu_epic's own check
    checked_under_guard(torch_, lambda: TE.check_exact(sp, e, nn=16), what)


@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_epic_prefilter(torch_, size):
    """Both stages on: saliency at the median of the frame's own saliency, consistency over 8 neighbours."""
    import epic_prefilter_cases as PC
    import epic_prefilter_ref as P
    import test_gpu_epic_prefilter as TPF
    pipeline = pkg("pipeline")
    H, W = size
    sp, e = PC.random_field(H, W, 0.3, seed=100 * H + W)
    sp[0, 0] = (1.5, -0.5, 1.0)
    # 1x1: the "noise1x1" frame of PC.saliency_images(); 37x101: the generator of its synthetic frames
    img = np.random.default_rng(2).integers(0, 256, (1, 1, 3)).astype(np.uint8) if size == (1, 1) else PC.synth_image(H, W, 7)
    kw = dict(saliency_th=0.045 if size == (1, 1) else TPF.median_saliency(img), pref_nn=8, pref_th=3.0, k=0.8)
    ref = P.prefilter(sp, e, img, **kw)
    got = three_poisons(torch_, lambda: pipeline.epic_prefilter(sp, e, img, aux=True, **kw), "prefilter %dx%d" % size)
    TPF.compare(sp, e, img, tuple(got), ref, kw["saliency_th"], kw["pref_th"])
    if size != (1, 1):
        assert all((ref["reason"] == r).any() for r in (P.KEPT, P.SALIENCY, P.CONSISTENCY))
    out, = three_poisons(torch_, lambda: pipeline.epic_prefilter(sp, e, img, **kw), "prefilter %dx%d, field only" % size)
    assert out.tobytes() == got[0].tobytes()


@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_variational(torch_, size):
    """Fused and unfused solver, one outer iteration.  Tolerance: test_gpu_variational.TOL_OUTER1, whose yardstick is a maximum
    over variational_cases.parity_cases(); 1x1 is one of them, 37x101 comes from the same generator (synth_case) with one of
    their parameter sets, between its 33x65 and 129x257."""
    import test_gpu_variational as TV
    import variational_cases as VC
    import variational_ref as R
    pipeline, L = pkg("pipeline"), pkg("_lib")
    H, W = size
    img1, img2, flow, _ = VC.synth_case(H, W, seed=100 * H + W)
    P = dict(delta=0.5, sigma=1.0, niter_inner=2, niter_outer=1)
    assert dict(delta=0.5, sigma=1.0, niter_inner=2) in VC.PARAM_SETS
    fused, = three_poisons(torch_, lambda: pipeline.variational_refine(img1, img2, flow, **P), "variational %dx%d fused" % size)
    plain, = three_poisons(torch_, lambda: pipeline.variational_refine(img1, img2, flow, flags=L.VAR_FLAG_SOR_UNFUSED, **P),
                           "variational %dx%d unfused" % size)
    assert fused.tobytes() == plain.tobytes(), "fused differs from unfused"
    want = R.refine(img1, img2, flow, np.float64, **P)
    err = float(np.abs(fused - want).max())
    print("variational %dx%d: max |gpu - float64| = %.3e (tolerance %.3e)" % (H, W, err, TV.TOL_OUTER1))
    assert np.isfinite(fused).all() and err <= TV.TOL_OUTER1


@pytest.mark.parametrize("size", SMALL + [BIG], ids=ids)
def test_flow_eval(torch_, size):
    import test_gpu_eval as TEV
    torch, pipeline = torch_, pkg("pipeline")
    H, W = size
    test, gt, ref = TEV.case(H, W)
    what = "eval %dx%d" % size
    stats, err, img = three_poisons(torch, lambda: pipeline.flow_eval(test, gt, 3.0, err=True, image=True), what)
    TEV.check_stats(pipeline.eval_stats(torch.from_numpy(stats)), ref, what)
    assert TEV.same_plane(err, ref["err"], test, gt, "err") and TEV.same_plane(img, ref["bgr"], test, gt, "picture")
    bare, = three_poisons(torch, lambda: pipeline.flow_eval(test, gt, 3.0), what + ", statistics only")
    assert bare.tobytes() == stats.tobytes()
    # DFLOW_EVAL_FLAG_ACCUMULATE onto zeros: 0 + x and max(0, x) are x, the same 64 bytes
    acc, = three_poisons(torch, lambda: pipeline.flow_eval(test, gt, 3.0, stats=torch.zeros(8, dtype=torch.int64, device="cuda:0")),
                         what + ", accumulated")
    assert acc.tobytes() == stats.tobytes()


@pytest.mark.parametrize("size", SMALL + [BIG], ids=ids)
def test_flow_color(torch_, size):
    import flowpic_ref as R
    import test_gpu_flowpic as TF
    pipeline = pkg("pipeline")
    H, W = size
    flow, planted = R.color_case(H, W, 4.0)
    for max_flow in ((None,) if size == BIG else (None, 10.0)):        # None: max_flow == 0, the radius comes through the workspace
        what = "colour %dx%d max_flow %s" % (H, W, max_flow)
        ref = R.flow_color(flow, max_flow or 0.0)
        img, radius = three_poisons(torch_, lambda: pipeline.flow_color(flow, max_flow, return_radius=True), what)
        assert radius.view(np.uint32)[0] == np.array([ref["maxrad"]], np.float32).view(np.uint32)[0], (radius, ref["maxrad"])
        TF.check_color(img, ref, planted, what)
        bare, = three_poisons(torch_, lambda: pipeline.flow_color(flow, max_flow), what + ", picture only")
        assert bare.tobytes() == img.tobytes()


@pytest.mark.parametrize("size", SMALL + [BIG], ids=ids)
def test_warp_eval(torch_, size):
    import flowpic_ref as R
    import test_gpu_flowpic as TF
    torch, pipeline = torch_, pkg("pipeline")
    H, W = size
    img1, img2, flow, _ = R.warp_case(H, W, 4.0)
    what = "warp %dx%d" % size
    ref = R.warp(img1, img2, flow, 10.0, 30.0)
    stats, wp, err, pic = three_poisons(torch, lambda: pipeline.warp_eval(img1, img2, flow, 10.0, 30.0, warped=True, err=True, image=True),
                                        what)
    TF.check_stats(pipeline.photo_stats(torch.from_numpy(stats)), ref, what)
    assert TF.same_plane(err, ref["err"], "err") and TF.same_plane(wp, ref["warped"], "warped") and TF.same_plane(pic, ref["bgr"], "picture")
    bare, = three_poisons(torch, lambda: pipeline.warp_eval(img1, img2, flow, 10.0, 30.0), what + ", statistics only")
    assert bare.tobytes() == stats.tobytes()
    acc, = three_poisons(torch, lambda: pipeline.warp_eval(img1, img2, flow, 10.0, 30.0,
                                                           stats=torch.zeros(6, dtype=torch.int64, device="cuda:0")), what + ", accumulated")
    assert acc.tobytes() == stats.tobytes()


def advance_field(H, W):
    """The fields of test_gpu_prior.test_flow_advance_matches_the_reference, [U,V,valid] layout."""
    rng = np.random.default_rng(H * 1000 + W)
    amp = max(1, min(H, W) // 3)
    flow = (rng.integers(-amp, amp + 1, (H, W, 2)) + rng.choice([0.0, 0.5], (H, W, 2), p=[0.7, 0.3])).astype(np.float32)
    if H * W > 1:
        flow[0, 0] = (0.0, -0.0)
        flow[H - 1, W - 1] = (np.nan, 1.0)
    return np.ascontiguousarray(np.concatenate([flow[..., ::-1], (rng.random((H, W, 1)) > 0.2).astype(np.float32)], axis=-1))


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_flow_advance(torch_, size, offset):
    """offset 4: the alignment include/dflow.h states for this d_ws (uint32 winners under atomicMin, nothing wider)."""
    import prior_ref as R
    pipeline = pkg("pipeline")
    flow = advance_field(*size)
    want, counts = R.flow_advance(flow, R.NEGATE)
    assert sum(counts) == size[0] * size[1] and (size == (1, 1) or counts[1] > 0)
    what = "advance %dx%d" % size
    got, cnt = three_poisons(torch_, lambda: pipeline.flow_advance(flow, negate=True, counts=True), what, offset)
    assert cnt.tolist() == counts and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    bare, = three_poisons(torch_, lambda: pipeline.flow_advance(flow, negate=True), what + ", without counts", offset)
    assert bare.tobytes() == got.tobytes()


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("size", SMALL, ids=ids)
def test_segment_filter(torch_, size, offset):
    """offset 4: the alignment include/dflow.h states for this d_ws (int32 labels and sizes, nothing wider)."""
    import test_gpu_segments as TS
    pipeline = pkg("pipeline")
    h, w = size
    f = TS.blocks(h, w, 0.75, 12)
    want = TS.reference(("ws-blocks", h, w), f, 2.0, 12)
    if size != (1, 1):
        assert 0 < want[3][1] < want[3][0], "segments are both removed and kept"
    what = "segments %dx%d" % size
    out, seg, sz, cnt = three_poisons(torch_, lambda: pipeline.segment_filter(f, 2.0, 12, segments=True, sizes=True, counts=True), what, offset)
    TS.same((out, seg, sz, cnt.tolist()), want, what)
    bare, = three_poisons(torch_, lambda: pipeline.segment_filter(f, 2.0, 12), what + ", field only", offset)
    assert bare.tobytes() == out.tobytes()


# ================================================================================================ bcd_stats
def stats_state(torch):
    import test_gpu_bcd_stats as TB
    s = TB.State(torch, 33, 65, seed=77, maxnprop=40)
    assert s.wsb == int(pkg("_lib").lib().dflow_bcd_stats_workspace_bytes(C.byref(s.p)))
    return TB, s


@pytest.mark.parametrize("offset", [0, 8], ids=["aligned", "offset8"])
def test_bcd_stats(torch_, offset):
    """33x65 against an earlier labelling, d_prev_out given.  offset 8: the alignment include/dflow.h states for this d_ws."""
    torch = torch_
    TB, s = stats_state(torch)
    rng = np.random.default_rng(6)
    prev = s.random_labels(rng)
    raws, outs = [], []
    for poison in POISONS:
        g = G.GuardedWs(torch, s.wsb, poison, s.dev, offset)
        assert g.ptr % 256 == offset
        s.ws = g.region
        out = torch.full((33, 65), TB.SENTINEL, dtype=torch.int32, device=s.dev)
        raws.append(s.call(d_prev=s.upload(prev), d_prev_out=out))
        outs.append(out.cpu().numpy())
        g.assert_guards("bcd_stats, poison 0x%02X" % poison)
    assert raws[0] == raws[1] == raws[2] and all(np.array_equal(o, s.labels) for o in outs)
    got = TB.check(raws[0], s.ref(prev=prev), "33x65 with prev:")
    assert got["n_changed"] > 0


def test_bcd_stats_batch_of_nine_in_one_exact_region(torch_):
    """Nine labellings in one region of exactly 9 * dflow_bcd_stats_workspace_bytes (two pairs of launches, 8 + 1: the second must
    find pass 8's slice): byte for byte the 48 bytes of nine single calls, under every poison."""
    torch = torch_
    L = pkg("_lib")
    TB, s = stats_state(torch)
    rng = np.random.default_rng(6)
    labs = [s.random_labels(rng) for _ in range(9)]
    prevs = [s.random_labels(rng) for _ in range(9)]
    g1 = G.GuardedWs(torch, s.wsb, 0xFF, s.dev)
    s.ws = g1.region
    single = []
    for k in range(9):
        g1.repoison()
        single.append(s.call(d_labels=s.upload(labs[k]), d_prev=s.upload(prevs[k])))
    g1.assert_guards("single calls")
    assert len(set(single)) == 9
    TB.check(single[8], s.ref(labels=labs[8], prev=prevs[8]), "pass 8:")
    same = lambda t: (C.c_void_p * 9)(*[t.data_ptr()] * 9)                # noqa: E731
    each = lambda ts: (C.c_void_p * 9)(*[t.data_ptr() for t in ts])       # noqa: E731
    for poison in POISONS:
        g = G.GuardedWs(torch, 9 * s.wsb, poison, s.dev)
        d_labs, d_prevs = [s.upload(a) for a in labs], [s.upload(a) for a in prevs]
        out = torch.full((9, 6), TB.SENTINEL, dtype=torch.int64, device=s.dev)
        L.call("dflow_bcd_stats_batch", C.byref(s.p), 9, same(s.d_prop), same(s.d_cost), same(s.d_nprop), each(d_labs), each(d_prevs),
               out.data_ptr(), g.ptr, g.nbytes, L.stream(s.dev))
        raw = out.cpu().numpy().tobytes()
        g.assert_guards("bcd_stats_batch, poison 0x%02X" % poison)
        for k in range(9):
            assert raw[48 * k:48 * (k + 1)] == single[k], "pass %d of the batch differs from the single call (poison 0x%02X)" % (k, poison)
            assert np.array_equal(d_prevs[k].cpu().numpy(), labs[k]), k
        # one byte less is refused
        assert L.lib().dflow_bcd_stats_batch(C.byref(s.p), 9, same(s.d_prop), same(s.d_cost), same(s.d_nprop), each(d_labs), each(d_prevs),
                                             out.data_ptr(), g.ptr, g.nbytes - 1, L.stream(s.dev)) == G.ENOSPC


# ================================================================================================ main-path stages
import test_gpu_abi_edges as AE      # noqa: E402  (new_pass, oracle_params, stored, poison, the O fixture)

O = AE.O

GEOMS = [((40, 48, 5, 6), "f32"), ((40, 48, 5, 6), "f16"), ((45, 35, 9, 7), "f32")]
geom_ids = ["%dx%d_c%dx%d_%s" % (g + (s,)) for g, s in GEOMS]


def main_needs(df):
    pp, P = C.byref(df.p), G.PTR
    needs = {"dflow_daisy": G.stage_need("dflow_daisy", pp, P, P),
             "dflow_daisy_pair": G.stage_need("dflow_daisy_pair", pp, P, P, P, P),
             "dflow_knn_proposals": G.stage_need("dflow_knn_proposals", pp, P, P, P, P, P, P),
             "dflow_neighbour_proposals": G.stage_need("dflow_neighbour_proposals", pp, P, P, P, P, P, P),
             "dflow_bcd_prepare": G.stage_need("dflow_bcd_prepare", pp, P, P, P)}
    assert G.stage_need("dflow_bcd_phase", pp, P, P, P, 0) == needs["dflow_bcd_prepare"]
    assert max(needs.values()) + 256 == df.ws_bytes, (needs, df.ws_bytes)
    return needs


def pair(synth, H, W, seed=0):
    return synth.make_pair(H, W, seed=seed, amp_x=0.1 * W, amp_y=0.1 * H)[:2]


def state_bytes(df):
    return [t.cpu().numpy().tobytes() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)]


def prepared_planes(df):
    """The bytes of the two regions dflow_bcd_prepare writes in full, lab [pix][LP] and blkA [pix][2][LP] of uint2, cut out of
    the workspace by the layout of planes_of (csrc/bcd.hip): back, the longest phase's chains x 192 bytes per step, comes first;
    every region starts on a multiple of 256."""
    H, W, LP = df.p.pich, df.p.picw, df.p.label_pitch
    a256 = lambda v: (v + 255) & ~255                    # noqa: E731
    back = a256(max(((W + 1) // 2) * H, ((H + 1) // 2) * W) * 192)
    lab, blk_a = H * W * LP * 8, H * W * 2 * LP * 8
    assert back + a256(lab) + a256(blk_a) < df.ws_bytes
    ws = df.ws.cpu().numpy()
    return [ws[back:back + lab].tobytes(), ws[back + a256(lab):back + a256(lab) + blk_a].tobytes()]


@pytest.mark.parametrize("geom,storage", GEOMS, ids=geom_ids)
def test_main_path_stage_by_stage(torch_, O, synth, geom, storage):
    """dflow_daisy, dflow_daisy_pair, the screened dflow_knn_proposals (and its measurement aids), dflow_neighbour_proposals,
    dflow_bcd_prepare + the four dflow_bcd_phase: each in a guarded region of its own need; every stage against the oracle bit
    for bit, as test_gpu_abi_edges.stages does."""
    H, W, ch, cw = geom
    img1, img2 = pair(synth, H, W)
    runs = []
    for poison in POISONS:
        df = AE.new_pass(H, W, ch, cw, storage, seed=5)
        needs = main_needs(df)
        what = "%s poison 0x%02X: " % (geom_ids[GEOMS.index((geom, storage))], poison)
        got = {}

        def stage(name, fn):
            g = G.guard_pass(df, poison, needs[name])
            ret = fn()
            g.assert_guards(what + name)
            return ret
        one = stage("dflow_daisy", lambda: df.izracunajDaisy(img1))
        got["daisy"] = [one.cpu().numpy().tobytes()]
        stage("dflow_daisy_pair", lambda: df.load_pair(img1, img2))
        got["daisy_pair"] = [df.descrs1.cpu().numpy().tobytes(), df.descrs2.cpu().numpy().tobytes()]
        got["descr"] = [df.descriptors_f32(i).cpu().numpy() for i in (0, 1)]
        AE.poison(df)
        stats = stage("dflow_knn_proposals", lambda: (df.generisi(), df.knn_stats())[1])
        assert stats["flags"] == 0 and stats["query_cell_pairs"] > 0, stats           # the screen ran
        got["knn"], got["knn_stats"], got["knn_state"] = state_bytes(df), stats, df.host_state()
        AE.assert_fill(df, "knn")

        def timed():
            """The measurement aids on a freshly poisoned region: the same launches with events between them, and the 13-value
            form of the statistics."""
            AE.poison(df)
            df.generisi_timed()
            first13 = (C.c_int64 * 13)()
            pkg("_lib").call("dflow_knn_screen_stats", df._pp(), df.ws.data_ptr(), df.ws_bytes, df._stream(), first13)
            return [int(v) for v in first13]
        first13 = stage("dflow_knn_proposals", timed)
        assert state_bytes(df) == got["knn"], what + "dflow_knn_proposals_timed writes what dflow_knn_proposals writes"
        assert first13 == [stats[k] for k in df.KNN_STATS], (first13, stats)
        stage("dflow_neighbour_proposals", df.nasumicni)
        got["neighbour"], got["neighbour_state"] = state_bytes(df), df.host_state()
        AE.assert_fill(df, "neighbour")

        def sweep():
            df.pakovanje()
            got["prepared"] = prepared_planes(df)
            for phase in range(4):
                df.bcd_phase(phase)
        stage("dflow_bcd_prepare", sweep)
        got["labels"] = df.bestlabels.cpu().numpy()
        runs.append(got)
    for k in (1, 2):
        for key in ("daisy", "daisy_pair", "knn", "neighbour", "prepared"):
            assert runs[k][key] == runs[0][key], "%s differs between poison 0x%02X and 0x%02X" % (key, POISONS[k], POISONS[0])
        assert runs[k]["knn_stats"] == runs[0]["knn_stats"], (runs[k]["knn_stats"], runs[0]["knn_stats"])
        assert np.array_equal(runs[k]["labels"], runs[0]["labels"]), "labels after four phases, poison 0x%02X" % POISONS[k]
    # the first run against the oracle
    r, p = runs[0], AE.oracle_params(O, df)
    assert r["daisy"][0] == r["daisy_pair"][0], "dflow_daisy and dflow_daisy_pair write the same plane"
    d1, d2 = AE.stored(O.daisy(img1), storage), AE.stored(O.daisy(img2), storage)
    for i, d in enumerate((d1, d2)):
        assert np.array_equal(r["descr"][i].view(np.uint32), d.view(np.uint32)), ("daisy", i)
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    for k, v in zip(AE.OUTPUTS, (pr, lc, npr, bl)):
        assert np.array_equal(r["knn_state"][k], v), ("knn", k)
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    for k, v in zip(AE.OUTPUTS[:3], (pr, lc, npr)):
        assert np.array_equal(r["neighbour_state"][k], v), ("neighbour", k)
    for phase in range(4):
        O.bcd_phase(p, pr, lc, npr, bl, phase)
    assert np.array_equal(r["labels"], bl), "labels after four phases"


def test_whole_pass_in_one_exact_buffer(torch_, O, synth):
    """One pass in a single region of exactly dflow_workspace_bytes, re-poisoned before dflow_daisy_pair, dflow_knn_proposals,
    dflow_neighbour_proposals and dflow_bcd_prepare (not between prepare and the sweeps): labels and flow after two dflow_bcd_sweep
    equal an ordinary DiscreteFlow.run bit for bit, and the oracle's."""
    H, W, ch, cw = 40, 48, 5, 6
    img1, img2 = pair(synth, H, W, seed=2)
    plain = AE.new_pass(H, W, ch, cw, seed=9)
    want_flow = plain.run(img1, img2, 2).cpu().numpy()
    want_labels = plain.bestlabels.cpu().numpy()
    ref = O.full_pass(AE.oracle_params(O, plain), img1, img2, 2)
    assert np.array_equal(want_labels, ref["bestlabels"]) and np.array_equal(want_flow.astype(np.float64), ref["flows"][-1])
    for poison in POISONS:
        df = AE.new_pass(H, W, ch, cw, seed=9)
        g = G.guard_pass(df, poison)
        assert g.nbytes == int(pkg("_lib").lib().dflow_workspace_bytes(C.byref(df.p)))
        for step in (lambda: df.load_pair(img1, img2), df.generisi, df.nasumicni, lambda: (df.pakovanje(), df.ceoBCD(2))):
            g.repoison()
            step()
            g.assert_guards("whole pass, poison 0x%02X" % poison)
        assert np.array_equal(df.bestlabels.cpu().numpy(), want_labels), "labels, poison 0x%02X" % poison
        assert df.vratiKonacniFlow().cpu().numpy().tobytes() == want_flow.tobytes(), "flow, poison 0x%02X" % poison


def test_prepared_records_survive_the_calls_the_header_names(torch_, oracle, synth):
    """include/dflow.h: the records of dflow_bcd_prepare "stay valid until another stage reuses the workspace"; dflow_bcd_stats
    "neither reads nor writes" them; dflow_prior_proposals "leaves the caller's [workspace] alone".  A snapshot of the whole
    region after dflow_bcd_prepare is unchanged after dflow_bcd_stats, dflow_bcd_stats_batch (its own workspace),
    dflow_labels_to_flow and dflow_pack_compat, and the sweep that follows gives the labels of an uninterrupted run; it is
    unchanged after dflow_prior_proposals, after which the header asks for another prepare: that sweep against the oracle
    composition of test_gpu_prior.test_bcd_sweeps_after_the_prior_step_match_the_oracle."""
    import test_gpu_prior as TPR
    torch, L = torch_, pkg("_lib")
    ps = TPR.Pass(synth, "40x48")
    df = ps.df
    g = G.guard_pass(df, 0xFF)
    labels0 = df.bestlabels.clone()
    df.pakovanje()
    df.ceoBCD(1)
    uninterrupted = df.bestlabels.cpu().numpy().copy()
    g.assert_guards("uninterrupted sweep")
    # again, with the calls between prepare and the sweep
    df.bestlabels.copy_(labels0)
    g.repoison()
    df.pakovanje()
    snap = g.snapshot()
    per_pass = int(L.lib().dflow_bcd_stats_workspace_bytes(C.byref(df.p)))
    gs = G.GuardedWs(torch, 2 * per_pass, 0x7F, df.device)
    df._stats_ws = gs.region[:per_pass]                                      # DiscreteFlow.bcd_stats draws from it
    prev = labels0.clone()
    st = df.bcd_stats(prev=prev, prev_out=prev)
    assert g.snapshot() == snap, "dflow_bcd_stats changed the prepared workspace"
    two = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())           # noqa: E731
    out = torch.empty((2, 6), dtype=torch.int64, device=df.device)
    L.call("dflow_bcd_stats_batch", C.byref(df.p), 2, two(df.proposals), two(df.lcosts), two(df.nprop), two(df.bestlabels), None,
           out.data_ptr(), gs.ptr, gs.nbytes, L.stream(df.device))
    assert g.snapshot() == snap, "dflow_bcd_stats_batch changed the prepared workspace"
    raw = out.cpu().numpy().tobytes()
    assert raw[:48] == raw[48:] and raw[:24] == st.cpu().numpy().tobytes()[:24]       # the sums; n_changed is the single call's own
    gs.assert_guards("statistics workspaces")
    df.vratiKonacniFlow()
    assert g.snapshot() == snap, "dflow_labels_to_flow changed the prepared workspace"
    pkg("compat").packedksets(df)
    assert g.snapshot() == snap, "dflow_pack_compat changed the prepared workspace"
    assert df._bcd_ready
    df.ceoBCD(1)
    assert np.array_equal(df.bestlabels.cpu().numpy(), uninterrupted), "the sweep after the four calls"
    g.assert_guards("interrupted sweep")
    # the prior step: the device against prior_ref bit for bit (Pass.check), the workspace untouched
    snap = g.snapshot()
    ps.check(ps.gt, 2)
    assert g.snapshot() == snap, "dflow_prior_proposals changed the caller's workspace"
    stt = df.host_state()
    assert stt["nprop"].max() > ps.host()[2].max()
    H, W, ch, cw = TPR.GEOMS["40x48"][:4]
    p = oracle.make_params(H, W, ch, cw, seed=TPR.SEED)
    bl = stt["bestlabels"].copy()
    for sweep in range(2):
        df.ceoBCD(1)                                                         # the first one prepares again
        oracle.bcd_sweep(p, stt["proposals"], stt["lcosts"], stt["nprop"], bl)
        assert np.array_equal(df.bestlabels.cpu().numpy(), bl), sweep
    g.assert_guards("after the prior step")


def test_sweep_batch_of_nine_in_regions_4096_bytes_apart(torch_, synth):
    """dflow_bcd_sweep_batch over 9 passes at (24, 40, 6, 8): two launches per phase, 8 + 1.  Every pass has "its own workspace of
    ws_bytes": nine regions of exactly the BCD stage's need, 4096 guard bytes between them, in one allocation.  "Results
    identical to npass separate calls": every pass's labels after two sweeps equal its single run in the same region."""
    torch = torch_
    H, W, ch, cw = 24, 40, 6, 8
    pl = pkg("pipeline")
    n = 9
    passes = []
    for k in range(n):
        img1, img2, _ = synth.make_pair(H, W, seed=synth.pair_seed(k // 2, 0), amp_x=0.08 * W, amp_y=0.08 * H)
        if k % 2:
            img1, img2 = img2, img1
        df = AE.new_pass(H, W, ch, cw, seed=k)
        df.load_pair(img1, img2); df.generisi(); df.nasumicni()
        passes.append(df)
    need = main_needs(passes[0])["dflow_bcd_prepare"]
    assert need % 256 == 0
    pitch = need + G.GUARD
    for poison in POISONS:
        buf = torch.full((G.GUARD + 256 + n * pitch,), G.GUARD_BYTE, dtype=torch.uint8, device=passes[0].device)
        first = G.GUARD + (-(buf.data_ptr() + G.GUARD)) % 256
        inside = np.zeros(buf.numel(), bool)
        start = [df.bestlabels.clone() for df in passes]
        for k, df in enumerate(passes):
            a = first + k * pitch
            df.ws, df.ws_bytes, df._bcd_ready = buf[a:a + need], need, False
            inside[a:a + need] = True
            assert df.ws.data_ptr() % 256 == 0

        def fill():
            for df in passes:
                df.ws.fill_(poison)

        def assert_guards(what):
            changed = np.flatnonzero((buf.cpu().numpy() != G.GUARD_BYTE) & ~inside)
            assert changed.size == 0, "%s, poison 0x%02X: %d guard bytes changed, first at %d, last at %d (regions start at %d + k * %d, %d bytes)" \
                % (what, poison, changed.size, changed[0], changed[-1], first, pitch, need)
        fill()
        single = []
        for df in passes:
            df.pakovanje()
            df.ceoBCD(2)
            single.append(df.bestlabels.cpu().numpy().copy())
        assert_guards("single runs")
        assert len({s.tobytes() for s in single}) == n
        for df, s in zip(passes, start):
            df.bestlabels.copy_(s)
            df._bcd_ready = False
        fill()
        pl.ceoBCD_batch(passes, 2)                                           # prepares every pass, then dflow_bcd_sweep_batch twice
        assert_guards("batch")
        for k, (df, want) in enumerate(zip(passes, single)):
            assert np.array_equal(df.bestlabels.cpu().numpy(), want), "pass %d of the batch, poison 0x%02X" % (k, poison)
        for df, s in zip(passes, start):
            df.bestlabels.copy_(s)
