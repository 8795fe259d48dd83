"""Every data plane of every entry point exact-size, between guards, at its lowest documented alignment.

The rest of the GPU suite places every plane at the start of a torch allocation: 256-byte-aligned (and more) and followed by
the allocator's slack.  A kernel that stores four pixels at a time and writes a dword past a plane whose byte count is no
multiple of four, or one whose result depends on a plane being more aligned than include/dflow.h asks, passes all of it.  Here
every input and every output plane of a call is the region of a ws_guard.GuardedWs: exactly the plane's bytes, 4096 guard bytes
on both sides, its address `a` bytes past a 256-byte boundary, a the alignment the header states for the plane (a multiple of a
and of nothing coarser).  All planes of a call sit at their lowest alignment at once; the workspace is an ordinary allocation
(tests/test_gpu_workspace.py is about it).  After one call:

* every output plane, state plane and counts array equals, byte for byte, what the same call writes with every plane in an
  ordinary allocation (the placement all other GPU tests judge against the references);
* where tests/*_ref.py defines the stage and the stage's own tests compare byte for byte, the planes equal that definition too;
* every guard holds its pattern, every input region is unchanged (but those the header lets a stage write in place).

Outputs and state planes a stage must fill start as 0xFF.  No tolerances: everything is byte equality.

Sizes: image-plane stages at 1x1, 5x7 (35 pixels) and 37x101 (3737 pixels: no multiple of four, ragged against 32x8 tiles, more
than one tile both ways); the main path at test_gpu_workspace.GEOMS, stage after stage on the state the one before left.
STAGES is the table: name -> (the entry points it calls, builder); the builders make Stage records (planes, call) and one
driver, check(), places and judges them.  Host-only tests hold ALIGN against the gates of csrc/abi.hip and STAGES against the
list of entry points.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import test_abi_refusals as TR
import ws_guard as G
from conftest import pkg

gpu = pytest.mark.gpu
POISON = 0xFF
IMAGE_SIZES = [(1, 1), (5, 7), (37, 101)]
GEOMS = [((40, 48, 5, 6), "f32"), ((40, 48, 5, 6), "f16"), ((45, 35, 9, 7), "f32")]      # those of test_gpu_workspace.py
geom_ids = ["%dx%d_c%dx%d_%s" % (g + (s,)) for g, s in GEOMS]
F = np.float32
UVV, DYDX = 0, 1

# include/dflow.h, Conventions, "Alignment of data planes": entry point -> plane -> bytes, as that paragraph lists them (a plane it
# does not name needs 1).  NAME[] is every entry of a batch form's host array.  test_alignments_are_the_gates_of_abi_hip holds
# this table against the library.
ALIGN = {
    "dflow_daisy": dict(d_descr=16),
    "dflow_daisy_pair": dict(d_descr1=16, d_descr2=16),
    "dflow_knn_proposals": dict(d_descr1=16, d_descr2=16, d_proposals=16, d_lcosts=16, d_nprop=4, d_bestlabels=4),
    "dflow_knn_proposals_timed": dict(d_descr1=16, d_descr2=16, d_proposals=16, d_lcosts=16, d_nprop=4, d_bestlabels=4),
    "dflow_neighbour_proposals": dict(d_descr1=16, d_descr2=16, d_proposals=16, d_lcosts=16, d_nprop=4, d_bestlabels=4),
    "dflow_bcd_prepare": dict(d_proposals=16, d_lcosts=16, d_nprop=4),
    "dflow_bcd_phase": dict(d_proposals=16, d_nprop=4, d_bestlabels=4),
    "dflow_bcd_sweep": dict(d_proposals=16, d_nprop=4, d_bestlabels=4),
    "dflow_bcd_phase_batch": {"d_nprop[]": 4, "d_bestlabels[]": 4},
    "dflow_bcd_sweep_batch": {"d_nprop[]": 4, "d_bestlabels[]": 4},
    "dflow_bcd_stats": dict(d_proposals=16, d_lcosts=16, d_nprop=4, d_bestlabels=4, d_prev_labels=4, d_prev_out=4, d_stats=8),
    "dflow_bcd_stats_batch": {"d_proposals[]": 16, "d_lcosts[]": 16, "d_nprop[]": 4, "d_bestlabels[]": 4, "d_prev[]": 4, "d_stats": 8},
    "dflow_labels_to_flow": dict(d_proposals=16, d_bestlabels=4, d_flow=8),
    "dflow_fb_consistency": dict(d_fwd=8, d_bwd=8, d_sparse=4),
    "dflow_pack_compat": dict(d_proposals=16, d_nprop=4),
    "dflow_canny_edges": dict(d_ivice=4),
    "dflow_pb_edges": dict(d_strength=4, d_orient_strength=4),
    "dflow_epic_interpolate": dict(d_sparse=4, d_edges=4, d_flow=4, d_seed_of=4, d_dist=4, d_lists=4, d_list_g=8),
    "dflow_epic_prefilter": dict(d_sparse_in=4, d_edges=4, d_sparse_out=4, d_saliency=4, d_estimate=4),
    "dflow_var_refine": dict(d_flow_in=8, d_flow_out=8),
    "dflow_flow_eval": dict(d_test=16, d_gt=16, d_err=16, d_stats=8, d_err_bgr=4),
    "dflow_flow_color": dict(d_flow=16, d_bgr=4, d_maxrad=4),
    "dflow_warp_eval": dict(d_flow=16, d_err=16, d_stats=8, d_bgr1=4, d_warped=4, d_err_bgr=4),
    "dflow_prior_proposals": dict(d_descr1=16, d_descr2=16, d_proposals=16, d_prior=4, d_lcosts=4, d_nprop=4, d_bestlabels=4, d_counts=4),
    "dflow_flow_advance": dict(d_flow=4, d_out=4, d_counts=4),
    "dflow_pyr_down": dict(d_in1=4, d_in2=4, d_out1=4, d_out2=4),
    "dflow_flow_upsample": dict(d_coarse=4, d_out=4, d_counts=4),
    "dflow_flow_consistency": dict(d_fwd=4, d_bwd=4, d_out_fwd=4, d_out_bwd=4, d_err_fwd=4, d_err_bwd=4, d_counts=4),
    "dflow_segment_filter": dict(d_flow=4, d_out=4, d_segment=4, d_size=4, d_counts=4),
    "dflow_frame_interp": dict(d_keys=8, d_fwd=4, d_bwd=4, d_motion=4, d_motion_tmp=4, d_counts=4),
    "dflow_flow_wmedian": dict(d_flow=4, d_out=4, d_counts=4),
    "dflow_motion_fit": dict(d_state=8, d_flow=4, d_model=4, d_models=4, d_hyp_counts=4, d_model_flow=4, d_residual=4, d_counts=4),
    "dflow_label_confidence": dict(d_proposals=16, d_lcosts=16, d_sparse=16, d_nprop=4, d_bestlabels=4, d_margin=4, d_alt=4, d_counts=4),
    "dflow_flow_gate": dict(d_flow=16, d_score=16, d_out=16, d_counts=4),
}


# ================================================================================================ the harness
class Plane:
    """One device plane of a call.  role "in": `data` is copied in and must be unchanged afterwards; "io": `data` is copied in
    and the stage updates it in place; "out": poisoned, the stage fills it; "scratch": poisoned, guarded, not compared."""

    def __init__(self, name, align, role, data=None, dtype=None, shape=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype, shape = data.dtype, data.shape
        self.name, self.align, self.role, self.data = name, align, role, data
        self.dtype, self.shape = np.dtype(dtype), tuple(shape)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        assert self.nbytes > 0 and (role in ("in", "io")) == (data is not None) and align >= self.dtype.itemsize, name


class Planes:
    """The planes of entry point `fn`, their alignments read off ALIGN."""

    def __init__(self, fn):
        self.fn = fn

    def _a(self, arg):
        assert self.fn in ALIGN
        return ALIGN[self.fn].get(arg, 1)

    def inp(self, arg, data, name=None):
        return Plane(name or arg, self._a(arg), "in", data)

    def io(self, arg, data, name=None):
        return Plane(name or arg, self._a(arg), "io", data)

    def out(self, arg, dtype, shape, name=None, role="out"):
        return Plane(name or arg, self._a(arg), role, None, dtype, shape)


class Stage:
    """name, planes, call(ptr: plane name -> address), aliases {argument: the plane it is}, ref(got: name -> array) or None."""

    def __init__(self, name, planes, call, aliases=None, ref=None):
        self.name, self.planes, self.call, self.aliases, self.ref = name, planes, call, aliases or {}, ref
        assert len({p.name for p in planes}) == len(planes)


class Ordinary:
    """A plane the way every other test places it: a torch allocation of its own."""

    def __init__(self, torch, nbytes, dev):
        self.region = torch.full((nbytes,), POISON, dtype=torch.uint8, device=dev)
        self.ptr = self.region.data_ptr()

    def snapshot(self):
        return self.region.cpu().numpy().tobytes()


def run_placed(torch, stage, guarded):
    """One call of the stage with every plane placed; returns {plane: array} of everything the stage may write."""
    dev = torch.device("cuda", 0)
    regions, ptr = {}, {}
    for pl in stage.planes:
        if guarded:
            g = G.GuardedWs(torch, pl.nbytes, POISON, dev, offset=pl.align)
            assert g.ptr % pl.align == 0 and g.ptr % (2 * pl.align) != 0, (stage.name, pl.name)
        else:
            g = Ordinary(torch, pl.nbytes, dev)
        if pl.data is not None:
            g.region.copy_(torch.from_numpy(np.frombuffer(pl.data.tobytes(), np.uint8).copy()).to(dev))
        regions[pl.name], ptr[pl.name] = g, g.ptr
    for arg, target in stage.aliases.items():
        ptr[arg] = ptr[target]
    stage.call(ptr)
    torch.cuda.synchronize()
    got = {}
    for pl in stage.planes:
        what = "%s, plane %s (%d bytes, %d-byte aligned)" % (stage.name, pl.name, pl.nbytes, pl.align)
        if guarded:
            regions[pl.name].assert_guards(what)
        raw = regions[pl.name].snapshot()
        if pl.role == "in":
            assert raw == pl.data.tobytes(), what + ": the input was changed"
        elif pl.role != "scratch":
            got[pl.name] = np.frombuffer(raw, pl.dtype).reshape(pl.shape)
    return got


def check(torch, stage):
    """The stage in ordinary allocations, then between guards at the lowest alignments: the same bytes, and the reference's."""
    plain = run_placed(torch, stage, False)
    placed = run_placed(torch, stage, True)
    assert plain.keys() == placed.keys()
    for name, a in plain.items():
        b = placed[name]
        ndiff = int((np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).sum())
        assert ndiff == 0, "%s: plane %s differs from the ordinary placement in %d of %d bytes" % (stage.name, name, ndiff, a.nbytes)
    if stage.ref is not None:
        stage.ref(placed)
    print("%s: %d planes placed, %d output bytes equal to the ordinary placement%s"
          % (stage.name, len(stage.planes), sum(a.nbytes for a in plain.values()), ", and the reference's" if stage.ref else ""))
    return placed


class Env:
    """What the calls share: the library, the stream, and workspaces that live until the stage has been judged."""

    def __init__(self, torch):
        self.torch, self.L = torch, pkg("_lib")
        self.dev = torch.device("cuda", 0)
        self.keep = []

    @property
    def st(self):
        return self.L.stream(self.dev)

    def ws(self, nbytes):
        t = self.torch.empty(max(int(nbytes), 1), dtype=self.torch.uint8, device=self.dev)
        self.keep.append(t)
        return t.data_ptr(), int(nbytes)

    def frame_ws(self, size_fn, h, w):
        n = int(getattr(self.L.lib(), size_fn)(h, w))
        assert n > 0, size_fn
        return self.ws(n)


def same_words(got, want, what):
    """The same elements in the same order, byte for byte."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, want.dtype, got.shape, want.shape)
    ndiff = int((got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8)).sum())
    assert ndiff == 0, "%s: %d of %d bytes differ" % (what, ndiff, got.nbytes)


# ================================================================================================ image-plane stages
def st_canny(E, h, w):
    import canny_ref as CR
    import test_gpu_canny as TC
    img = TC.noise_image(h, w, seed=h + w)
    P = Planes("dflow_canny_edges")

    def call(q):
        E.L.call("dflow_canny_edges", h, w, q["d_bgr"], 20.0, 40.0, q["d_edges"], q["d_ivice"], *E.frame_ws("dflow_canny_workspace_bytes", h, w), E.st)

    def ref(got):
        want = CR.canny(img, 20, 40)
        same_words(got["d_edges"], want.astype(np.uint8), "canny edges")
        same_words(got["d_ivice"], CR.ivice(want), "canny ivice")
    return [Stage("canny %dx%d" % (h, w), [P.inp("d_bgr", img), P.out("d_edges", np.uint8, (h, w)), P.out("d_ivice", F, (h, w))], call, ref=ref)]


def st_pb(E, h, w):
    import test_gpu_pb as TP
    img = TP.random_image(h, w, seed=5)
    P = Planes("dflow_pb_edges")

    def call(q):
        E.L.call("dflow_pb_edges", h, w, q["d_bgr"], 5, q["d_strength"], q["d_orient_strength"], *E.frame_ws("dflow_pb_workspace_bytes", h, w), E.st)

    def ref(got):
        _, _, e32, m32 = TP.reference("placement%dx%d" % (h, w), img, 5)
        same_words(got["d_strength"], e32, "pb strength")
        same_words(got["d_orient_strength"], m32, "pb orientation strengths")
    return [Stage("pb %dx%d" % (h, w), [P.inp("d_bgr", img), P.out("d_strength", F, (h, w)), P.out("d_orient_strength", F, (h, w, 8))], call, ref=ref)]


def st_epic(E, h, w):
    import test_gpu_epic as TE
    sp, e = TE.random_field(h, w, 0.3, seed=3 + h, edge_style="sparse")
    sp[h // 2, w // 3] = (2.0, -1.0, 1.0)
    P, n, nn = Planes("dflow_epic_interpolate"), h * w, 3
    out = []
    for method, name in ((0, "LA"), (1, "NW")):
        def call(q, method=method):
            E.L.call("dflow_epic_interpolate", h, w, q["d_sparse"], q["d_edges"], nn, 0.8, method, q["d_flow"], q["d_seed_of"], q["d_dist"],
                     q["d_lists"], q["d_list_g"], *E.frame_ws("dflow_epic_workspace_bytes", h, w), E.st)
        out.append(Stage("epic %s %dx%d" % (name, h, w),
                         [P.inp("d_sparse", sp), P.inp("d_edges", e), P.out("d_flow", F, (h, w, 2)), P.out("d_seed_of", np.int32, (h, w)),
                          P.out("d_dist", np.uint32, (h, w)), P.out("d_lists", np.int32, (n, nn)), P.out("d_list_g", np.uint64, (n, nn))], call))
    return out


def st_epic_prefilter(E, h, w):
    import epic_prefilter_cases as PC
    sp, e = PC.random_field(h, w, 0.3, seed=100 * h + w)
    sp[0, 0] = (1.5, -0.5, 1.0)
    img = np.random.default_rng(2).integers(0, 256, (h, w, 3)).astype(np.uint8) if h * w < 64 else PC.synth_image(h, w, 7)
    P = Planes("dflow_epic_prefilter")

    def call(q):
        E.L.call("dflow_epic_prefilter", h, w, q["d_bgr"], q["d_sparse_in"], q["d_edges"], 0.045, 8, 3.0, 0.8, q["d_sparse_out"], q["d_reason"],
                 q["d_saliency"], q["d_estimate"], *E.frame_ws("dflow_epic_prefilter_workspace_bytes", h, w), E.st)
    aux = [P.out("d_reason", np.uint8, (h, w)), P.out("d_saliency", F, (h, w)), P.out("d_estimate", F, (h, w, 2))]
    two = Stage("prefilter %dx%d" % (h, w), [P.inp("d_bgr", img), P.inp("d_sparse_in", sp), P.inp("d_edges", e), P.out("d_sparse_out", F, (h, w, 3))] + aux, call)
    kept = {}

    def ref_in_place(got):
        same_words(got["d_sparse_in"], kept["out"], "d_sparse_out == d_sparse_in")
    two.ref = lambda got: kept.update(out=got["d_sparse_out"])
    one = Stage("prefilter in place %dx%d" % (h, w), [P.inp("d_bgr", img), P.io("d_sparse_in", sp), P.inp("d_edges", e)] + aux, call,
                aliases={"d_sparse_out": "d_sparse_in"}, ref=ref_in_place)
    return [two, one]


def st_var(E, h, w):
    import variational_cases as VC
    img1, img2, flow, _ = VC.synth_case(h, w, seed=100 * h + w)
    P, L = Planes("dflow_var_refine"), E.L
    out, kept = [], {}
    for flags, name in ((0, "fused"), (L.VAR_FLAG_SOR_UNFUSED, "unfused")):
        vp = L.VarParams()
        L.lib().dflow_var_default_params(C.byref(vp))
        vp.niter_outer, vp.niter_solver, vp.flags = 1, 7, flags

        def call(q, vp=vp):
            L.call("dflow_var_refine", h, w, q["d_bgr1"], q["d_bgr2"], q["d_flow_in"], C.byref(vp), q["d_flow_out"],
                   *E.frame_ws("dflow_var_workspace_bytes", h, w), E.st)

        def ref(got, name=name):
            kept.setdefault("out", got["d_flow_out"])
            same_words(got["d_flow_out"], kept["out"], "variational %s against fused" % name)
        out.append(Stage("variational %s %dx%d" % (name, h, w),
                         [P.inp("d_bgr1", img1), P.inp("d_bgr2", img2), P.inp("d_flow_in", flow), P.out("d_flow_out", F, (h, w, 2))], call, ref=ref))
        if not flags:
            out.append(Stage("variational in place %dx%d" % (h, w), [P.inp("d_bgr1", img1), P.inp("d_bgr2", img2), P.io("d_flow_in", flow)], call,
                             aliases={"d_flow_out": "d_flow_in"}, ref=lambda got: same_words(got["d_flow_in"], kept["out"], "d_flow_out == d_flow_in")))
    return out


def st_eval(E, h, w):
    import test_gpu_eval as TEV
    test, gt, want = TEV.case(h, w)
    P = Planes("dflow_flow_eval")

    def call(q):
        E.L.call("dflow_flow_eval", h, w, q["d_test"], UVV, q["d_gt"], 3.0, 0, q["d_stats"], q["d_err"], q["d_err_bgr"],
                 *E.frame_ws("dflow_eval_workspace_bytes", h, w), E.st)

    def ref(got):
        st = E.L.EvalStats.from_buffer_copy(got["d_stats"].tobytes())
        for k in TEV.COUNTS:
            assert getattr(st, k) == want[k], (k, getattr(st, k), want[k])
        assert st.max_err == want["max_err"]
        same_words(got["d_err"].view(np.uint32), want["err"].view(np.uint32), "eval err")
        same_words(got["d_err_bgr"], want["bgr"], "eval picture")
    return [Stage("eval %dx%d" % (h, w), [P.inp("d_test", test), P.inp("d_gt", gt), P.out("d_stats", np.uint8, (64,)), P.out("d_err", F, (h, w)),
                                           P.out("d_err_bgr", np.uint8, (h, w, 3))], call, ref=ref)]


def st_color(E, h, w):
    import flowpic_ref as R
    flow, planted = R.color_case(h, w, 4.0)
    P = Planes("dflow_flow_color")

    def call(q):
        E.L.call("dflow_flow_color", h, w, q["d_flow"], UVV, 0.0, q["d_bgr"], q["d_maxrad"], *E.frame_ws("dflow_flow_color_workspace_bytes", h, w), E.st)

    def ref(got):
        # what the definition fixes to the bit (atan2 is the one operation it leaves open): the radius, the planted pixels, the unknown ones
        want = R.flow_color(flow, 0.0)
        same_words(got["d_maxrad"], np.array([want["maxrad"]], F), "colour radius")
        at = np.unravel_index(planted, (h, w))
        assert np.array_equal(got["d_bgr"][at], want["bgr"][at]) and not got["d_bgr"][~want["known"]].any()
    return [Stage("colour %dx%d" % (h, w), [P.inp("d_flow", flow), P.out("d_bgr", np.uint8, (h, w, 3)), P.out("d_maxrad", F, (1,))], call, ref=ref)]


def st_warp(E, h, w):
    import flowpic_ref as R
    import test_gpu_flowpic as TF
    img1, img2, flow, _ = R.warp_case(h, w, 4.0)
    P = Planes("dflow_warp_eval")

    def call(q):
        E.L.call("dflow_warp_eval", h, w, q["d_bgr1"], q["d_bgr2"], q["d_flow"], UVV, 10.0, 30.0, 0, q["d_stats"], q["d_warped"], q["d_err"],
                 q["d_err_bgr"], *E.frame_ws("dflow_warp_eval_workspace_bytes", h, w), E.st)

    def ref(got):
        want = R.warp(img1, img2, flow, 10.0, 30.0)
        st = E.L.PhotoStats.from_buffer_copy(got["d_stats"].tobytes())
        for k in TF.COUNTS:
            assert getattr(st, k) == want[k], (k, getattr(st, k), want[k])
        assert st.max_err == want["max_err"]
        same_words(got["d_err"].view(np.uint32), want["err"].view(np.uint32), "warp err")
        same_words(got["d_warped"], want["warped"], "warped image")
        same_words(got["d_err_bgr"], want["bgr"], "warp picture")
    return [Stage("warp %dx%d" % (h, w), [P.inp("d_bgr1", img1), P.inp("d_bgr2", img2), P.inp("d_flow", flow), P.out("d_stats", np.uint8, (48,)),
                                           P.out("d_warped", np.uint8, (h, w, 3)), P.out("d_err", F, (h, w)), P.out("d_err_bgr", np.uint8, (h, w, 3))],
                  call, ref=ref)]


def advance_field(h, w):
    """The fields of test_gpu_workspace.test_flow_advance, [U,V,valid] layout."""
    rng = np.random.default_rng(h * 1000 + w)
    amp = max(1, min(h, w) // 3)
    flow = (rng.integers(-amp, amp + 1, (h, w, 2)) + rng.choice([0.0, 0.5], (h, w, 2), p=[0.7, 0.3])).astype(F)
    if h * w > 1:
        flow[0, 0] = (0.0, -0.0)
        flow[h - 1, w - 1] = (np.nan, 1.0)
    return np.ascontiguousarray(np.concatenate([flow[..., ::-1], (rng.random((h, w, 1)) > 0.2).astype(F)], axis=-1))


def st_advance(E, h, w):
    import prior_ref as R
    flow = advance_field(h, w)
    P = Planes("dflow_flow_advance")

    def call(q):
        E.L.call("dflow_flow_advance", h, w, q["d_flow"], UVV, E.L.ADVANCE_NEGATE, q["d_out"], q["d_counts"],
                 *E.frame_ws("dflow_flow_advance_workspace_bytes", h, w), E.st)

    def ref(got):
        want, counts = R.flow_advance(flow, R.NEGATE)
        assert got["d_counts"].tolist() == counts
        same_words(got["d_out"].view(np.uint32), want.view(np.uint32), "advanced flow")
    return [Stage("advance %dx%d" % (h, w), [P.inp("d_flow", flow), P.out("d_out", F, (h, w, 3)), P.out("d_counts", np.int32, (3,))], call, ref=ref)]


def st_pyr_down(E, h, w):
    import pyramid_ref as R
    import test_gpu_pyramid as TPY
    a, b = TPY.image("random", h, w), TPY.image("random", h, w, seed=1)
    hc, wc = R.coarse_size(h, w)
    P = Planes("dflow_pyr_down")

    def call(q):
        E.L.call("dflow_pyr_down", h, w, q["d_in1"], q["d_in2"], q["d_out1"], q["d_out2"], E.st)

    def ref(got):
        same_words(got["d_out1"], R.pyr_down(a), "pyr_down, first image")
        same_words(got["d_out2"], R.pyr_down(b), "pyr_down, second image")
    return [Stage("pyr_down %dx%d" % (h, w), [P.inp("d_in1", a), P.inp("d_in2", b), P.out("d_out1", np.uint8, (hc, wc, 3)),
                                               P.out("d_out2", np.uint8, (hc, wc, 3))], call, ref=ref)]


def st_upsample(E, h, w):
    import pyramid_ref as R
    import test_gpu_pyramid as TPY
    f = TPY.coarse_flow(h, w, "uvv")
    P = Planes("dflow_flow_upsample")

    def call(q):
        E.L.call("dflow_flow_upsample", h, w, q["d_coarse"], UVV, q["d_out"], q["d_counts"], E.st)

    def ref(got):
        want, counts = R.flow_upsample(f, (h, w))
        assert got["d_counts"].tolist() == counts
        same_words(got["d_out"].view(np.uint32), want.view(np.uint32), "upsampled flow")
    return [Stage("upsample %dx%d" % (h, w), [P.inp("d_coarse", f), P.out("d_out", F, (h, w, 3)), P.out("d_counts", np.int32, (3,))], call, ref=ref)]


def st_consistency(E, h, w):
    import consistency_ref as R
    import test_gpu_consistency as TCO
    fwd, bwd = TCO.fields(h, w, "fractional", 3)
    P = Planes("dflow_flow_consistency")

    def call(q):
        E.L.call("dflow_flow_consistency", h, w, q["d_fwd"], UVV, q["d_bwd"], UVV, 4.0, E.L.FBC_BILINEAR, q["d_out_fwd"], q["d_out_bwd"],
                 q["d_err_fwd"], q["d_err_bwd"], q["d_counts"], E.st)

    def ref(got):
        want = R.flow_consistency(fwd, bwd, 4.0, R.BILINEAR, both=True)
        assert got["d_counts"].tolist() == want[4]
        for name, v in zip(("d_out_fwd", "d_out_bwd", "d_err_fwd", "d_err_bwd"), want[:4]):
            TCO.same_bits(got[name], v, name)       # a NaN must meet a NaN: IEEE 754 leaves its payload open
    return [Stage("consistency %dx%d" % (h, w), [P.inp("d_fwd", fwd), P.inp("d_bwd", bwd), P.out("d_out_fwd", F, (h, w, 3)),
                                                  P.out("d_out_bwd", F, (h, w, 3)), P.out("d_err_fwd", F, (h, w)), P.out("d_err_bwd", F, (h, w)),
                                                  P.out("d_counts", np.int32, (10,))], call, ref=ref)]


def st_segments(E, h, w):
    import test_gpu_segments as TS
    f = TS.blocks(h, w, 0.75, 12)
    P = Planes("dflow_segment_filter")

    def call(q):
        E.L.call("dflow_segment_filter", h, w, q["d_flow"], UVV, 2.0, 12, 0, q["d_out"], q["d_segment"], q["d_size"], q["d_counts"],
                 *E.frame_ws("dflow_segment_filter_workspace_bytes", h, w), E.st)

    def ref(got, out="d_out"):
        want = TS.reference(("placement", h, w), f, 2.0, 12)
        TS.same((got[out], got["d_segment"], got["d_size"], got["d_counts"].tolist()), want, "segments %dx%d" % (h, w))
    aux = [P.out("d_segment", np.int32, (h, w)), P.out("d_size", np.int32, (h, w)), P.out("d_counts", np.int32, (4,))]
    return [Stage("segments %dx%d" % (h, w), [P.inp("d_flow", f), P.out("d_out", F, (h, w, 3))] + aux, call, ref=ref),
            Stage("segments in place %dx%d" % (h, w), [P.io("d_flow", f)] + aux, call, aliases={"d_out": "d_flow"},
                  ref=lambda got: ref(got, "d_flow"))]


def st_frame_interp(E, h, w):
    import frame_interp_ref as R
    import test_gpu_frame_interp as TFI
    img1, img2 = R.images(h, w, 11)
    fwd, bwd = R.flow_field(h, w, 12, "frac"), R.flow_field(h, w, 13, "frac")
    P = Planes("dflow_frame_interp")

    def call(q):
        E.L.call("dflow_frame_interp", h, w, q["d_bgr1"], q["d_bgr2"], q["d_fwd"], UVV, q["d_bwd"], UVV, 0.5, 2, 30.0, 0, q["d_out"], q["d_keys"],
                 q["d_motion"], q["d_motion_tmp"], q["d_source"], q["d_counts"], E.st)

    def ref(got):
        want = R.frame_interp(img1, img2, fwd, bwd, t=0.5, fill_rounds=2, occl_thresh=30.0)
        TFI.same(dict(out=got["d_out"], keys=got["d_keys"], motion=got["d_motion"], source=got["d_source"], counts=got["d_counts"].tolist()),
                 want, "frame_interp %dx%d" % (h, w))
    return [Stage("frame_interp %dx%d" % (h, w),
                  [P.inp("d_bgr1", img1), P.inp("d_bgr2", img2), P.inp("d_fwd", fwd), P.inp("d_bwd", bwd), P.out("d_out", np.uint8, (h, w, 3)),
                   P.out("d_keys", np.uint64, (h, w)), P.out("d_motion", F, (h, w, 3)), P.out("d_motion_tmp", F, (h, w, 3), role="scratch"),
                   P.out("d_source", np.uint8, (h, w)), P.out("d_counts", np.int32, (8,))], call, ref=ref)]


def st_wmedian(E, h, w):
    import flow_wmedian_ref as R
    import test_gpu_flow_wmedian as TWM
    flow, bgr = R.field(h, w, 21, "holes"), R.image(h, w, 22)
    wspace, wcolor = R.tables(2, 1.5, 12.0)
    P = Planes("dflow_flow_wmedian")

    def call(q):
        E.L.call("dflow_flow_wmedian", h, w, q["d_flow"], UVV, q["d_bgr"], 2, q["d_wspace"], q["d_wcolor"], 0.0, 0, q["d_out"], q["d_counts"], E.st)

    def ref(got):
        want = R.flow_wmedian(flow, bgr, radius=2, wspace=wspace, wcolor=wcolor)
        TWM.same((got["d_out"], got["d_counts"].tolist()), want, "wmedian %dx%d" % (h, w))
    return [Stage("wmedian %dx%d" % (h, w), [P.inp("d_flow", flow), P.inp("d_bgr", bgr), P.inp("d_wspace", wspace), P.inp("d_wcolor", wcolor),
                                              P.out("d_out", F, (h, w, 3)), P.out("d_counts", np.int32, (4,))], call, ref=ref)]


def st_motion(E, h, w):
    import motion_ref as R
    import test_gpu_motion as TM
    flow, _, exclude = R.field(h, w, 31, "affine")
    P, n_hyp = Planes("dflow_motion_fit"), 64

    def call(q):
        E.L.call("dflow_motion_fit", h, w, q["d_flow"], UVV, q["d_exclude"], R.AFFINE, 1.0, n_hyp, 1, 2, 1, 0, 0, q["d_model"], q["d_models"],
                 q["d_hyp_counts"], q["d_state"], q["d_class"], q["d_model_flow"], q["d_residual"], q["d_counts"], E.st)

    def ref(got):
        want = R.fit(flow, exclude=exclude, model=R.AFFINE, thresh=1.0, n_hyp=n_hyp, lo_rounds=1, polish=2, step=1, seed=0)
        TM.same(dict(key=int(got["d_state"].view(np.uint64)[0]), hyp_counts=got["d_hyp_counts"], models=got["d_models"], model=got["d_model"],
                     model_flow=got["d_model_flow"], residual=got["d_residual"], cls=got["d_class"].reshape(-1), counts=got["d_counts"]),
                want, "motion_fit %dx%d" % (h, w))
    return [Stage("motion_fit %dx%d" % (h, w),
                  [P.inp("d_flow", flow), P.inp("d_exclude", exclude), P.out("d_model", F, (9,)), P.out("d_models", F, (n_hyp * 9,)),
                   P.out("d_hyp_counts", np.int32, (n_hyp,)), P.out("d_state", np.int64, (32,)), P.out("d_class", np.uint8, (h, w)),
                   P.out("d_model_flow", F, (h, w, 3)), P.out("d_residual", F, (h, w, 3)), P.out("d_counts", np.int32, (8,))], call, ref=ref)]


def st_gate(E, h, w):
    import label_conf_ref as R
    import test_gpu_label_conf as TLC
    uvv, score = TLC.gate_case(h, w, seed=h * w)
    P = Planes("dflow_flow_gate")

    def call(q):
        E.L.call("dflow_flow_gate", h, w, q["d_flow"], UVV, q["d_score"], -0.5, 0.75, q["d_out"], q["d_counts"], E.st)

    def ref(got, out="d_out"):
        want, counts = R.flow_gate_ref(uvv, score, -0.5, 0.75)
        assert got["d_counts"].tolist() == counts
        same_words(got[out].view(np.uint32), want.view(np.uint32), "gated flow")
    cnt = P.out("d_counts", np.int32, (2,))
    return [Stage("gate %dx%d" % (h, w), [P.inp("d_flow", uvv), P.inp("d_score", score), P.out("d_out", F, (h, w, 3)), cnt], call, ref=ref),
            Stage("gate in place %dx%d" % (h, w), [P.io("d_flow", uvv), P.inp("d_score", score), cnt], call, aliases={"d_out": "d_flow"},
                  ref=lambda got: ref(got, "d_flow"))]


# ================================================================================================ main path
class Pass:
    """The parameters, images and, stage after stage, the state of one pass (host arrays, from the ordinary placement's equal)."""

    def __init__(self, E, synth, geom, storage):
        L = E.L
        self.H, self.W, ch, cw = geom
        self.p = L.default_params(self.H, self.W, ch, cw, seed=5, flags=L.FLAG_DESCR_F16 if storage == "f16" else 0)
        self.pp, self.LP, self.f16 = C.byref(self.p), self.p.label_pitch, storage == "f16"
        self.img1, self.img2 = (np.ascontiguousarray(a, np.uint8) for a in synth.make_pair(self.H, self.W, seed=0, amp_x=0.1 * self.W, amp_y=0.1 * self.H)[:2])
        self.ddesc = (np.float16, (self.H, self.W, L.DESC_PITCH_F16)) if self.f16 else (F, (self.H, self.W, 68))
        self.ws_bytes = int(L.lib().dflow_workspace_bytes(self.pp))
        self.stats_ws = int(L.lib().dflow_bcd_stats_workspace_bytes(self.pp))
        assert self.ws_bytes > 0 and self.stats_ws > 0
        self.S = {}

    def with_flags(self, L, extra):
        q = L.Params.from_buffer_copy(self.p)
        q.flags |= extra
        return q

    def descr_f32(self, which):
        return np.ascontiguousarray(self.S[which][..., :68].astype(F))


def state_outs(P, ps):
    H, W, LP = ps.H, ps.W, ps.LP
    return [P.out("d_proposals", np.uint32, (H, W, LP)), P.out("d_lcosts", F, (H, W, LP)), P.out("d_nprop", np.int32, (H, W)),
            P.out("d_bestlabels", np.int32, (H, W))]


def ms_daisy(E, ps):
    P = Planes("dflow_daisy")
    got = check(E.torch, Stage("daisy", [P.inp("d_bgr", ps.img1), P.out("d_descr", *ps.ddesc)],
                               lambda q: E.L.call("dflow_daisy", ps.pp, q["d_bgr"], q["d_descr"], *E.ws(ps.ws_bytes), E.st)))
    ps.S["daisy"] = got["d_descr"]


def ms_daisy_pair(E, ps):
    P = Planes("dflow_daisy_pair")
    got = check(E.torch, Stage("daisy_pair", [P.inp("d_bgr1", ps.img1), P.inp("d_bgr2", ps.img2), P.out("d_descr1", *ps.ddesc), P.out("d_descr2", *ps.ddesc)],
                               lambda q: E.L.call("dflow_daisy_pair", ps.pp, q["d_bgr1"], q["d_bgr2"], q["d_descr1"], q["d_descr2"], *E.ws(ps.ws_bytes), E.st)))
    same_words(got["d_descr1"], ps.S["daisy"], "dflow_daisy_pair's first plane against dflow_daisy's")
    ps.S["descr1"], ps.S["descr2"] = got["d_descr1"], got["d_descr2"]


def ms_knn(E, ps):
    """Screened, exact (DFLOW_FLAG_KNN_EXACT) and timed: the header gives all three the same results bit for bit."""
    L = E.L
    exact = ps.with_flags(L, L.FLAG_KNN_EXACT)
    ms = (C.c_float * 8)()
    forms = (("knn screened", "dflow_knn_proposals", lambda a: L.call("dflow_knn_proposals", ps.pp, *a, *E.ws(ps.ws_bytes), E.st)),
             ("knn exact", "dflow_knn_proposals", lambda a: L.call("dflow_knn_proposals", C.byref(exact), *a, *E.ws(ps.ws_bytes), E.st)),
             ("knn timed", "dflow_knn_proposals_timed", lambda a: L.call("dflow_knn_proposals_timed", ps.pp, *a, *E.ws(ps.ws_bytes), E.st, ms, None)))
    names = ("d_descr1", "d_descr2", "d_proposals", "d_lcosts", "d_nprop", "d_bestlabels")
    first = None
    for what, fn, run in forms:
        P = Planes(fn)
        got = check(E.torch, Stage(what, [P.inp("d_descr1", ps.S["descr1"]), P.inp("d_descr2", ps.S["descr2"])] + state_outs(P, ps),
                                   lambda q, run=run: run([q[n] for n in names])))
        first = first or got
        for n in names[2:]:
            same_words(got[n], first[n], "%s: %s against the screened search's" % (what, n))
    assert (first["d_nprop"] > 0).all() and (first["d_nprop"] <= ps.p.maxnprop).all()
    for n in names[2:]:
        ps.S[n[2:]] = first[n]
    ps.S["wta"] = first["d_bestlabels"]


def ms_neighbour(E, ps):
    P, S = Planes("dflow_neighbour_proposals"), ps.S
    names = ("d_descr1", "d_descr2", "d_proposals", "d_lcosts", "d_nprop", "d_bestlabels")
    got = check(E.torch, Stage("neighbour", [P.inp("d_descr1", S["descr1"]), P.inp("d_descr2", S["descr2"]), P.io("d_proposals", S["proposals"]),
                                             P.io("d_lcosts", S["lcosts"]), P.io("d_nprop", S["nprop"]), P.inp("d_bestlabels", S["wta"])],
                               lambda q: E.L.call("dflow_neighbour_proposals", ps.pp, *[q[n] for n in names], *E.ws(ps.ws_bytes), E.st)))
    assert (got["d_nprop"] > S["nprop"]).any(), "labels were appended"
    S["proposals"], S["lcosts"], S["nprop"] = got["d_proposals"], got["d_lcosts"], got["d_nprop"]


def prepare_planes(ps):
    P, S = Planes("dflow_bcd_prepare"), ps.S
    return [P.inp("d_proposals", S["proposals"]), P.inp("d_lcosts", S["lcosts"])]


def ms_bcd_prepare(E, ps):
    P = Planes("dflow_bcd_prepare")
    check(E.torch, Stage("bcd_prepare", prepare_planes(ps) + [P.inp("d_nprop", ps.S["nprop"])],
                         lambda q: E.L.call("dflow_bcd_prepare", ps.pp, q["d_proposals"], q["d_lcosts"], q["d_nprop"], *E.ws(ps.ws_bytes), E.st)))


def ms_bcd_single(E, ps):
    """dflow_bcd_phase four times, then dflow_bcd_sweep, each on records prepared from the placed planes: the same labels."""
    L, S = E.L, ps.S
    for what in ("dflow_bcd_phase", "dflow_bcd_sweep"):
        P = Planes(what)

        def call(q, what=what):
            ws = E.ws(ps.ws_bytes)
            L.call("dflow_bcd_prepare", ps.pp, q["d_proposals"], q["d_lcosts"], q["d_nprop"], *ws, E.st)
            if what == "dflow_bcd_sweep":
                L.call(what, ps.pp, q["d_proposals"], q["d_nprop"], q["d_bestlabels"], *ws, E.st)
            else:
                for phase in range(4):
                    L.call(what, ps.pp, q["d_proposals"], q["d_nprop"], q["d_bestlabels"], phase, *ws, E.st)
        got = check(E.torch, Stage(what, prepare_planes(ps) + [P.inp("d_nprop", S["nprop"]), P.io("d_bestlabels", S["wta"])], call))
        assert (got["d_bestlabels"] != S["wta"]).any(), "the sweep moved labels"
        same_words(got["d_bestlabels"], S.setdefault("swept", got["d_bestlabels"]), what + " against the four phases")


def ms_bcd_batch(E, ps):
    """Three passes, every pass's planes in regions of their own: pass 0 starts from the WTA labels (and must end where the single
    sweep ends), pass 1 from label 0 everywhere, pass 2 from the swept labels."""
    L, S = E.L, ps.S
    starts = [S["wta"], np.zeros_like(S["wta"]), S["swept"]]
    first = None
    for what in ("dflow_bcd_phase_batch", "dflow_bcd_sweep_batch"):
        P = Planes(what)
        planes = prepare_planes(ps)
        for k in range(3):
            planes += [P.inp("d_nprop[]", S["nprop"], "d_nprop%d" % k), P.io("d_bestlabels[]", starts[k], "d_bestlabels%d" % k)]

        def call(q, what=what):
            wss = [E.ws(ps.ws_bytes) for _ in range(3)]
            for k in range(3):
                L.call("dflow_bcd_prepare", ps.pp, q["d_proposals"], q["d_lcosts"], q["d_nprop%d" % k], *wss[k], E.st)
            arr = lambda name: (C.c_void_p * 3)(*[q[name % k] for k in range(3)])       # noqa: E731
            d_ws = (C.c_void_p * 3)(*[w[0] for w in wss])
            if what == "dflow_bcd_sweep_batch":
                L.call(what, ps.pp, 3, arr("d_nprop%d"), arr("d_bestlabels%d"), d_ws, ps.ws_bytes, E.st)
            else:
                for phase in range(4):
                    L.call(what, ps.pp, 3, arr("d_nprop%d"), arr("d_bestlabels%d"), phase, d_ws, ps.ws_bytes, E.st)
        got = check(E.torch, Stage(what, planes, call))
        same_words(got["d_bestlabels0"], S["swept"], what + ": pass 0 against the single sweep")
        first = first or got
        for k in range(3):
            same_words(got["d_bestlabels%d" % k], first["d_bestlabels%d" % k], "%s: pass %d against dflow_bcd_phase_batch" % (what, k))
    S["batch"] = [first["d_bestlabels%d" % k] for k in range(3)]


def ms_bcd_stats(E, ps):
    L, S = E.L, ps.S
    P = Planes("dflow_bcd_stats")
    names = ("d_proposals", "d_lcosts", "d_nprop", "d_bestlabels", "d_prev_labels", "d_prev_out", "d_stats")
    ins = [P.inp("d_proposals", S["proposals"]), P.inp("d_lcosts", S["lcosts"]), P.inp("d_nprop", S["nprop"]), P.inp("d_bestlabels", S["swept"])]

    def call(q):
        L.call("dflow_bcd_stats", ps.pp, *[q[n] for n in names], *E.ws(ps.stats_ws), E.st)
    got = check(E.torch, Stage("bcd_stats", ins + [P.inp("d_prev_labels", S["wta"]), P.out("d_prev_out", np.int32, (ps.H, ps.W)),
                                                   P.out("d_stats", np.uint8, (48,))], call))
    same_words(got["d_prev_out"], S["swept"], "d_prev_out")
    st = L.BcdStats.from_buffer_copy(got["d_stats"].tobytes())
    assert st.n_changed == int((S["swept"] != S["wta"]).sum()) and st.n_bad_label == 0
    one = check(E.torch, Stage("bcd_stats, d_prev_out == d_prev_labels", ins + [P.io("d_prev_labels", S["wta"]), P.out("d_stats", np.uint8, (48,))], call,
                               aliases={"d_prev_out": "d_prev_labels"}))
    same_words(one["d_prev_labels"], S["swept"], "d_prev_labels after the in-place call")
    same_words(one["d_stats"], got["d_stats"], "the statistics of the in-place call")
    S["stats"] = got["d_stats"]


def ms_bcd_stats_batch(E, ps):
    L, S = E.L, ps.S
    P = Planes("dflow_bcd_stats_batch")
    labels = [S["swept"]] + S["batch"][1:]
    planes = [P.out("d_stats", np.uint8, (3 * 48,))]
    for k in range(3):
        planes += [P.inp("d_proposals[]", S["proposals"], "d_proposals%d" % k), P.inp("d_lcosts[]", S["lcosts"], "d_lcosts%d" % k),
                   P.inp("d_nprop[]", S["nprop"], "d_nprop%d" % k), P.inp("d_bestlabels[]", labels[k], "d_bestlabels%d" % k),
                   P.io("d_prev[]", S["wta"], "d_prev%d" % k)]

    def call(q):
        arr = lambda name: (C.c_void_p * 3)(*[q[name % k] for k in range(3)])       # noqa: E731
        L.call("dflow_bcd_stats_batch", ps.pp, 3, arr("d_proposals%d"), arr("d_lcosts%d"), arr("d_nprop%d"), arr("d_bestlabels%d"), arr("d_prev%d"),
               q["d_stats"], *E.ws(3 * ps.stats_ws), E.st)
    got = check(E.torch, Stage("bcd_stats_batch", planes, call))
    same_words(got["d_stats"][:48], S["stats"], "pass 0 of the batch against the single call")
    for k in range(3):
        same_words(got["d_prev%d" % k], labels[k], "d_prev[%d]" % k)


def ms_labels_to_flow(E, ps):
    P, S = Planes("dflow_labels_to_flow"), ps.S
    got = check(E.torch, Stage("labels_to_flow", [P.inp("d_proposals", S["proposals"]), P.inp("d_bestlabels", S["swept"]), P.out("d_flow", F, (ps.H, ps.W, 2))],
                               lambda q: E.L.call("dflow_labels_to_flow", ps.pp, q["d_proposals"], q["d_bestlabels"], q["d_flow"], E.st)))
    packed = np.take_along_axis(S["proposals"], S["swept"][..., None].astype(np.int64), axis=2)[..., 0]
    dy, dx = (packed & 0xFFFF).astype(np.uint16).view(np.int16), (packed >> 16).astype(np.uint16).view(np.int16)
    same_words(got["d_flow"], np.stack([dy, dx], axis=-1).astype(F), "the flow of the labels")
    S["flow"] = got["d_flow"]


def ms_fb_consistency(E, ps):
    P, S = Planes("dflow_fb_consistency"), ps.S
    rng = np.random.default_rng(ps.H)
    bwd = (-S["flow"] + rng.integers(-1, 2, S["flow"].shape)).astype(F)
    got = check(E.torch, Stage("fb_consistency", [P.inp("d_fwd", S["flow"]), P.inp("d_bwd", bwd), P.out("d_sparse", F, (ps.H, ps.W, 3))],
                               lambda q: E.L.call("dflow_fb_consistency", ps.pp, q["d_fwd"], q["d_bwd"], 1.0, q["d_sparse"], E.st)))
    valid = got["d_sparse"][..., 2]
    assert 0 < valid.sum() < valid.size and set(np.unique(valid)) == {0.0, 1.0}


def ms_pack_compat(E, ps):
    P, S = Planes("dflow_pack_compat"), ps.S
    kdim = ps.p.maxnprop * ps.p.maxnprop // 8 + 1
    got = check(E.torch, Stage("pack_compat", [P.inp("d_proposals", S["proposals"]), P.inp("d_nprop", S["nprop"]),
                                               P.out("d_packed", np.uint8, (ps.H, ps.W, 2, kdim))],
                               lambda q: E.L.call("dflow_pack_compat", ps.pp, q["d_proposals"], q["d_nprop"], q["d_packed"], E.st)))
    assert got["d_packed"].any() and not got["d_packed"][ps.H - 1, :, 0].any(), "no pixel below the last row"


def ms_prior(E, ps):
    import prior_ref as R
    P, S, L = Planes("dflow_prior_proposals"), ps.S, E.L
    prior = np.ascontiguousarray(np.concatenate([S["flow"][..., ::-1], np.ones((ps.H, ps.W, 1), F)], axis=-1))
    prior[3:9, 5:11, 2] = 0.0
    names = ("d_proposals", "d_lcosts", "d_nprop", "d_bestlabels", "d_counts")

    def ref(got):
        st = [S["proposals"].copy(), S["lcosts"].copy(), S["nprop"].astype(np.int64), S["wta"].astype(np.int64)]
        counts = R.prior_proposals(*st, ps.descr_f32("descr1"), ps.descr_f32("descr2"), prior, 2, R.SEED_LABELS, ps.p.maxnprop, ps.p.tphi)
        assert got["d_counts"].tolist() == counts
        same_words(got["d_proposals"], st[0], "proposals after the prior step")
        same_words(got["d_lcosts"].view(np.uint32), st[1].view(np.uint32), "lcosts after the prior step")
        assert np.array_equal(got["d_nprop"], st[2]) and np.array_equal(got["d_bestlabels"], st[3])
    check(E.torch, Stage("prior_proposals", [P.inp("d_descr1", S["descr1"]), P.inp("d_descr2", S["descr2"]), P.inp("d_prior", prior),
                                             P.io("d_proposals", S["proposals"]), P.io("d_lcosts", S["lcosts"]), P.io("d_nprop", S["nprop"]),
                                             P.io("d_bestlabels", S["wta"]), P.out("d_counts", np.int32, (4,))],
                         lambda q: L.call("dflow_prior_proposals", ps.pp, q["d_descr1"], q["d_descr2"], q["d_prior"], UVV, 2, L.PRIOR_SEED_LABELS,
                                          *[q[n] for n in names], E.st), ref=ref))


def ms_label_confidence(E, ps):
    import label_conf_ref as R
    import test_gpu_label_conf as TLC
    P, S, L = Planes("dflow_label_confidence"), ps.S, E.L
    H, W = ps.H, ps.W
    names = ("d_proposals", "d_lcosts", "d_nprop", "d_bestlabels")

    def ref(got):
        pk = S["proposals"]
        flows = np.stack([(pk & 0xFFFF).astype(np.uint16).view(np.int16), (pk >> 16).astype(np.uint16).view(np.int16)], axis=-1).astype(np.int64)
        want = TLC.expected(R.label_conf_ref(flows, S["lcosts"], S["nprop"], S["swept"], ps.p.tpsi, ps.p.lamda, mode=R.LOCAL, min_sep=1, thresh=0.25))
        TLC.compare(dict(margin=got["d_margin"].view(np.uint32).reshape(-1), alt=got["d_alt"].reshape(-1),
                         sparse=got["d_sparse"].view(np.uint32).reshape(-1), counts=got["d_counts"]), want, "label confidence")
    check(E.torch, Stage("label_confidence", [P.inp("d_proposals", S["proposals"]), P.inp("d_lcosts", S["lcosts"]), P.inp("d_nprop", S["nprop"]),
                                              P.inp("d_bestlabels", S["swept"]), P.out("d_margin", F, (H, W)), P.out("d_alt", np.int32, (H, W)),
                                              P.out("d_sparse", F, (H, W, 3)), P.out("d_counts", np.int32, (L.CONF_COUNTS,))],
                         lambda q: L.call("dflow_label_confidence", ps.pp, *[q[n] for n in names], L.CONF_LOCAL, 1, 0.25, q["d_margin"], q["d_alt"],
                                          q["d_sparse"], q["d_counts"], E.st), ref=ref))


# ================================================================================================ the table
# stage -> (the entry points it calls with placed planes, kind, builder).  "image": builder(E, h, w) -> [Stage]; "main":
# builder(E, pass) places, calls and judges, in this order, each on the state the ones before it left.
STAGES = {
    "canny": (("dflow_canny_edges",), "image", st_canny),
    "pb": (("dflow_pb_edges",), "image", st_pb),
    "epic": (("dflow_epic_interpolate",), "image", st_epic),
    "epic_prefilter": (("dflow_epic_prefilter",), "image", st_epic_prefilter),
    "variational": (("dflow_var_refine",), "image", st_var),
    "eval": (("dflow_flow_eval",), "image", st_eval),
    "colour": (("dflow_flow_color",), "image", st_color),
    "warp": (("dflow_warp_eval",), "image", st_warp),
    "advance": (("dflow_flow_advance",), "image", st_advance),
    "pyr_down": (("dflow_pyr_down",), "image", st_pyr_down),
    "upsample": (("dflow_flow_upsample",), "image", st_upsample),
    "consistency": (("dflow_flow_consistency",), "image", st_consistency),
    "segments": (("dflow_segment_filter",), "image", st_segments),
    "frame_interp": (("dflow_frame_interp",), "image", st_frame_interp),
    "wmedian": (("dflow_flow_wmedian",), "image", st_wmedian),
    "motion_fit": (("dflow_motion_fit",), "image", st_motion),
    "gate": (("dflow_flow_gate",), "image", st_gate),
    "daisy": (("dflow_daisy",), "main", ms_daisy),
    "daisy_pair": (("dflow_daisy_pair",), "main", ms_daisy_pair),
    "knn": (("dflow_knn_proposals", "dflow_knn_proposals_timed"), "main", ms_knn),
    "neighbour": (("dflow_neighbour_proposals",), "main", ms_neighbour),
    "bcd_prepare": (("dflow_bcd_prepare",), "main", ms_bcd_prepare),
    "bcd_single": (("dflow_bcd_phase", "dflow_bcd_sweep"), "main", ms_bcd_single),
    "bcd_batch": (("dflow_bcd_phase_batch", "dflow_bcd_sweep_batch"), "main", ms_bcd_batch),
    "bcd_stats": (("dflow_bcd_stats",), "main", ms_bcd_stats),
    "bcd_stats_batch": (("dflow_bcd_stats_batch",), "main", ms_bcd_stats_batch),
    "labels_to_flow": (("dflow_labels_to_flow",), "main", ms_labels_to_flow),
    "fb_consistency": (("dflow_fb_consistency",), "main", ms_fb_consistency),
    "pack_compat": (("dflow_pack_compat",), "main", ms_pack_compat),
    "prior_proposals": (("dflow_prior_proposals",), "main", ms_prior),
    "label_confidence": (("dflow_label_confidence",), "main", ms_label_confidence),
}
IMAGE_STAGES = [k for k, v in STAGES.items() if v[1] == "image"]
MAIN_STAGES = [k for k, v in STAGES.items() if v[1] == "main"]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@gpu
@pytest.mark.parametrize("size", IMAGE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("stage", IMAGE_STAGES)
def test_image_plane_stage(torch_, stage, size):
    E = Env(torch_)
    stages = STAGES[stage][2](E, *size)
    assert stages
    for st in stages:
        check(torch_, st)


@gpu
@pytest.mark.parametrize("geom,storage", GEOMS, ids=geom_ids)
def test_main_path_stage_after_stage(torch_, synth, geom, storage):
    E = Env(torch_)
    ps = Pass(E, synth, geom, storage)
    for stage in MAIN_STAGES:
        STAGES[stage][2](E, ps)
        E.keep.clear()


@gpu
def test_a_view_into_a_stack_is_cloned_where_a_stage_needs_16_bytes(torch_):
    """flows[1] of a stacked (2,45,35,3) float32 tensor is contiguous and starts 45*35*12 bytes in: 4-byte aligned only.
    dflow_flow_eval, dflow_flow_color and dflow_flow_gate ask for 16: the wrappers give the bytes they give on a fresh copy."""
    import test_gpu_label_conf as TLC
    torch, P = torch_, pkg("pipeline")
    H, W = 45, 35
    a, score = TLC.gate_case(H, W, seed=1)
    b, _ = TLC.gate_case(H, W, seed=2)
    a, b = np.nan_to_num(a, nan=1.5, posinf=2.5, neginf=-2.5), np.nan_to_num(b, nan=0.5, posinf=1.0, neginf=-1.0)
    stack = torch.from_numpy(np.stack([a, b])).cuda()
    view, gt = stack[1], stack[0].clone()
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
    fresh = view.clone()
    assert fresh.data_ptr() % 16 == 0
    raw = lambda t: t.cpu().numpy().tobytes()                                     # noqa: E731
    for x, y in zip(P.flow_eval(view, gt, 3.0, err=True, image=True), P.flow_eval(fresh, gt, 3.0, err=True, image=True)):
        assert raw(x) == raw(y), "flow_eval"
    assert raw(P.flow_eval(gt, view, 3.0)) == raw(P.flow_eval(gt, fresh, 3.0)), "flow_eval, the view as ground truth"
    assert raw(P.flow_color(view)) == raw(P.flow_color(fresh)), "flow_color"
    sc = torch.from_numpy(score).cuda()
    for x, y in zip(P.flow_gate(view, sc, lo=-0.5, hi=0.75, counts=True), P.flow_gate(fresh, sc, lo=-0.5, hi=0.75, counts=True)):
        assert raw(x) == raw(y), "flow_gate"
    assert raw(stack[1]) == raw(fresh), "the caller's tensor is left alone"


# ================================================================================================ host only
def takes_planes(names):
    return any(n.startswith("d_") and n != "d_ws" for n in names.split())


# the three entry points whose refusals tests/test_abi_motion.py and tests/test_abi_label_conf.py pin: a base call that the last
# check refuses (d_counts is an input's plane)
SHARED_GATE = {
    "dflow_motion_fit": ("h w d_flow layout d_exclude model thresh n_hyp lo_rounds polish step seed flags d_model d_models d_hyp_counts d_state "
                         "d_class d_model_flow d_residual d_counts stream",
                         dict(h=37, w=101, d_flow=TR.A, layout=0, d_exclude=TR.B, model=0, thresh=1.0, n_hyp=64, lo_rounds=1, polish=2, step=1,
                              seed=0, flags=0, d_model=TR.D, d_models=TR.E, d_hyp_counts=TR.F, d_state=TR.G, d_class=TR.H, d_model_flow=TR.I,
                              d_residual=TR.J, d_counts=TR.A, stream=None)),
    "dflow_label_confidence": ("p d_proposals d_lcosts d_nprop d_bestlabels mode min_sep thresh d_margin d_alt d_sparse d_counts stream",
                               dict(p=TR.GEOM, d_proposals=TR.A, d_lcosts=TR.B, d_nprop=TR.D, d_bestlabels=TR.E, mode=0, min_sep=1, thresh=0.0,
                                    d_margin=TR.F, d_alt=TR.G, d_sparse=TR.H, d_counts=TR.A, stream=None)),
    "dflow_flow_gate": ("h w d_flow layout d_score lo hi d_out d_counts stream",
                        dict(h=37, w=101, d_flow=TR.A, layout=0, d_score=TR.B, lo=-1.0, hi=1.0, d_out=TR.D, d_counts=TR.A, stream=None)),
}
# the plane the entry point's last check is about: a call with it in place would be launched, so only its refusal is made
CHECKED_LAST = {("dflow_labels_to_flow", "d_flow"), ("dflow_fb_consistency", "d_sparse"), ("dflow_pack_compat", "d_nprop")}
STAND_IN = 1 << 44                  # 4 GiB-aligned like TR's stand-ins, and none of them


def entry_points_with_planes():
    L = pkg("_lib")
    names = {n for n, (args, _, _) in TR.TABLES.items() if n not in TR.RETURNS_A_SIZE and takes_planes(args)} | set(SHARED_GATE)
    assert names <= set(L.SYMBOLS) and set(SHARED_GATE) == set(L._SIGNATURES_SHARED_GATE)
    return names


def test_the_tables_name_every_entry_point_that_takes_a_device_plane():
    """STAGES and ALIGN against the library's list, the way test_every_function_that_returns_a_status_has_a_table does."""
    want = entry_points_with_planes()
    assert "dflow_daisy" in want and "dflow_knn_screen_stats" not in want and len(want) == 34
    assert set(ALIGN) == want
    called = [fn for fns, _, _ in STAGES.values() for fn in fns]
    assert sorted(called) == sorted(want), sorted(set(want) ^ set(called))
    for fn, planes in ALIGN.items():
        args = (TR.TABLES[fn][0] if fn in TR.TABLES else SHARED_GATE[fn][0]).split()
        assert all(k.replace("[]", "") in args for k in planes), fn
        assert all(a in (1, 2, 4, 8, 16) for a in planes.values()), fn


def refusal(L, fn, values):
    names = TR.TABLES[fn][0] if fn in TR.TABLES else SHARED_GATE[fn][0]
    out = []

    def run():
        rc = getattr(L.lib(), fn)(*TR.marshal(L, names, values))
        out.append((rc, L.lib().dflow_last_error().decode()))
    t = TR.threading.Thread(target=run)          # the *_last_stats state and the last error belong to the calling thread
    t.start()
    t.join()
    assert out and out[0][0] in (-1, G.ENOSPC), "%s was not refused by its gate: %r" % (fn, out)       # DFLOW_EHIP: something was launched
    return out[0]


@pytest.mark.parametrize("fn", sorted(ALIGN))
def test_alignments_are_the_gates_of_abi_hip(fn):
    """Every plane of ALIGN, moved off its stand-in by its alignment (a multiple of it and of nothing coarser), is accepted, and
    moved by half of it the gate names the plane and the number.  As in tests/test_abi_refusals.py every call is refused, so
    nothing is launched on the stand-in pointers: the base call's own last fault stays in every call.  Where that fault is two
    arguments naming one plane they move together; where it is this plane's own boundary only the refusal is made."""
    L = pkg("_lib")
    if not TR.os.path.exists(L.LIB_PATH):
        L.build()
    base = dict(TR.TABLES[fn][1]) if fn in TR.TABLES else dict(SHARED_GATE[fn][1])
    refusal(L, fn, base)
    said_by = "dflow_bcd_phase" + fn[len("dflow_bcd_sweep"):] if fn.startswith("dflow_bcd_sweep") else fn      # a sweep is four phases
    sweeps_batch = fn in ("dflow_bcd_phase_batch", "dflow_bcd_sweep_batch")
    for plane, a in ALIGN[fn].items():
        arg, entry = plane.replace("[]", ""), plane.endswith("[]")

        def moved(offset, alone=False):
            v = dict(base)
            if entry:
                was = v[arg] if v[arg] is not None else [STAND_IN] * v["npass"]
                v[arg] = [was[0], was[1] + offset]
                if sweeps_batch:                                         # they look at the one size before the passes' pointers:
                    v["ws_bytes"], v["d_ws"] = TR.BIG, [TR.WS, TR.WS + 4096 + 8]     # the last check, a pass's d_ws, refuses instead
            elif alone:                                                  # off its boundary: this plane's own check refuses, or one before it
                v[arg] = STAND_IN + offset
            elif v[arg] is None:
                assert v.get("ws_bytes", 1) == 0, (fn, arg)               # the workspace check, after the planes, refuses
                v[arg] = STAND_IN + offset
            else:
                for k, x in base.items():                                # this plane and whatever the base call makes the same plane
                    if k.startswith("d_") and not isinstance(x, list) and x == base[arg]:
                        v[k] = x + offset
            return v
        name = "%s[1]" % arg if entry else arg
        if a > 1:
            assert refusal(L, fn, moved(a // 2, alone=True)) == (-1, "%s: %s is not %d-byte aligned" % (said_by, name, a)), (fn, plane)
        if (fn, arg) not in CHECKED_LAST:
            rc, msg = refusal(L, fn, moved(a))
            assert ": %s is not" % name not in msg, (fn, plane, msg)
