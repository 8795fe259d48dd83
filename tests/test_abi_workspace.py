"""What include/dflow.h says d_ws must be, on the host: every entry point that takes a workspace refuses one below its alignment
with DFLOW_EINVAL and names d_ws, still reports an argument error first and a short workspace last, and the exact per-stage
sizes (ws_guard.stage_need) agree with the public size functions.  Every refusal precedes the launches: CPU only."""
import ctypes as C
import os
import re

import pytest

import ws_guard as G
from conftest import ROOT, pkg

PLANE = 1 << 32                                            # more than any plane of an 8192 x 8192 frame
A, B, D, E, F_, H_, I, J = (PLANE * k for k in range(1, 9))      # non-NULL, aligned, disjoint stand-ins for device pointers
WS = PLANE * 16
EINVAL, ENOSPC = -1, -2
HH, WW = 37, 101


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def params(L, H=40, W=48, ch=5, cw=6, **kw):
    return L.default_params(H, W, ch, cw, **kw)


def entry_points(L):
    """name -> (alignment the header states, call(ws, ws_bytes, bad=False)); bad=True breaks one other argument."""
    lib = L.lib()
    p = params(L)
    pp = C.byref(p)
    vp = L.VarParams()
    lib.dflow_var_default_params(C.byref(vp))
    ms, st = (C.c_float * 6)(), (C.c_int64 * 14)()
    one = lambda v: (C.c_void_p * 1)(v)                  # noqa: E731
    nul = lambda bad, v: None if bad else v              # noqa: E731
    # the screened search runs for these parameters: dflow_knn_proposals checks a workspace (and launches nothing below)
    assert G.stage_need("dflow_knn_proposals", pp, *[G.PTR] * 6) > 0
    return {
        "dflow_daisy": (16, lambda ws, n, bad=False: lib.dflow_daisy(pp, nul(bad, A), B, ws, n, None)),
        "dflow_daisy_pair": (16, lambda ws, n, bad=False: lib.dflow_daisy_pair(pp, A, B, D, nul(bad, E), ws, n, None)),
        "dflow_knn_proposals": (16, lambda ws, n, bad=False: lib.dflow_knn_proposals(pp, A, B, D, E, F_, nul(bad, H_), ws, n, None)),
        "dflow_knn_proposals_timed": (16, lambda ws, n, bad=False: lib.dflow_knn_proposals_timed(pp, A, B, D, E, F_, nul(bad, H_), ws, n,
                                                                                                 None, ms, None)),
        "dflow_knn_screen_stats": (16, lambda ws, n, bad=False: lib.dflow_knn_screen_stats(pp, ws, n, None, nul(bad, st))),
        "dflow_knn_screen_stats_n": (16, lambda ws, n, bad=False: lib.dflow_knn_screen_stats_n(pp, ws, n, None, st, 15 if bad else 14)),
        "dflow_neighbour_proposals": (16, lambda ws, n, bad=False: lib.dflow_neighbour_proposals(pp, A, B, D, E, F_, nul(bad, H_), ws, n, None)),
        "dflow_bcd_prepare": (16, lambda ws, n, bad=False: lib.dflow_bcd_prepare(pp, A, B, nul(bad, D), ws, n, None)),
        "dflow_bcd_phase": (16, lambda ws, n, bad=False: lib.dflow_bcd_phase(pp, A, B, nul(bad, D), 0, ws, n, None)),
        "dflow_bcd_sweep": (16, lambda ws, n, bad=False: lib.dflow_bcd_sweep(pp, A, B, nul(bad, D), ws, n, None)),
        "dflow_bcd_stats": (8, lambda ws, n, bad=False: lib.dflow_bcd_stats(pp, A, B, D, E, None, None, nul(bad, F_), ws, n, None)),
        "dflow_bcd_stats_batch": (8, lambda ws, n, bad=False: lib.dflow_bcd_stats_batch(pp, 0 if bad else 1, one(A), one(B), one(D), one(E), None,
                                                                                         F_, ws, n, None)),
        "dflow_canny_edges": (4, lambda ws, n, bad=False: lib.dflow_canny_edges(HH, WW, A, 100.0, 200.0, nul(bad, B), None, ws, n, None)),
        "dflow_pb_edges": (2, lambda ws, n, bad=False: lib.dflow_pb_edges(HH, WW, A, 8 if bad else 5, B, None, ws, n, None)),
        "dflow_epic_interpolate": (8, lambda ws, n, bad=False: lib.dflow_epic_interpolate(HH, WW, A, B, 0 if bad else 16, 0.8, 0, D, None, None,
                                                                                           None, None, ws, n, None)),
        "dflow_epic_prefilter": (8, lambda ws, n, bad=False: lib.dflow_epic_prefilter(HH, WW, A, B, D, 0.045, 256 if bad else 25, 5.0, 0.8, E,
                                                                                       None, None, None, ws, n, None)),
        "dflow_var_refine": (4, lambda ws, n, bad=False: lib.dflow_var_refine(HH, WW, A, B, D, C.byref(vp), nul(bad, E), ws, n, None)),
        "dflow_flow_eval": (8, lambda ws, n, bad=False: lib.dflow_flow_eval(HH, WW, A, 2 if bad else 0, B, 3.0, 0, D, None, None, ws, n, None)),
        "dflow_flow_color": (4, lambda ws, n, bad=False: lib.dflow_flow_color(HH, WW, A, 0, -1.0 if bad else 0.0, B, None, ws, n, None)),
        "dflow_warp_eval": (8, lambda ws, n, bad=False: lib.dflow_warp_eval(HH, WW, A, B, D, 0, 10.0, 0.0 if bad else 30.0, 0, E, None, None,
                                                                             None, ws, n, None)),
        "dflow_flow_advance": (4, lambda ws, n, bad=False: lib.dflow_flow_advance(HH, WW, A, 0, 2 if bad else 0, B, None, ws, n, None)),
        "dflow_segment_filter": (4, lambda ws, n, bad=False: lib.dflow_segment_filter(HH, WW, A, 0, 1.0, -1 if bad else 20, 0, B, D, E, F_,
                                                                                       ws, n, None)),
    }


BATCH = ("dflow_bcd_phase_batch", "dflow_bcd_sweep_batch")
REPORTS_AS = {"dflow_knn_screen_stats": "dflow_knn_screen_stats_n", "dflow_bcd_sweep": "dflow_bcd_phase"}     # the function that checks


def test_every_entry_point_with_a_workspace_is_listed(L):
    """The table above and the two batch entry points are all the functions of the binding that take a ws_bytes."""
    with_ws = {name for name, (_, argtypes) in L._SIGNATURES.items() if C.c_size_t in argtypes}
    assert with_ws == set(entry_points(L)) | set(BATCH)


def test_the_header_states_an_alignment_for_every_entry_point(L):
    """The Conventions block of include/dflow.h lists every entry point under the alignment this file tests."""
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    block = header[header.index("Alignment of d_ws"):header.index("Device layouts")]
    groups = {int(m.group(1)): m.group(2) for m in re.finditer(r"\n \*\s+(16|8|4|2)  (.*?)(?=\n \*\s+(?:16|8|4|2)  |\n \*     A d_ws)", block, re.S)}
    assert set(groups) == {16, 8, 4, 2}
    for name, (align, _) in entry_points(L).items():
        short = name[:-2] if name == "dflow_knn_screen_stats_n" else name
        assert short in groups[align], (name, align)
    for name in BATCH:
        assert name in groups[16]


def test_a_workspace_one_alignment_step_too_low_is_refused(L):
    lib = L.lib()
    for name, (align, call) in entry_points(L).items():
        for off in sorted({align // 2, align // 2 + align} | ({1, align - 1} if align > 2 else set())):
            assert call(WS + off, 1 << 40) == EINVAL, (name, off, lib.dflow_last_error())
            assert lib.dflow_last_error().decode() == "%s: d_ws is not %d-byte aligned" % (REPORTS_AS.get(name, name), align)
        # at the stated alignment and no more the call gets as far as the size check: the header asks for nothing stricter
        for off in (0, align, 3 * align):
            assert call(WS + off, 0) == ENOSPC and b"workspace 0 <" in lib.dflow_last_error(), (name, off, lib.dflow_last_error())
        # a NULL workspace is a short one, whatever its size
        assert call(None, 1 << 40) == ENOSPC and b"workspace" in lib.dflow_last_error(), name


# the entry points that have always named d_ws among their aligned pointers: they check it before its size
ALIGNMENT_FIRST = ("dflow_bcd_stats", "dflow_bcd_stats_batch", "dflow_flow_advance", "dflow_segment_filter")


def test_an_argument_error_comes_first_then_a_short_workspace(L):
    lib = L.lib()
    for name, (align, call) in entry_points(L).items():
        # a bad argument with a misaligned, a short and a NULL workspace: the argument is what is reported
        for ws, n in ((WS + align // 2, 1 << 40), (WS, 0), (None, 0), (WS + align // 2, 0)):
            assert call(ws, n, bad=True) == EINVAL and b"d_ws" not in lib.dflow_last_error(), (name, ws, n, lib.dflow_last_error())
        # misaligned and short
        rc = call(WS + align // 2, 0)
        if name in ALIGNMENT_FIRST:
            assert rc == EINVAL and b"d_ws is not" in lib.dflow_last_error(), name
        else:
            assert rc == ENOSPC and b"workspace 0 <" in lib.dflow_last_error(), name


def test_batch_workspaces_are_checked_one_by_one(L):
    lib = L.lib()
    p = params(L, 24, 40, 6, 8)
    need = G.stage_need("dflow_bcd_prepare", C.byref(p), G.PTR, G.PTR, G.PTR)
    n = 9
    arr = lambda vals: (C.c_void_p * n)(*vals)           # noqa: E731
    npr, bl = arr([A] * n), arr([B] * n)
    good = [WS + 4096 * k for k in range(n)]
    calls = {"dflow_bcd_phase_batch": lambda ws, nb=need, npass=n: lib.dflow_bcd_phase_batch(C.byref(p), npass, npr, bl, 0, arr(ws), nb, None),
             "dflow_bcd_sweep_batch": lambda ws, nb=need, npass=n: lib.dflow_bcd_sweep_batch(C.byref(p), npass, npr, bl, arr(ws), nb, None)}
    for name, call in calls.items():
        for k in (0, 7, 8):                                # the first pass, the last of the first launch, the pass of the second
            for off in (8, 4, 1, 24):
                ws = list(good)
                ws[k] += off
                assert call(ws) == EINVAL, (name, k, off)
                assert lib.dflow_last_error().decode() == "dflow_bcd_phase_batch: d_ws[%d] is not 16-byte aligned" % k
            ws = list(good)
            ws[k] += 16
            assert call(ws, nb=need - 1) == ENOSPC and b"workspace" in lib.dflow_last_error(), (name, k)
        # an argument error first, a short workspace before the per-pass pointers (as it always was)
        bad = list(good)
        bad[3] += 8
        assert call(bad, npass=0) == EINVAL and b"npass" in lib.dflow_last_error()
        assert call(bad, nb=need - 1) == ENOSPC
        bad[2] = None
        assert call(bad) == EINVAL and b"pass 2 has a NULL pointer" in lib.dflow_last_error()


IMAGE_PLANE = {"dflow_canny_edges": ("dflow_canny_workspace_bytes", lambda h, w: (h, w, A, 100.0, 200.0, B, None)),
               "dflow_pb_edges": ("dflow_pb_workspace_bytes", lambda h, w: (h, w, A, 5, B, None)),
               "dflow_epic_interpolate": ("dflow_epic_workspace_bytes", lambda h, w: (h, w, A, B, 16, 0.8, 0, D, None, None, None, None)),
               "dflow_epic_prefilter": ("dflow_epic_prefilter_workspace_bytes",
                                        lambda h, w: (h, w, A, B, D, 0.045, 25, 5.0, 0.8, E, None, None, None)),
               "dflow_flow_eval": ("dflow_eval_workspace_bytes", lambda h, w: (h, w, A, 0, B, 3.0, 0, D, None, None)),
               "dflow_flow_color": ("dflow_flow_color_workspace_bytes", lambda h, w: (h, w, A, 0, 0.0, B, None)),
               "dflow_warp_eval": ("dflow_warp_eval_workspace_bytes", lambda h, w: (h, w, A, B, D, 0, 10.0, 30.0, 0, E, None, None, None)),
               "dflow_flow_advance": ("dflow_flow_advance_workspace_bytes", lambda h, w: (h, w, A, 0, 0, B, None)),
               "dflow_segment_filter": ("dflow_segment_filter_workspace_bytes", lambda h, w: (h, w, A, 0, 1.0, 20, 0, B, D, E, F_))}


@pytest.mark.parametrize("size", [(1, 1), (37, 101), (1025, 1027), (8192, 8192)], ids=lambda s: "%dx%d" % s)
def test_stage_need_agrees_with_the_public_size_functions(L, size):
    lib = L.lib()
    h, w = size
    for name, (size_fn, args) in IMAGE_PLANE.items():
        assert G.stage_need(name, *args(h, w)) == getattr(lib, size_fn)(h, w) > 0, name
    vp = L.VarParams()
    lib.dflow_var_default_params(C.byref(vp))
    assert G.stage_need("dflow_var_refine", h, w, A, B, D, C.byref(vp), E) == lib.dflow_var_workspace_bytes(h, w) > 0
    if h >= 8 and w >= 8 or h * w == 1:
        p = L.default_params(h, w, 1, 1)
        need = G.stage_need("dflow_bcd_stats", C.byref(p), A, B, D, E, None, None, F_)
        assert need == lib.dflow_bcd_stats_workspace_bytes(C.byref(p)) > 0
        one = lambda v: (C.c_void_p * 9)(*[v] * 9)       # noqa: E731
        assert G.stage_need("dflow_bcd_stats_batch", C.byref(p), 9, one(A), one(B), one(D), one(E), None, F_) == 9 * need


def test_stage_need_fails_loudly(L):
    p = params(L)
    with pytest.raises(AssertionError, match="expected DFLOW_ENOSPC"):
        G.stage_need("dflow_bcd_prepare", C.byref(p), G.PTR, G.PTR, None)            # DFLOW_EINVAL: d_nprop is NULL
    with pytest.raises(AssertionError, match="expected DFLOW_ENOSPC"):
        G.stage_need("dflow_knn_proposals", C.byref(params(L, flags=L.FLAG_KNN_EXACT)), *[G.PTR] * 6)   # the brute-force search takes none
    with pytest.raises(AssertionError, match="arguments in front of d_ws"):
        G.stage_need("dflow_bcd_prepare", C.byref(p), G.PTR)
    with pytest.raises(AssertionError, match="takes no workspace"):
        G.stage_need("dflow_labels_to_flow", C.byref(p), G.PTR, G.PTR, G.PTR)


def main_path_needs(L, p):
    pp, P = C.byref(p), G.PTR
    return {"dflow_daisy": G.stage_need("dflow_daisy", pp, P, P),
            "dflow_daisy_pair": G.stage_need("dflow_daisy_pair", pp, P, P, P, P),
            "dflow_knn_proposals": G.stage_need("dflow_knn_proposals", pp, P, P, P, P, P, P),
            "dflow_neighbour_proposals": G.stage_need("dflow_neighbour_proposals", pp, P, P, P, P, P, P),
            "dflow_bcd_prepare": G.stage_need("dflow_bcd_prepare", pp, P, P, P),
            "dflow_bcd_phase": G.stage_need("dflow_bcd_phase", pp, P, P, P, 0)}


SLACK = 256                                                # include/dflow.h: "plus 256 spare bytes"
# the geometries of the GPU workspace tests in both storages, and the tight pair just above 64 labels of
# test_gpu_abi_edges.PITCHES on its frame
SETS = [((40, 48, 5, 6), {}, "f32"), ((40, 48, 5, 6), {}, "f16"), ((45, 35, 9, 7), {}, "f32"),
        ((60, 84, 10, 12), dict(window=1, ngauss=7, maxnprop=52, label_pitch=64), "f32"),
        ((60, 84, 10, 12), dict(window=2, ngauss=7, maxnprop=132, label_pitch=144), "f16")]


@pytest.mark.parametrize("geom,over,storage", SETS, ids=["40x48_f32", "40x48_f16", "45x35_f32", "60x84_lp64", "60x84_lp144_f16"])
def test_the_largest_stage_plus_the_slack_is_dflow_workspace_bytes(L, geom, over, storage):
    import test_gpu_abi_edges as AE
    if over:
        assert (over["window"], over["ngauss"], over["maxnprop"], over["label_pitch"], storage) in AE.PITCHES
    p = L.default_params(*geom, flags=L.FLAG_DESCR_F16 if storage == "f16" else 0, **over)
    needs = main_path_needs(L, p)
    print(geom, over, storage, needs)
    assert all(v > 0 and v % 256 == 0 for v in needs.values())
    assert needs["dflow_bcd_phase"] == needs["dflow_bcd_prepare"] and needs["dflow_daisy_pair"] == 2 * needs["dflow_daisy"]
    assert max(needs.values()) + SLACK == L.lib().dflow_workspace_bytes(C.byref(p))
    assert "plus %d spare bytes" % SLACK in open(os.path.join(ROOT, "include", "dflow.h")).read()


def test_the_guard_helper_itself(L):
    """GuardedWs on the host: layout, poison, alignment and offset, and that a byte written on either side is reported with its
    offset; `guarded` hands the wrappers' _lib.workspace exact regions, records them and puts the real function back."""
    import torch
    for need, poison, offset in ((1, 0x00, 0), (1000, 0xFF, 0), (4096, 0x7F, 8), (37, 0xFF, 4)):
        g = G.GuardedWs(torch, need, poison, "cpu", offset)
        assert g.nbytes == need == g.region.numel() and g.ptr == g.region.data_ptr() and g.ptr % 256 == offset
        assert g.start >= G.GUARD and g.buf.numel() - g.start - need >= G.GUARD
        assert (g.region == poison).all() and g.snapshot() == bytes([poison]) * need
        g.assert_guards("untouched")
        g.region.fill_(0x11)                                       # the stage's own bytes are its own
        g.assert_guards("region written")
        g.repoison()
        assert g.snapshot() == bytes([poison]) * need
        for at, text in ((g.start + need, r"offsets \+0 \.\. \+0 from its end"), (g.start + need + 300, r"offsets \+300 \.\. \+300"),
                         (g.start - 1, r"offsets -1 \.\. -1 from its start"), (g.start - G.GUARD, r"offsets -4096 \.\. -4096")):
            old = int(g.buf[at])
            g.buf[at] = poison
            with pytest.raises(AssertionError, match=text):
                g.assert_guards("one byte")
            g.buf[at] = old
        g.assert_guards("restored")
    assert all(p != G.GUARD_BYTE for p in G.POISONS) and G.POISONS == (0x00, 0xFF, 0x7F)
    real = L.workspace
    with G.guarded(torch, 0x7F, offset=4) as handed:
        assert L.workspace is not real
        ws, nbytes = L.workspace("dflow_flow_advance_workspace_bytes", 37, 101, "cpu")
        assert nbytes == L.lib().dflow_flow_advance_workspace_bytes(37, 101) == ws.numel() and ws.data_ptr() % 256 == 4
        assert (ws == 0x7F).all() and len(handed.all) == 1 and handed.all[0].region.data_ptr() == ws.data_ptr()
        with pytest.raises(L.DflowError, match="size"):
            L.workspace("dflow_flow_advance_workspace_bytes", 0, 101, "cpu")
        handed.assert_guards("nothing ran")
        ws[-1] = 0                                                 # inside
        handed.assert_guards("last byte of the region")
        handed.all[0].buf[handed.all[0].start + nbytes] = 0        # one past
        with pytest.raises(AssertionError, match=r"workspace 0 \(\d+ bytes, poison 0x7F\).*\+0 \.\. \+0 from its end"):
            handed.assert_guards("one past")
    assert L.workspace is real
    with pytest.raises(AssertionError, match="no workspace was asked for"):
        G.Handed().assert_guards("empty")
