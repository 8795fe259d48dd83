"""Every refusal of the C-ABI's host-side gates (csrc/abi.hip), pinned: the status, the exact text of dflow_last_error() and the
order of the checks, against tests/golden/abi_refusals.json.

One table per entry point: the arguments' names, a base call, and the faults in the order the source checks them.  Every base
call is itself refused: where there is a workspace its size is 0 bytes, elsewhere the entry point's last check fails (a NULL or
an alias).  A row replaces some arguments of the base call by a fault of its own: no call here passes every check, so nothing is
launched on the stand-in pointers, and run_tables asserts the refusal of each call before it makes the next.
Every row is run alone ("id") and, unless it is SOLO, together with every later row that is not SOLO ("id+"): faults i..n
together must answer exactly what fault i answers alone, which fixes the order.  CPU only.

python tests/test_abi_refusals.py writes the golden file from the library that is built."""
import ctypes as C
import json
import os
import re
import threading

import pytest

from conftest import ROOT, pkg

GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
PLANE = 1 << 32                                     # more than any plane of an 8192 x 8192 frame
A, B, D, E, F, G, H, I, J, K = (PLANE * k for k in range(1, 11))   # non-NULL, 4 GiB-aligned, disjoint stand-ins for device pointers
WS = PLANE * 16
BIG = 1 << 40                                       # a ws_bytes above every need
GEOM = (40, 48, 5, 6)                               # the screened kNN search runs for it: dflow_knn_proposals checks a workspace
HH, WW = 37, 101
NAN = float("nan")
SOLO = "solo"                                       # a row that is left out of the "id+" calls and has none of its own
KNN_EXACT, WMED_REJECT = 1, 2


def null(name):
    return (name + "_null", {name: None})


def mis(name, by):
    """`name` moved `by` bytes off its base value"""
    return ("%s_plus%d" % (name, by), {name: ("+", by)})


def same(name, other, **more):
    """`name` given the base value of `other`"""
    return ("%s_is_%s" % (name, other), dict({name: ("=", other)}, **more))


P_ROWS = [("p_null", {"p": None}), ("p_flags", {"p.flags": 64})]          # flags are dflow_check_params' last check
# the message names both sizes: one of the four goes into the "id+" calls
SIZE_ROWS = [("h_0", {"h": 0}), ("w_0", {"w": 0}, SOLO), ("h_8193", {"h": 8193}, SOLO), ("w_8193", {"w": 8193}, SOLO)]


def ws_base(align, **kw):
    """The base call of an entry point that checks d_ws last (CHECK_WS): a workspace that is short AND misaligned, so that every
    "id+" call carries both faults behind its own."""
    return dict(kw, d_ws=WS + align // 2, ws_bytes=0, stream=None)


def af_base(**kw):
    """The same for the entry points that name d_ws among their aligned pointers, in the middle of their checks: short only."""
    return dict(kw, d_ws=WS, ws_bytes=0, stream=None)


# CHECK_WS: a NULL or short workspace first, then its alignment (the last row's fault is ws_base's misaligned d_ws)
WS_ROWS = [("ws_null", {"d_ws": None, "ws_bytes": BIG}, SOLO), ("ws_short", {"d_ws": WS}, SOLO), ("ws_short_and_misaligned", {"ws_bytes": 0}),
           ("ws_misaligned", {"ws_bytes": BIG}, SOLO)]
KNN_PTRS = "d_descr1 d_descr2 d_proposals d_lcosts d_nprop d_bestlabels"
# the data planes' boundaries (include/dflow.h, "Alignment of data planes"), after the NULL checks and before the workspace
KNN_MIS = [mis("d_descr1", 8), mis("d_descr2", 4), mis("d_proposals", 8), mis("d_lcosts", 4), mis("d_nprop", 2), mis("d_bestlabels", 1)]
BCD_MIS = [mis("d_proposals", 8), mis("d_nprop", 2), mis("d_bestlabels", 2)]
KNN_BASE = ws_base(16, p=GEOM, d_descr1=A, d_descr2=B, d_proposals=D, d_lcosts=E, d_nprop=F, d_bestlabels=G)
BCD_BASE = ws_base(16, p=GEOM, d_proposals=A, d_nprop=B, d_bestlabels=D, phase=0)
BATCH_BASE = dict(p=GEOM, npass=2, d_nprop=[A, B], d_bestlabels=[D, E], phase=0, d_ws=[WS, WS + 4096], ws_bytes=0, stream=None)
BATCH_HEAD = P_ROWS + [null("d_nprop"), null("d_bestlabels"), null("d_ws"), ("npass_0", {"npass": 0}), ("npass_1025", {"npass": 1025})]
# the size comes before the per-pass pointers
BATCH_TAIL = [("ws_short", {"ws_bytes": 0}), ("ws_short_by_one", {"ws_bytes": 255}, SOLO),
              ("pass_0_bestlabels_null", {"d_bestlabels": [None, E], "ws_bytes": BIG}), ("pass_1_nprop_null", {"d_nprop": [A, None], "ws_bytes": BIG}),
              ("pass_1_ws_null", {"d_ws": [WS, None], "ws_bytes": BIG}),
              # a pass's planes are checked pass by pass, d_nprop[i] before d_bestlabels[i]
              ("pass_0_nprop_plus2", {"d_nprop": [A + 2, B], "ws_bytes": BIG}), ("pass_1_bestlabels_plus1", {"d_bestlabels": [D, E + 1], "ws_bytes": BIG}),
              ("pass_1_ws_plus8", {"d_ws": [WS, WS + 4096 + 8], "ws_bytes": BIG}),
              ("pass_0_ws_plus1", {"d_ws": [WS + 1, WS + 4096], "ws_bytes": BIG}, SOLO)]
STATS_P_ROWS = [("p_null", {"p": None}), ("p_pich_0", {"p.pich": 0}), ("p_picw_8193", {"p.picw": 8193}, SOLO), ("p_label_pitch_8", {"p.label_pitch": 8}),
                ("p_label_pitch_24", {"p.label_pitch": 24}), ("p_maxnprop_0", {"p.maxnprop": 0}), ("p_tpsi_9", {"p.tpsi": 9}),
                ("p_tphi_nan", {"p.tphi": NAN}, SOLO), ("p_tphi_negative", {"p.tphi": -1.0})]
# dflow_bcd_stats(_batch) name d_ws among their aligned pointers: its alignment comes before its size
STATS_TAIL = [mis("d_stats", 4), mis("d_ws", 4), ("ws_null", {"d_ws": None, "ws_bytes": BIG}, SOLO), ("ws_short", {"ws_bytes": 0})]
VAR = ws_base(4, h=HH, w=WW, d_bgr1=A, d_bgr2=B, d_flow_in=D, p="var", d_flow_out=E)

# name -> (argument names, base call, rows in the order of the checks)
TABLES = {
    # dflow_check_params, field by field, through the size function (as test_abi.py does): 0 and a message
    "dflow_workspace_bytes": ("p", {"p": GEOM, "p.max_attempts": 1}, [
        ("p_null", {"p": None}), ("pich_4", {"p.pich": 4}), ("picw_8193", {"p.picw": 8193}, SOLO), ("cellh_0", {"p.cellh": 0, "p.cellw": 2}),
        ("cellw_49", {"p.cellw": 49}, SOLO), ("knn_4", {"p.knn": 4}), ("cell_2x2", {"p.cellh": 2, "p.cellw": 2}),
        ("window_3", {"p.window": 3}), ("ngauss_65", {"p.ngauss": 65}), ("maxnprop_200", {"p.maxnprop": 200}),
        ("maxnprop_100", {"p.maxnprop": 100}, SOLO), ("label_pitch_150", {"p.label_pitch": 150}), ("label_pitch_176", {"p.label_pitch": 176}, SOLO),
        ("tpsi_0", {"p.tpsi": 0}), ("tpsi_9", {"p.tpsi": 9}, SOLO), ("lamda_nan", {"p.lamda": NAN}), ("lamda_negative", {"p.lamda": -1.0}, SOLO),
        ("tphi_inf", {"p.tphi": float("inf")}), ("tphi_negative", {"p.tphi": -0.5}, SOLO), ("dp_sentinel", {"p.lamda": 1e6}),
        ("sigma_0", {"p.sigma": 0.0}), ("sigma_9", {"p.sigma": 9.0}, SOLO), ("max_attempts_1", {"p.max_attempts": 1}),
        ("flags_64", {"p.flags": 64, "p.max_attempts": 1 << 16}, SOLO), ("flags_2", {"p.flags": 2, "p.max_attempts": 1 << 16}, SOLO)]),
    "dflow_daisy": ("p d_bgr d_descr d_ws ws_bytes stream", ws_base(16, p=GEOM, d_bgr=A, d_descr=B),
                    P_ROWS + [null("d_bgr"), null("d_descr"), mis("d_descr", 8)] + WS_ROWS),
    "dflow_daisy_pair": ("p d_bgr1 d_bgr2 d_descr1 d_descr2 d_ws ws_bytes stream", ws_base(16, p=GEOM, d_bgr1=A, d_bgr2=B, d_descr1=D, d_descr2=E),
                         P_ROWS + [null("d_bgr1"), null("d_bgr2"), null("d_descr1"), null("d_descr2"), mis("d_descr1", 4), mis("d_descr2", 8)] + WS_ROWS
                         + [same("d_descr2", "d_descr1", d_ws=WS, ws_bytes=BIG) + (SOLO,)]),
    # never with DFLOW_FLAG_KNN_EXACT: the brute-force search takes no workspace and would run
    "dflow_knn_proposals": ("p " + KNN_PTRS + " d_ws ws_bytes stream", KNN_BASE, P_ROWS + [null(n) for n in KNN_PTRS.split()] + KNN_MIS + WS_ROWS),
    "dflow_knn_proposals_timed": ("p " + KNN_PTRS + " d_ws ws_bytes stream h_ms h_mfma_issued", dict(KNN_BASE, h_ms="ms", h_mfma_issued=None),
                                  P_ROWS + [null(n) for n in KNN_PTRS.split()] + [null("h_ms")] + KNN_MIS + [("knn_exact", {"p.flags": KNN_EXACT})] + WS_ROWS),
    "dflow_knn_screen_stats": ("p d_ws ws_bytes stream h_stats", ws_base(16, p=GEOM, h_stats="stats"),
                               P_ROWS + [null("h_stats"), ("knn_exact", {"p.flags": KNN_EXACT})] + WS_ROWS),
    "dflow_knn_screen_stats_n": ("p d_ws ws_bytes stream h_stats n_stats", ws_base(16, p=GEOM, h_stats="stats", n_stats=14),
                                 P_ROWS + [null("h_stats"), ("n_stats_0", {"n_stats": 0}), ("n_stats_15", {"n_stats": 15}),
                                           ("knn_exact", {"p.flags": KNN_EXACT})] + WS_ROWS),
    "dflow_neighbour_proposals": ("p " + KNN_PTRS + " d_ws ws_bytes stream", KNN_BASE, P_ROWS + [null(n) for n in KNN_PTRS.split()] + KNN_MIS + WS_ROWS),
    "dflow_bcd_prepare": ("p d_proposals d_lcosts d_nprop d_ws ws_bytes stream", ws_base(16, p=GEOM, d_proposals=A, d_lcosts=B, d_nprop=D),
                          P_ROWS + [null("d_proposals"), null("d_lcosts"), null("d_nprop"), mis("d_proposals", 4), mis("d_lcosts", 8), mis("d_nprop", 1)] + WS_ROWS),
    "dflow_bcd_phase": ("p d_proposals d_nprop d_bestlabels phase d_ws ws_bytes stream", BCD_BASE,
                        P_ROWS + [null("d_proposals"), null("d_nprop"), null("d_bestlabels"), ("phase_negative", {"phase": -1}), ("phase_4", {"phase": 4})]
                        + BCD_MIS + WS_ROWS),
    "dflow_bcd_sweep": ("p d_proposals d_nprop d_bestlabels d_ws ws_bytes stream", BCD_BASE,
                        P_ROWS + [null("d_proposals"), null("d_nprop"), null("d_bestlabels")] + BCD_MIS + WS_ROWS),
    "dflow_bcd_phase_batch": ("p npass d_nprop d_bestlabels phase d_ws ws_bytes stream", BATCH_BASE,
                              BATCH_HEAD + [("phase_negative", {"phase": -1}), ("phase_4", {"phase": 4})] + BATCH_TAIL),
    "dflow_bcd_sweep_batch": ("p npass d_nprop d_bestlabels d_ws ws_bytes stream", BATCH_BASE, BATCH_HEAD + BATCH_TAIL),
    # bcd_stats_check_params, field by field
    "dflow_bcd_stats_workspace_bytes": ("p", {"p": GEOM, "p.tphi": -1.0}, STATS_P_ROWS),
    "dflow_bcd_stats": ("p d_proposals d_lcosts d_nprop d_bestlabels d_prev_labels d_prev_out d_stats d_ws ws_bytes stream",
                        af_base(p=GEOM, d_proposals=A, d_lcosts=B, d_nprop=D, d_bestlabels=E, d_prev_labels=None, d_prev_out=None, d_stats=F),
                        [("p_null", {"p": None}), ("p_tphi_nan", {"p.tphi": NAN})]
                        + [null(n) for n in "d_proposals d_lcosts d_nprop d_bestlabels d_stats".split()]
                        + [mis("d_proposals", 8), mis("d_lcosts", 8), mis("d_nprop", 2), mis("d_bestlabels", 2), ("d_prev_labels_plus2", {"d_prev_labels": G + 2}),
                           ("d_prev_out_plus1", {"d_prev_out": H + 1})] + STATS_TAIL),
    "dflow_bcd_stats_batch": ("p npass d_proposals d_lcosts d_nprop d_bestlabels d_prev d_stats d_ws ws_bytes stream",
                              af_base(p=GEOM, npass=2, d_proposals=[A, A], d_lcosts=[B, B], d_nprop=[D, D], d_bestlabels=[E, E], d_prev=None,
                                   d_stats=F),
                              [("p_null", {"p": None}), ("p_tphi_nan", {"p.tphi": NAN}), ("npass_0", {"npass": 0}), ("npass_1025", {"npass": 1025})]
                              + [null(n) for n in "d_proposals d_lcosts d_nprop d_bestlabels d_stats".split()]
                              + [("pass_0_proposals_null", {"d_proposals": [None, A]}), ("pass_1_bestlabels_null", {"d_bestlabels": [E, None]})]
                              # pass by pass, in the order of the arguments; a NULL d_prev[i] passes
                              + [("pass_0_proposals_plus8", {"d_proposals": [A + 8, A]}), ("pass_0_lcosts_plus4", {"d_lcosts": [B + 4, B]}),
                                 ("pass_0_nprop_plus2", {"d_nprop": [D + 2, D]}), ("pass_0_bestlabels_plus2", {"d_bestlabels": [E + 2, E]}),
                                 ("pass_1_prev_plus2", {"d_prev": [None, G + 2]})]
                              + STATS_TAIL),
    # no workspace: in the base call the last plane that is checked is off its boundary (d_packed moves byte by byte)
    "dflow_labels_to_flow": ("p d_proposals d_bestlabels d_flow stream", dict(p=GEOM, d_proposals=A, d_bestlabels=B, d_flow=D + 4, stream=None),
                             P_ROWS + [null("d_proposals"), null("d_bestlabels"), null("d_flow"), mis("d_proposals", 8), mis("d_bestlabels", 2),
                                       ("d_flow_plus4", {})]),
    "dflow_fb_consistency": ("p d_fwd d_bwd tresh d_sparse stream", dict(p=GEOM, d_fwd=A, d_bwd=B, tresh=1.0, d_sparse=D + 2, stream=None),
                             P_ROWS + [null("d_fwd"), null("d_bwd"), null("d_sparse"), mis("d_fwd", 4), mis("d_bwd", 4), ("d_sparse_plus2", {})]),
    "dflow_pack_compat": ("p d_proposals d_nprop d_packed stream", dict(p=GEOM, d_proposals=A, d_nprop=B + 2, d_packed=D, stream=None),
                          P_ROWS + [null("d_proposals"), null("d_nprop"), null("d_packed"), mis("d_proposals", 8), ("d_nprop_plus2", {})]),
    # runs on the host, on h_sparse: the base call has no columns
    "dflow_remove_small_segments_host": ("h_sparse dim0 dim1 tresh min_segment_size", dict(h_sparse=A, dim0=4, dim1=0, tresh=1.0, min_segment_size=3),
                                         [null("h_sparse"), ("dim0_0", {"dim0": 0}), ("dim0_negative", {"dim0": -1}, SOLO), ("dim1_0", {"dim1": 0})]),
    "dflow_canny_edges": ("h w d_bgr low high d_edges d_ivice d_ws ws_bytes stream", ws_base(4, h=HH, w=WW, d_bgr=A, low=100.0, high=200.0, d_edges=B, d_ivice=None),
                          SIZE_ROWS + [("low_nan", {"low": NAN}), ("high_negative", {"high": -1.0}, SOLO), ("high_inf", {"high": float("inf")}, SOLO),
                                       null("d_bgr"), null("d_edges"), ("d_ivice_plus2", {"d_ivice": D + 2})] + WS_ROWS),
    "dflow_pb_edges": ("h w d_bgr radius d_strength d_orient_strength d_ws ws_bytes stream",
                       ws_base(2, h=HH, w=WW, d_bgr=A, radius=5, d_strength=B, d_orient_strength=None),
                       SIZE_ROWS + [("radius_0", {"radius": 0}), ("radius_8", {"radius": 8}), null("d_bgr"), null("d_strength"), mis("d_strength", 2),
                                    ("d_orient_strength_plus2", {"d_orient_strength": D + 2})] + WS_ROWS),
    "dflow_epic_interpolate": ("h w d_sparse d_edges nn k method d_flow d_seed_of d_dist d_lists d_list_g d_ws ws_bytes stream",
                               ws_base(8, h=HH, w=WW, d_sparse=A, d_edges=B, nn=16, k=0.8, method=0, d_flow=D, d_seed_of=None, d_dist=None,
                                    d_lists=None, d_list_g=None),
                               SIZE_ROWS + [("nn_0", {"nn": 0}), ("nn_257", {"nn": 257}), ("k_0", {"k": 0.0}), ("k_inf", {"k": float("inf")}, SOLO),
                                            ("method_2", {"method": 2}), null("d_sparse"), null("d_edges"), null("d_flow"), mis("d_sparse", 2), mis("d_edges", 1), mis("d_flow", 2),
                                            ("d_seed_of_plus2", {"d_seed_of": E + 2}), ("d_dist_plus2", {"d_dist": F + 2}),
                                            ("d_lists_plus1", {"d_lists": G + 1}), ("d_list_g_plus4", {"d_list_g": H + 4})] + WS_ROWS),
    "dflow_epic_prefilter": ("h w d_bgr d_sparse_in d_edges saliency_th pref_nn pref_th k d_sparse_out d_reason d_saliency d_estimate d_ws ws_bytes stream",
                             ws_base(8, h=HH, w=WW, d_bgr=A, d_sparse_in=B, d_edges=D, saliency_th=0.045, pref_nn=25, pref_th=5.0, k=0.8, d_sparse_out=E,
                                  d_reason=None, d_saliency=None, d_estimate=None),
                             SIZE_ROWS + [("saliency_th_negative", {"saliency_th": -1.0}), ("pref_nn_negative", {"pref_nn": -1}),
                                          ("pref_nn_256", {"pref_nn": 256}), ("pref_th_nan", {"pref_th": NAN}), ("k_negative", {"k": -0.5}),
                                          null("d_bgr"), null("d_sparse_in"), null("d_edges"), null("d_sparse_out"), mis("d_sparse_in", 2), mis("d_edges", 2),
                                          mis("d_sparse_out", 1), ("d_saliency_plus2", {"d_saliency": F + 2}),
                                          ("d_estimate_plus2", {"d_estimate": G + 2})] + WS_ROWS),
    "dflow_var_refine": ("h w d_bgr1 d_bgr2 d_flow_in p d_flow_out d_ws ws_bytes stream", VAR,
                         SIZE_ROWS + [null("p"), null("d_bgr1"), null("d_bgr2"), null("d_flow_in"), null("d_flow_out"),
                                      ("alpha_negative", {"p.alpha": -1.0}), ("gamma_nan", {"p.gamma": NAN}), ("delta_inf", {"p.delta": float("inf")}),
                                      ("sigma_6", {"p.sigma": 6.0}), ("sigma_nan", {"p.sigma": NAN}, SOLO), ("sor_omega_2", {"p.sor_omega": 2.0}),
                                      ("sor_omega_nan", {"p.sor_omega": NAN}, SOLO), ("niter_outer_negative", {"p.niter_outer": -1}),
                                      ("niter_inner_0", {"p.niter_inner": 0}), ("niter_solver_10001", {"p.niter_solver": 10001}), ("flags_2", {"p.flags": 2}),
                                      mis("d_flow_in", 4), mis("d_flow_out", 4)]
                         + WS_ROWS),
    "dflow_flow_eval": ("h w d_test test_layout d_gt abs_thresh flags d_stats d_err d_err_bgr d_ws ws_bytes stream",
                        ws_base(8, h=HH, w=WW, d_test=A, test_layout=0, d_gt=B, abs_thresh=3.0, flags=0, d_stats=D, d_err=E, d_err_bgr=F),
                        SIZE_ROWS + [("test_layout_2", {"test_layout": 2}), ("abs_thresh_negative", {"abs_thresh": -1.0}), ("flags_2", {"flags": 2}),
                                     null("d_test"), null("d_gt"), null("d_stats"), mis("d_test", 8), mis("d_gt", 4), mis("d_stats", 4), mis("d_err", 8),
                                     mis("d_err_bgr", 2)] + WS_ROWS),
    "dflow_flow_color": ("h w d_flow layout max_flow d_bgr d_maxrad d_ws ws_bytes stream",
                         ws_base(4, h=HH, w=WW, d_flow=A, layout=0, max_flow=0.0, d_bgr=B, d_maxrad=D),
                         SIZE_ROWS + [("layout_negative", {"layout": -1}), ("max_flow_negative", {"max_flow": -1.0}), null("d_flow"), null("d_bgr"),
                                      mis("d_flow", 8), mis("d_bgr", 1), mis("d_maxrad", 2)] + WS_ROWS),
    "dflow_warp_eval": ("h w d_bgr1 d_bgr2 d_flow layout err_thresh err_max flags d_stats d_warped d_err d_err_bgr d_ws ws_bytes stream",
                        ws_base(8, h=HH, w=WW, d_bgr1=A, d_bgr2=B, d_flow=D, layout=1, err_thresh=10.0, err_max=30.0, flags=0, d_stats=E, d_warped=F,
                             d_err=G, d_err_bgr=H),
                        SIZE_ROWS + [("layout_2", {"layout": 2}), ("err_thresh_nan", {"err_thresh": NAN}), ("err_max_0", {"err_max": 0.0}),
                                     ("err_max_inf", {"err_max": float("inf")}, SOLO), ("flags_2", {"flags": 2}), null("d_bgr1"), null("d_bgr2"),
                                     null("d_flow"), null("d_stats"), mis("d_bgr1", 2), mis("d_flow", 4), mis("d_stats", 4), mis("d_warped", 1),
                                     mis("d_err", 8), mis("d_err_bgr", 2)] + WS_ROWS),
    # no workspace: in the base call d_counts is the prior, the last of the state pointers that are compared with it
    "dflow_prior_proposals": ("p d_descr1 d_descr2 d_prior layout stride flags d_proposals d_lcosts d_nprop d_bestlabels d_counts stream",
                              dict(p=GEOM, d_descr1=A, d_descr2=B, d_prior=D, layout=0, stride=1, flags=0, d_proposals=E, d_lcosts=F, d_nprop=G,
                                   d_bestlabels=H, d_counts=D, stream=None),
                              P_ROWS + [("layout_2", {"layout": 2}), ("stride_negative", {"stride": -1}), ("stride_8193", {"stride": 8193}),
                                        ("flags_2", {"flags": 2})]
                              + [null(n) for n in "d_descr1 d_descr2 d_prior d_proposals d_lcosts d_nprop d_bestlabels".split()]
                              + [mis("d_descr1", 8), mis("d_descr2", 4), mis("d_prior", 2), mis("d_proposals", 8), mis("d_lcosts", 2), mis("d_nprop", 1),
                                 mis("d_bestlabels", 2), ("d_counts_plus2", {"d_counts": I + 2}),
                                 same("d_descr1", "d_prior"), same("d_lcosts", "d_prior"), same("d_counts", "d_prior")]),
    # d_ws is among the aligned pointers: its alignment comes before its size
    "dflow_flow_advance": ("h w d_flow layout flags d_out d_counts d_ws ws_bytes stream",
                           af_base(h=HH, w=WW, d_flow=A, layout=0, flags=0, d_out=B, d_counts=D),
                           SIZE_ROWS + [("layout_2", {"layout": 2}), ("flags_2", {"flags": 2}), null("d_flow"), null("d_out"), mis("d_flow", 2),
                                        mis("d_out", 1), mis("d_counts", 2), mis("d_ws", 2), same("d_out", "d_flow"),
                                        ("ws_null", {"d_ws": None, "ws_bytes": BIG}, SOLO), ("ws_short", {"ws_bytes": 0})]),
    # no workspace: in the base call the two outputs are one plane, the last check
    "dflow_pyr_down": ("h w d_in1 d_in2 d_out1 d_out2 stream", dict(h=HH, w=WW, d_in1=A, d_in2=B, d_out1=D, d_out2=D, stream=None),
                       SIZE_ROWS + [null("d_in1"), null("d_out1"), ("d_in2_null_alone", {"d_in2": None}), ("d_out2_null_alone", {"d_out2": None}, SOLO),
                                    mis("d_in1", 2), mis("d_in2", 1), mis("d_out1", 2), ("d_out2_plus2", {"d_out2": E + 2}),
                                    same("d_out1", "d_in1"), same("d_out2", "d_in1", d_out1=E) + (SOLO,), same("d_out1", "d_in2"),
                                    same("d_out2", "d_out1")]),
    # no workspace: in the base call d_counts is d_out, the last check
    "dflow_flow_upsample": ("h w d_coarse layout d_out d_counts stream", dict(h=HH, w=WW, d_coarse=A, layout=0, d_out=B, d_counts=B, stream=None),
                            SIZE_ROWS + [("layout_2", {"layout": 2}), null("d_coarse"), null("d_out"), mis("d_coarse", 2), mis("d_out", 2),
                                         ("d_counts_plus1", {"d_counts": D + 1}), same("d_out", "d_coarse"), same("d_counts", "d_coarse"),
                                         same("d_counts", "d_out")]),
    # no workspace: in the base call d_counts is d_err_bwd, the last pair of outputs that is compared
    "dflow_flow_consistency": ("h w d_fwd layout_fwd d_bwd layout_bwd thresh flags d_out_fwd d_out_bwd d_err_fwd d_err_bwd d_counts stream",
                               dict(h=HH, w=WW, d_fwd=A, layout_fwd=0, d_bwd=B, layout_bwd=1, thresh=1.0, flags=0, d_out_fwd=D, d_out_bwd=E, d_err_fwd=F,
                                    d_err_bwd=G, d_counts=G, stream=None),
                               SIZE_ROWS + [("layout_fwd_2", {"layout_fwd": 2}), ("layout_bwd_negative", {"layout_bwd": -1}), ("flags_2", {"flags": 2}),
                                            ("thresh_nan", {"thresh": NAN}), null("d_fwd"), null("d_bwd"), null("d_out_fwd"),
                                            ("d_err_bwd_without_d_out_bwd", {"d_out_bwd": None}), mis("d_fwd", 2), mis("d_bwd", 1), mis("d_out_fwd", 2),
                                            mis("d_out_bwd", 2), mis("d_err_fwd", 1), mis("d_err_bwd", 2), ("d_counts_plus2", {"d_counts": H + 2}),
                                            same("d_out_fwd", "d_bwd"), same("d_err_fwd", "d_fwd"), same("d_out_bwd", "d_out_fwd") + (SOLO,),
                                            same("d_counts", "d_err_bwd")]),
    # d_ws is among the aligned pointers, and among the planes that must not overlap: both come before its size
    "dflow_segment_filter": ("h w d_flow layout thresh min_size flags d_out d_segment d_size d_counts d_ws ws_bytes stream",
                             af_base(h=HH, w=WW, d_flow=A, layout=0, thresh=1.0, min_size=20, flags=0, d_out=B, d_segment=D, d_size=E, d_counts=F),
                             SIZE_ROWS + [("layout_2", {"layout": 2}), ("flags_2", {"flags": 2}), ("thresh_negative", {"thresh": -1.0}),
                                          ("min_size_negative", {"min_size": -1}), null("d_flow"), null("d_out"), mis("d_flow", 2), mis("d_out", 2),
                                          mis("d_segment", 1), mis("d_size", 2), mis("d_counts", 2), mis("d_ws", 2),
                                          same("d_out", "d_flow", layout=1), ("d_segment_in_d_flow", {"d_segment": A + 4 * HH * WW}),
                                          ("d_size_in_d_segment", {"d_size": D + 4 * HH * WW - 4}), ("d_ws_at_d_counts", {"d_ws": F + 12}),
                                          ("ws_null", {"d_ws": None, "ws_bytes": BIG}, SOLO), ("ws_short", {"ws_bytes": 0})]),
    # no workspace: in the base call d_counts is d_source, the last pair of outputs that is compared
    "dflow_frame_interp": ("h w d_bgr1 d_bgr2 d_fwd layout_fwd d_bwd layout_bwd t fill_rounds occl_thresh flags d_out d_keys d_motion d_motion_tmp "
                           "d_source d_counts stream",
                           dict(h=HH, w=WW, d_bgr1=A, d_bgr2=B, d_fwd=D, layout_fwd=0, d_bwd=E, layout_bwd=1, t=0.5, fill_rounds=2, occl_thresh=1.0, flags=0,
                                d_out=F, d_keys=G, d_motion=H, d_motion_tmp=I, d_source=J, d_counts=J, stream=None),
                           SIZE_ROWS + [("layout_fwd_2", {"layout_fwd": 2}), ("layout_bwd_2", {"layout_bwd": 2}), ("t_0", {"t": 0.0}), ("t_1", {"t": 1.0}, SOLO),
                                        ("t_nan", {"t": NAN}, SOLO), ("fill_rounds_negative", {"fill_rounds": -1}), ("fill_rounds_65", {"fill_rounds": 65}),
                                        ("occl_thresh_negative", {"occl_thresh": -1.0}), ("flags_1", {"flags": 1})]
                           + [null(n) for n in "d_bgr1 d_bgr2 d_fwd d_out d_keys d_motion d_motion_tmp".split()]
                           + [mis("d_keys", 4), mis("d_fwd", 2), mis("d_bwd", 2), mis("d_motion", 1), mis("d_motion_tmp", 2),
                              ("d_counts_plus2", {"d_counts": K + 2}), same("d_out", "d_bgr2"), same("d_keys", "d_out"), same("d_motion", "d_bwd"),
                              same("d_motion_tmp", "d_motion"), same("d_source", "d_bgr1"), same("d_counts", "d_fwd"), same("d_counts", "d_source")]),
    # no workspace: in the base call d_counts is d_out, the last check
    "dflow_flow_wmedian": ("h w d_flow layout d_bgr radius d_wspace d_wcolor reject_thresh flags d_out d_counts stream",
                           dict(h=HH, w=WW, d_flow=A, layout=0, d_bgr=B, radius=2, d_wspace=D, d_wcolor=E, reject_thresh=1.0, flags=0, d_out=F, d_counts=F,
                                stream=None),
                           SIZE_ROWS + [("layout_2", {"layout": 2}), ("radius_0", {"radius": 0}), ("radius_9", {"radius": 9}), ("flags_4", {"flags": 4}),
                                        ("reject_thresh_nan", {"reject_thresh": NAN, "flags": WMED_REJECT}), null("d_flow"), null("d_out"),
                                        ("d_bgr_null_alone", {"d_bgr": None}), ("d_wcolor_null_alone", {"d_wcolor": None}, SOLO), mis("d_flow", 2),
                                        mis("d_out", 1), ("d_counts_plus2", {"d_counts": G + 2}), same("d_out", "d_flow"), same("d_out", "d_wcolor"),
                                        same("d_counts", "d_wspace"), same("d_counts", "d_out")]),
    # the timings of the last call on this thread: none has run on the thread these tables are called from
    "dflow_epic_last_stats": ("rounds stage_ms", dict(rounds=None, stage_ms="ms"), [("nothing_ran", {})]),
    "dflow_epic_prefilter_last_stats": ("counts stage_ms", dict(counts=None, stage_ms="ms"), [("nothing_ran", {})]),
}
# the eleven size functions of an (h, w) frame: 0 and a message
SIZE_FUNCTIONS = ("dflow_canny_workspace_bytes", "dflow_pb_workspace_bytes", "dflow_epic_workspace_bytes", "dflow_epic_prefilter_workspace_bytes",
                  "dflow_var_workspace_bytes", "dflow_eval_workspace_bytes", "dflow_flow_color_workspace_bytes", "dflow_warp_eval_workspace_bytes",
                  "dflow_flow_advance_workspace_bytes", "dflow_segment_filter_workspace_bytes")
for _name in SIZE_FUNCTIONS:
    TABLES[_name] = ("h w", {"h": HH, "w": 8193}, [("h_0", {"h": 0}, SOLO), ("w_0", {"w": 0}, SOLO), ("h_8193", {"h": 8193}, SOLO), ("w_8193", {"w": 8193})])
RETURNS_A_SIZE = SIZE_FUNCTIONS + ("dflow_workspace_bytes", "dflow_bcd_stats_workspace_bytes")
NO_STATUS = ("dflow_version", "dflow_last_error", "dflow_default_params", "dflow_var_default_params")     # nothing to refuse


def resolve(base, over):
    """A row's arguments with ("+", n) and ("=", other) worked out against the base call."""
    return {k: (base[k] + v[1] if v[0] == "+" else base[v[1]]) if isinstance(v, tuple) else v for k, v in over.items()}


def cases(name):
    """(case id, arguments by name) of one table: every row alone, and every row that is not SOLO with the later ones."""
    _, base, rows = TABLES[name]

    def put(values, over):
        values.update(resolve(base, over))
    rows = [(r[0], r[1], len(r) > 2) for r in rows]
    assert len({r[0] for r in rows}) == len(rows), name
    out = []
    for i, (rid, over, solo) in enumerate(rows):
        values = dict(base)
        put(values, over)
        out.append((rid, values))
        later = [r for r in rows[i + 1:] if not r[2]]
        if not solo and later:
            values = dict(base)
            for _, o, _ in reversed(later):
                put(values, o)
            put(values, over)                            # last: where two faults are values of one argument, this row's stays
            out.append((rid + "+", values))
    return out


def marshal(L, names, values):
    """The ctypes arguments of one call (and what must outlive it)."""
    lib = L.lib()
    args = []
    for n in names.split():
        v = values[n]
        fields = {k[2:]: x for k, x in values.items() if k.startswith("p.")}
        if n == "p" and v == "var":
            s = L.VarParams()
            lib.dflow_var_default_params(C.byref(s))
            for k, x in fields.items():
                assert hasattr(s, k)
                setattr(s, k, x)
            v = C.byref(s)
        elif n == "p" and v is not None:
            s = L.default_params(*v)
            for k, x in fields.items():
                assert hasattr(s, k)
                setattr(s, k, x)
            v = C.byref(s)
        elif isinstance(v, list):
            v = (C.c_void_p * len(v))(*v)
        elif v == "ms":
            v = (C.c_float * 8)()
        elif v == "stats":
            v = (C.c_int64 * 16)()
        args.append(v)
    return args


def run_tables(L):
    """{function: {case id: [rc, message]}}.  Each call is checked to have been refused before the next one is made.  On a thread
    of its own: the last error and the 'last call' state of the *_last_stats functions belong to the calling thread."""
    lib = L.lib()
    got, failed = {}, []

    def run():
        try:
            for name, (names, _, _) in TABLES.items():
                fn = getattr(lib, name)
                got[name] = {}
                for cid, values in cases(name):
                    rc = fn(*marshal(L, names, values))
                    msg = lib.dflow_last_error().decode()
                    assert (rc == 0) if name in RETURNS_A_SIZE else (rc != 0), "%s/%s was not refused (%d, %r)" % (name, cid, rc, msg)
                    got[name][cid] = [rc, msg]
        except BaseException as e:                       # noqa: B902  (re-raised on the calling thread)
            failed.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failed:
        raise failed[0]
    return got


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


@pytest.fixture(scope="module")
def answers(L):
    return run_tables(L)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_function_that_returns_a_status_has_a_table(L):
    assert set(TABLES) | set(NO_STATUS) == set(L._SIGNATURES)
    for name in TABLES:
        restype, argtypes = L._SIGNATURES[name]
        assert len(TABLES[name][0].split()) == len(argtypes), name
        assert (restype is C.c_size_t) == (name in RETURNS_A_SIZE), name


def test_every_base_call_carries_the_last_fault(L):
    """What the docstring says of the base calls, read off the tables: with a workspace its size is 0 and one row is that call;
    without one the last row that is not SOLO is the base call."""
    for name, (names, base, rows) in TABLES.items():
        is_base = [dict(base, **resolve(base, r[1])) == base for r in rows if len(r) == 2]
        if "ws_bytes" in base:
            assert base["ws_bytes"] == 0 and any(is_base), name
        else:
            assert is_base[-1], name


@pytest.mark.parametrize("name", sorted(TABLES))
def test_refusals_are_the_golden_ones(answers, golden, name):
    assert answers[name] == golden[name]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_several_faults_answer_the_first(answers, name):
    """Faults i..n together answer what fault i answers alone: the checks run in the order of the table."""
    for cid, answer in answers[name].items():
        if cid.endswith("+"):
            assert answer == answers[name][cid[:-1]], (name, cid)


def test_the_golden_file_holds_these_cases_and_no_others(golden):
    assert {n: [c for c, _ in cases(n)] for n in TABLES} == {n: list(v) for n, v in golden.items()}


def message_shapes(source):
    """The format strings of the dflow_set_error sites of a source text (CHECK_PTR's and CHECK_WS's among them), as regular
    expressions over whole messages."""
    shapes = []
    for m in re.finditer(r'dflow_set_error\(\s*\w+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', source):
        fmt = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
        rx = re.escape(fmt)
        for spec, sub in (("%.17g", r"\S+"), ("%zu", r"\d+"), ("%s", ".+?"), ("%d", r"-?\d+"), ("%g", r"\S+"), ("%x", "[0-9a-f]+")):
            rx = rx.replace(re.escape(spec), sub)
        shapes.append((fmt, re.compile("^" + rx + "$")))
    return shapes


# the sites that need a HIP call to fail: dflow_check_launch (and DFLOW_HIP in dflow_knn_proposals_timed, no dflow_set_error by name)
NOT_PROVOKED = ("%s: %s",)


def test_every_refusal_site_of_abi_hip_is_answered(golden):
    """Every dflow_set_error site of csrc/abi.hip has a case above whose message it wrote."""
    source = open(os.path.join(ROOT, pkg().__name__, "csrc", "abi.hip")).read()
    messages = {msg for v in golden.values() for _, msg in v.values()}
    shapes = message_shapes(source)
    assert len(shapes) > 40
    unanswered = [fmt for fmt, rx in shapes if fmt not in NOT_PROVOKED and not any(rx.match(m) for m in messages)]
    assert not unanswered, unanswered


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join('"%s": {\n%s\n}' % (name, ",\n".join(" %s: %s" % (json.dumps(c), json.dumps(a)) for c, a in got.items()))
                                         for name, got in run_tables(pkg("_lib")).items()))     # one case per line
    print("wrote", GOLDEN)
