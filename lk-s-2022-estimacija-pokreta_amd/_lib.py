"""ctypes binding of libdflow.so (include/dflow.h).  There is no CPU fallback: if the HIP library is missing
or a call fails, an exception is raised."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libdflow.so")

FLAG_KNN_EXACT = 1      # DFLOW_FLAG_KNN_EXACT
FLAG_DESCR_F16 = 8      # DFLOW_FLAG_DESCR_F16
DESC_PITCH_F16 = 72     # DFLOW_DESC_PITCH_F16: binary16 descriptor planes are (H,W,72)
VAR_FLAG_SOR_UNFUSED = 1    # DFLOW_VAR_FLAG_SOR_UNFUSED
EVAL_UVV, EVAL_DYDX = 0, 1  # DFLOW_EVAL_UVV, DFLOW_EVAL_DYDX: the test field's layout in dflow_flow_eval
EVAL_FLAG_ACCUMULATE = 1    # DFLOW_EVAL_FLAG_ACCUMULATE
WARP_FLAG_ACCUMULATE = 1    # DFLOW_WARP_FLAG_ACCUMULATE
PRIOR_SEED_LABELS = 1       # DFLOW_PRIOR_SEED_LABELS
ADVANCE_NEGATE = 1          # DFLOW_ADVANCE_NEGATE
FBC_BILINEAR = 1            # DFLOW_FBC_BILINEAR
SEG_KEEP_SINGLETONS = 1     # DFLOW_SEG_KEEP_SINGLETONS
WMED_KEEP_HOLES, WMED_REJECT = 1, 2     # DFLOW_WMED_KEEP_HOLES, DFLOW_WMED_REJECT
MOTION_AFFINE, MOTION_HOMOGRAPHY = 0, 1     # DFLOW_MOTION_AFFINE, DFLOW_MOTION_HOMOGRAPHY
CONF_LOCAL, CONF_DATA = 0, 1                # DFLOW_CONF_LOCAL, DFLOW_CONF_DATA
CONF_COUNTS = 6                             # DFLOW_CONF_COUNTS
# DFLOW_TRACK_FREE .. DFLOW_TRACK_INCONSISTENT: the states of a track
TRACK_FREE, TRACK_LIVE, TRACK_LEFT, TRACK_NOFLOW, TRACK_NOBACK, TRACK_INCONSISTENT = range(6)
TRACK_CAP_MAX = 1 << 26                     # a track set's largest capacity
EPIPOLAR_MAX_HYP = 21845                    # DFLOW_EPIPOLAR_MAX_HYP: three slots per sample in a 16-bit index
SEGMENTS_MAX = 1 << 26                      # DFLOW_SEGMENTS_MAX: the most segments, and the largest min_size


class DflowError(RuntimeError):
    pass


class Params(C.Structure):
    """struct dflow_params (include/dflow.h) = the module globals of daisy i flann.py:34-48,88,172,207-208."""
    _fields_ = [("pich", C.c_int32), ("picw", C.c_int32), ("cellh", C.c_int32), ("cellw", C.c_int32),
                ("maxnprop", C.c_int32), ("knn", C.c_int32), ("window", C.c_int32), ("ngauss", C.c_int32),
                ("tpsi", C.c_int32), ("max_attempts", C.c_int32), ("tphi", C.c_float), ("sigma", C.c_float),
                ("lamda", C.c_double), ("seed", C.c_uint64), ("label_pitch", C.c_int32), ("flags", C.c_int32)]


class VarParams(C.Structure):
    """struct dflow_var_params (include/dflow.h): the parameters of dflow_var_refine."""
    _fields_ = [("alpha", C.c_float), ("gamma", C.c_float), ("delta", C.c_float), ("sigma", C.c_float),
                ("sor_omega", C.c_float), ("niter_outer", C.c_int32), ("niter_inner", C.c_int32),
                ("niter_solver", C.c_int32), ("flags", C.c_uint32)]


class EvalStats(C.Structure):
    """struct dflow_eval_stats (include/dflow.h): what dflow_flow_eval leaves in device memory."""
    _fields_ = [("n", C.c_uint64), ("n_out_abs", C.c_uint64), ("n_out_kitti", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("n_gt_valid", C.c_uint64), ("n_test_valid", C.c_uint64), ("sum_err", C.c_double), ("max_err", C.c_float),
                ("reserved", C.c_uint32)]


class PhotoStats(C.Structure):
    """struct dflow_photo_stats (include/dflow.h): what dflow_warp_eval leaves in device memory."""
    _fields_ = [("n", C.c_uint64), ("n_outside", C.c_uint64), ("n_unknown", C.c_uint64), ("n_above", C.c_uint64),
                ("sum_err", C.c_double), ("max_err", C.c_float), ("reserved", C.c_uint32)]


class BcdStats(C.Structure):
    """struct dflow_bcd_stats (include/dflow.h): what dflow_bcd_stats leaves in device memory, 48 bytes."""
    _fields_ = [("smooth_sum", C.c_uint64), ("n_pairs_trunc", C.c_uint64), ("n_data_trunc", C.c_uint64), ("n_changed", C.c_uint64),
                ("n_bad_label", C.c_uint64), ("data_sum", C.c_double)]


_vp, _sz, _i32, _f32, _f64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_float, C.c_double
_pp = C.POINTER(Params)


class _u64(C.c_uint64):
    """A uint64_t argument that is no byte count (a seed).  ctypes' c_uint64 is c_size_t itself on LP64, and in this table a
    c_size_t is a ws_bytes: a type of its own keeps the two apart."""


# every C-ABI function: name -> (return type, argument types)
_SIGNATURES = {
    "dflow_version": (C.c_int, []),
    "dflow_last_error": (C.c_char_p, []),
    "dflow_default_params": (None, [_pp, _i32, _i32, _i32, _i32]),
    "dflow_workspace_bytes": (_sz, [_pp]),
    "dflow_daisy": (C.c_int, [_pp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_daisy_pair": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_knn_proposals": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_knn_proposals_timed": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(_f32), C.POINTER(_f64)]),
    "dflow_knn_screen_stats": (C.c_int, [_pp, _vp, _sz, _vp, C.POINTER(C.c_int64)]),
    "dflow_knn_screen_stats_n": (C.c_int, [_pp, _vp, _sz, _vp, C.POINTER(C.c_int64), _i32]),
    "dflow_neighbour_proposals": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_bcd_prepare": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_bcd_phase": (C.c_int, [_pp, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),
    "dflow_bcd_sweep": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_bcd_phase_batch": (C.c_int, [_pp, _i32, _vp, _vp, _i32, _vp, _sz, _vp]),
    "dflow_bcd_sweep_batch": (C.c_int, [_pp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "dflow_bcd_stats_workspace_bytes": (_sz, [_pp]),
    "dflow_bcd_stats": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_bcd_stats_batch": (C.c_int, [_pp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_labels_to_flow": (C.c_int, [_pp, _vp, _vp, _vp, _vp]),
    "dflow_fb_consistency": (C.c_int, [_pp, _vp, _vp, _f32, _vp, _vp]),
    "dflow_pack_compat": (C.c_int, [_pp, _vp, _vp, _vp, _vp]),
    "dflow_remove_small_segments_host": (C.c_int, [_vp, _i32, _i32, _f32, _i32]),
    "dflow_canny_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_canny_edges": (C.c_int, [_i32, _i32, _vp, _f64, _f64, _vp, _vp, _vp, _sz, _vp]),
    "dflow_pb_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_pb_edges": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "dflow_epic_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_epic_interpolate": (C.c_int, [_i32, _i32, _vp, _vp, _i32, _f64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_epic_last_stats": (C.c_int, [_vp, _vp]),
    "dflow_epic_prefilter_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_epic_prefilter": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _f64, _i32, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_epic_prefilter_last_stats": (C.c_int, [_vp, _vp]),
    "dflow_var_default_params": (None, [C.POINTER(VarParams)]),
    "dflow_var_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_var_refine": (C.c_int, [_i32, _i32, _vp, _vp, _vp, C.POINTER(VarParams), _vp, _vp, _sz, _vp]),
    "dflow_eval_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_flow_eval": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _f32, C.c_uint32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_flow_color_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_flow_color": (C.c_int, [_i32, _i32, _vp, _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "dflow_warp_eval_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_warp_eval": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _i32, _f32, _f32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_prior_proposals": (C.c_int, [_pp, _vp, _vp, _vp, _i32, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_flow_advance_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_flow_advance": (C.c_int, [_i32, _i32, _vp, _i32, C.c_uint32, _vp, _vp, _vp, _sz, _vp]),
    "dflow_pyr_down": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "dflow_flow_upsample": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "dflow_flow_consistency": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, _f32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_segment_filter_workspace_bytes": (_sz, [_i32, _i32]),
    "dflow_segment_filter": (C.c_int, [_i32, _i32, _vp, _i32, _f32, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dflow_frame_interp": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _f32, _i32, _f32, C.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp]),
    "dflow_flow_wmedian": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _f32, C.c_uint32, _vp, _vp, _vp]),
}
# Entry points whose gates are made of abi.hip's shared checks alone (no refusal text of their own): the tables of
# tests/test_abi_refusals.py cover _SIGNATURES, these have their refusals pinned by their own test files (tests/test_abi_motion.py,
# tests/test_abi_label_conf.py).
_SIGNATURES_SHARED_GATE = {
    "dflow_motion_fit": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, _f32, _i32, _i32, _i32, _i32, _u64, C.c_uint32, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_label_confidence": (C.c_int, [_pp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "dflow_flow_gate": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _f32, _f32, _vp, _vp, _vp]),
}
# The track calls (csrc/tracks.hip): shared checks alone as well, their refusals pinned by tests/test_abi_tracks.py.  A table of
# their own: the key sets of the two above are compared against fixed tables by the tests that cover them.
_SIGNATURES_TRACKS = {
    "dflow_track_advance": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _f32, _f32, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "dflow_track_seed": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_track_flow": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# The epipolar fit (csrc/epipolar.hip): shared checks alone, its refusals pinned by tests/test_abi_epipolar.py.
_SIGNATURES_EPIPOLAR = {
    "dflow_epipolar_fit": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _f32, _i32, _i32, _i32, _u64, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp]),
}
# Superpixels and the per-segment fit (csrc/superpixels.hip): shared checks alone, their refusals pinned by
# tests/test_abi_superpixels.py.
_SIGNATURES_SUPERPIXELS = {
    "dflow_superpixels": (C.c_int, [_i32, _i32, _vp, _i32, _i32, _i32, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_segment_fit": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, _f32, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# The two-view reconstruction (csrc/two_view.hip): shared checks alone, its refusals pinned by tests/test_abi_two_view.py.
_SIGNATURES_TWO_VIEW = {
    "dflow_two_view": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _f64, _f64, _f64, _f64, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp]),
}
# Sparse feature tracking (csrc/klt.hip, include/dflow_klt.h): shared checks alone, the refusals pinned by tests/test_abi_klt.py.
# Declared in a header of their own and kept out of SYMBOLS, which is what include/dflow.h declares.
_SIGNATURES_KLT = {
    "dflow_klt_pyramid_bytes": (_sz, [_i32, _i32, _i32]),
    "dflow_klt_pyramid": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp]),
    "dflow_corners": (C.c_int, [_i32, _i32, _vp, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dflow_klt_track": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _f32, _f32, _f32, _f32, C.c_uint32, _vp, _vp,
                                  _vp, _vp, _vp, _vp]),
}
SYMBOLS_KLT = tuple(_SIGNATURES_KLT)
TRACK_FLAT, TRACK_RESIDUAL = 6, 7             # DFLOW_TRACK_FLAT, DFLOW_TRACK_RESIDUAL: the states dflow_klt_track adds
KLT_LEVELS_MAX = 8
SYMBOLS = (tuple(_SIGNATURES) + tuple(_SIGNATURES_SHARED_GATE) + tuple(_SIGNATURES_TRACKS) + tuple(_SIGNATURES_EPIPOLAR)
           + tuple(_SIGNATURES_SUPERPIXELS) + tuple(_SIGNATURES_TWO_VIEW))


def build(force=False):
    """Compile libdflow.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "libdflow.so"])


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DflowError("%s is missing: run __graft_entry__.build() (there is no CPU fallback)" % LIB_PATH)
        # torch brings its own copy of the HIP runtime (same SONAME as /opt/rocm's).  If libdflow.so is loaded first it pulls in
        # the system copy, torch then loads its own, and whichever initialises second finds "no ROCm-capable device"
        # (python __graft_entry__.py smoke = build() then smoke() in one process did exactly that).  torch first: one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for table in (_SIGNATURES, _SIGNATURES_SHARED_GATE, _SIGNATURES_TRACKS, _SIGNATURES_EPIPOLAR, _SIGNATURES_SUPERPIXELS,
                      _SIGNATURES_TWO_VIEW, _SIGNATURES_KLT):
            for name, (restype, argtypes) in table.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise DflowError("%s failed (%d): %s" % (what, rc, lib().dflow_last_error().decode()))


def call(name, *args):
    """lib().name(*args); raises DflowError (with the name and dflow_last_error()) unless it returns 0."""
    check(getattr(lib(), name)(*args), name)


def stream(device):
    """The HIP stream handle torch uses on `device` now (every C-ABI call runs on it)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace(name, h, w, device):
    """A device buffer of lib().name(h, w) bytes (a *_workspace_bytes function of an (h, w) image) and its size; raises
    DflowError if the function refuses the size."""
    import torch
    nbytes = getattr(lib(), name)(h, w)
    if nbytes == 0:
        raise DflowError("%s: %s" % (name, lib().dflow_last_error().decode()))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def default_params(pich, picw, cellh, cellw, **kw):
    p = Params()
    lib().dflow_default_params(C.byref(p), pich, picw, cellh, cellw)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p
