"""The C-ABI library loads without a GPU and exports every symbol include/dflow.h declares; parameter validation and
error reporting work on the host.  No compute calls here (CPU only)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_exports_every_declared_symbol(L):
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    declared = sorted(set(re.findall(r"\b(dflow_[a-z_]+)\s*\(", header)))
    assert "dflow_daisy" in declared and "dflow_bcd_prepare" in declared and len(declared) >= 12
    handle = C.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), "libdflow.so does not export %s" % name
    assert set(L.SYMBOLS) == set(declared), "python binding and header disagree"


def test_version_and_struct_layout(L):
    assert L.lib().dflow_version() == 1
    assert C.sizeof(L.Params) == 72                       # struct dflow_params
    p = L.default_params(375, 1241, 25, 73)               # reference constants, daisy i flann.py:34-48,88,172,207-208
    assert (p.pich, p.picw, p.cellh, p.cellw) == (375, 1241, 25, 73)
    assert (p.maxnprop, p.knn, p.window, p.ngauss, p.tpsi) == (150, 5, 2, 25, 8)
    assert abs(p.tphi - 2.5) < 1e-7 and abs(p.sigma - 8.0) < 1e-7 and p.lamda == 0.05 and p.label_pitch == 160
    assert p.flags == 0 and L.FLAG_KNN_EXACT == 1          # per-call switches live in the params, not in the environment
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert "getenv" not in open(os.path.join(ROOT, pkg().__name__, "csrc", "abi.hip")).read()
    assert re.search(r"#define\s+DFLOW_FLAG_KNN_EXACT\s+1\b", header)


def test_workspace_size_and_validation(L):
    lib = L.lib()
    p = L.default_params(436, 1024, 27, 64)
    ws = lib.dflow_workspace_bytes(C.byref(p))
    assert ws > 436 * 1024 * 2 * 160 * 20                 # at least the BCD bit matrices
    for field, bad, msg in (("knn", 4, b"knn"), ("window", 3, b"window"), ("maxnprop", 200, b"maxnprop"),
                            ("label_pitch", 150, b"label_pitch"), ("cellh", 0, b"cell"), ("pich", 4, b"image size"),
                            ("tpsi", 0, b"tpsi"), ("ngauss", 100, b"ngauss"), ("flags", 64, b"flags"), ("flags", 2, b"flags")):
        q = L.default_params(436, 1024, 27, 64)
        setattr(q, field, bad)
        assert lib.dflow_workspace_bytes(C.byref(q)) == 0
        assert msg in lib.dflow_last_error(), (field, lib.dflow_last_error())


def test_null_pointers_are_rejected_before_any_launch(L):
    lib = L.lib()
    p = L.default_params(64, 64, 8, 8)
    rc = lib.dflow_daisy(C.byref(p), None, None, None, 0, None)
    assert rc == -1 and b"NULL" in lib.dflow_last_error()
    P = 1 << 20                                         # a stand-in plane on every boundary include/dflow.h asks for
    rc = lib.dflow_bcd_phase(C.byref(p), P, P, P, 7, 1, 1 << 40, None)
    assert rc == -1 and b"phase" in lib.dflow_last_error()
    rc = lib.dflow_bcd_sweep(C.byref(p), P, P, P, 1, 16, None)
    assert rc == -2 and b"workspace" in lib.dflow_last_error()


def test_batched_entry_points_validate_on_the_host(L):
    """dflow_bcd_*_batch take host arrays of device pointers: count, phase, NULL entries and the workspace size are
    checked before anything is launched."""
    lib = L.lib()
    p = L.default_params(64, 64, 8, 8)
    ws = lib.dflow_workspace_bytes(C.byref(p))
    arr = (C.c_void_p * 2)(1, 1)
    bad = (C.c_void_p * 2)(1, None)
    assert lib.dflow_bcd_phase_batch(C.byref(p), 0, arr, arr, 0, arr, ws, None) == -1 and b"npass" in lib.dflow_last_error()
    assert lib.dflow_bcd_phase_batch(C.byref(p), 2, arr, arr, 4, arr, ws, None) == -1 and b"phase" in lib.dflow_last_error()
    assert lib.dflow_bcd_phase_batch(C.byref(p), 2, arr, bad, 0, arr, ws, None) == -1 and b"NULL" in lib.dflow_last_error()
    assert lib.dflow_bcd_sweep_batch(C.byref(p), 2, arr, arr, arr, 16, None) == -2 and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_bcd_phase_batch(C.byref(p), 2, None, arr, 0, arr, ws, None) == -1


def test_knn_measurement_aids_validate_before_touching_the_gpu(L):
    """dflow_knn_screen_stats / dflow_knn_proposals_timed describe the MFMA-screened search: with DFLOW_FLAG_KNN_EXACT, a null
    output or a workspace that is too small they fail on the host."""
    lib = L.lib()
    p = L.default_params(64, 64, 8, 8)
    out = (C.c_int64 * 13)()
    assert lib.dflow_knn_screen_stats(C.byref(p), 1, 16, None, out) == -2 and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_knn_screen_stats(C.byref(p), 1, 1 << 40, None, None) == -1 and b"NULL" in lib.dflow_last_error()
    q = L.default_params(64, 64, 8, 8, flags=L.FLAG_KNN_EXACT)
    assert lib.dflow_knn_screen_stats(C.byref(q), 1, 1 << 40, None, out) == -1 and b"MFMA" in lib.dflow_last_error()
    # the header's count of statistics is what the host mirror names
    import re
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    n = int(re.search(r"#define\s+DFLOW_KNN_STATS_N\s+(\d+)", header).group(1))
    assert n == 13 and n == len(pkg("pipeline").DiscreteFlow.KNN_STATS)
    # the workspace holds the event lists: one entry per tile of the largest cell + 1 per lane (no list can run out)
    big = L.default_params(436, 1024, 27, 64)
    tiles = -(-(31 * 64) // 192) * 6                        # the last cell row is 31 px high; cells are padded to 192 rows
    nl = 16 * 16 * 31 * 25
    assert lib.dflow_workspace_bytes(C.byref(big)) > nl * 2 * (tiles + 1) * 256


def test_knn_stats_with_a_count_validate_before_touching_the_gpu(L):
    """dflow_knn_screen_stats_n writes the first n_stats statistics of DFLOW_KNN_STATS_ALL_N (the 13 of dflow_knn_screen_stats
    and those added since): a count outside 1..DFLOW_KNN_STATS_ALL_N, a null output, DFLOW_FLAG_KNN_EXACT or a workspace that is
    too small fail on the host; the host mirror names every statistic, the first DFLOW_KNN_STATS_N in the old order."""
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    n = int(re.search(r"#define\s+DFLOW_KNN_STATS_N\s+(\d+)", header).group(1))
    n_all = int(re.search(r"#define\s+DFLOW_KNN_STATS_ALL_N\s+(\d+)", header).group(1))
    DF = pkg("pipeline").DiscreteFlow
    assert n_all == 14 and n_all == len(DF.KNN_STATS_ALL) and DF.KNN_STATS_ALL[:n] == DF.KNN_STATS
    assert DF.KNN_STATS_ALL[n:] == ("heavy_pairs_left",)
    p = L.default_params(64, 64, 8, 8)
    out = (C.c_int64 * (n_all + 1))()
    for bad in (0, -1, n_all + 1):
        assert lib.dflow_knn_screen_stats_n(C.byref(p), 1, 1 << 40, None, out, bad) == -1 and b"n_stats" in lib.dflow_last_error()
    assert lib.dflow_knn_screen_stats_n(C.byref(p), 1, 16, None, out, n_all) == -2 and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_knn_screen_stats_n(C.byref(p), 1, 1 << 40, None, None, n_all) == -1 and b"NULL" in lib.dflow_last_error()
    q = L.default_params(64, 64, 8, 8, flags=L.FLAG_KNN_EXACT)
    assert lib.dflow_knn_screen_stats_n(C.byref(q), 1, 1 << 40, None, out, n_all) == -1 and b"MFMA" in lib.dflow_last_error()


def test_no_cpu_fallback(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.DflowError):
        pkg("pipeline").DiscreteFlow(64, 64, 8, 8)


def test_wave_primitives_have_one_definition_each():
    # the DPP steps, reductions, scan, count and rank of the kNN, BCD and EPIC kernels are csrc/wave_ops.h's
    import wave_ops_pins
    wave_ops_pins.check(os.path.join(ROOT, pkg().__name__, "csrc"))


def test_lamda_and_tphi_contract(L):
    """lamda and tphi must be finite and >= 0, and max(pich, picw) (3 tpsi + lamda tphi) < 800000 (include/dflow.h,
    DFLOW_DP_SENTINEL): outside it the chain kernel's unsigned minimum over tpsi + dp stops ordering like the doubles, or the
    reference's 800000 sentinels bind.  Refused on the host, with the field named in the message."""
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "dflow.h")).read()
    assert re.search(r"#define\s+DFLOW_DP_SENTINEL\s+800000\.0\b", header)

    def refused(msg, geom=(436, 1024, 27, 64), **kw):
        q = L.default_params(*geom, **kw)
        return lib.dflow_workspace_bytes(C.byref(q)) == 0 and msg in lib.dflow_last_error()

    for field in ("lamda", "tphi"):
        for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
            assert refused(field.encode() + b"=", **{field: bad}), (field, bad, lib.dflow_last_error())
    for field, edge in (("lamda", 0.0), ("tphi", 0.0), ("lamda", -0.0), ("tphi", -0.0)):
        q = L.default_params(436, 1024, 27, 64, **{field: edge})
        assert lib.dflow_workspace_bytes(C.byref(q)) > 0, (field, edge, lib.dflow_last_error())
    # 8000 * (3*8 + 38 * 2) = 800000 exactly: refused; one double below lamda = 38, accepted.  tphi = 2 is float32-exact.
    assert refused(b"must be below", (8, 8000, 8, 64), lamda=38.0, tphi=2.0)
    assert refused(b"lamda", (8000, 8, 64, 8), lamda=38.0, tphi=2.0)       # max(pich, picw) either way
    under = L.default_params(8, 8000, 8, 64, lamda=float(np.nextafter(38.0, 0.0)), tphi=2.0)
    assert lib.dflow_workspace_bytes(C.byref(under)) > 0, lib.dflow_last_error()
    # the same in tphi (lamda = 2): 38 is the bound, the next float32 below it is accepted
    assert refused(b"tphi", (8, 8000, 8, 64), lamda=2.0, tphi=38.0)
    under = L.default_params(8, 8000, 8, 64, lamda=2.0, tphi=float(np.nextafter(np.float32(38.0), np.float32(0.0))))
    assert lib.dflow_workspace_bytes(C.byref(under)) > 0, lib.dflow_last_error()
    # and one pixel longer chains at the same lamda: refused
    assert refused(b"must be below", (8, 8001, 8, 64), lamda=float(np.nextafter(38.0, 0.0)), tphi=2.0)
    # the largest chains at the defaults: 8192 (24 + 0.05 * 2.5) = 197 632
    assert lib.dflow_workspace_bytes(C.byref(L.default_params(8192, 8192, 512, 512))) > 0


def test_set_host_state_refuses_costs_outside_zero_tphi():
    """DiscreteFlow.set_host_state refuses used-slot costs that are negative, not finite or above tphi before touching the
    device (unused slots may hold anything: the reference fills them with 1000.0).  Checked on an object without a device."""
    DF = pkg("pipeline").DiscreteFlow
    df = DF.__new__(DF)
    df.p = pkg("_lib").default_params(8, 8, 8, 8)
    H = W = 8
    L = df.p.maxnprop
    proposals = np.zeros((H, W, L, 2), np.int64)
    nprop = np.full((H, W), 3, np.int64)
    for bad in (-0.5, float("nan"), float("inf"), 2.5000002384185791):      # the float32 just above tphi = 2.5
        lcosts = np.full((H, W, L), 1000.0)
        lcosts[..., :3] = 1.0
        lcosts[3, 4, 2] = bad
        with pytest.raises(ValueError, match="tphi|float32"):
            df.set_host_state(proposals, lcosts, nprop, np.zeros((H, W), np.int64))
