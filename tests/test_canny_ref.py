"""The numpy restatement of the Canny edge map (canny_ref.py) on cases that can be computed by hand, and the host-side
validation of dflow_canny_edges / dflow_canny_workspace_bytes (CPU only, no launch)."""
import ctypes as C
import os

import numpy as np
import pytest

import canny_ref as R
from conftest import pkg


def _gray_bgr(g):
    """(H,W) gray levels -> a BGR image with that gray (equal channels: the weights sum to 1 << 14)."""
    g = np.asarray(g, np.uint8)
    return np.repeat(g[..., None], 3, axis=2)


def test_step_edge_lies_in_the_dark_column_only():
    g = np.zeros((16, 16), np.uint8)
    g[:, 8:] = 255
    assert np.array_equal(R.gray(_gray_bgr(g)), g)
    b = R.blur(g)
    assert list(b[5, 6:10]) == [0, 64, 191, 255]
    dx, dy = R.sobel(b)
    m = np.abs(dx) + np.abs(dy)
    assert list(m[5, 6:10]) == [256, 764, 764, 256] and not dy.any()
    e = R.canny(_gray_bgr(g))
    assert e.dtype == np.uint8 and set(np.unique(e)) == {0, 255}
    assert np.array_equal(np.nonzero(e)[1], np.full(16, 7)) and len(np.nonzero(e)[0]) == 16


def test_gray_of_pure_primaries():
    bgr = np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert list(R.gray(bgr)[0]) == [76, 150, 29, 255, 0]


def test_blur_reflects_101_on_thin_images():
    row = np.array([[160, 0, 0, 0, 0]])
    assert list(R.blur(row)[0]) == [80, 40, 0, 0, 0]            # 1xN: the one row is its own reflection
    assert list(R.blur(row.T)[:, 0]) == [80, 40, 0, 0, 0]       # Nx1
    mid = np.array([[0, 0, 160, 0, 0]])
    assert list(R.blur(mid)[0]) == [0, 40, 80, 40, 0]
    g = np.zeros((3, 3), np.int64)
    g[1, 1] = 90
    assert R.blur(g).tolist() == [[23] * 3] * 3                # reflect-101 puts the centre on both outer taps
    g = np.zeros((3, 3), np.int64)
    g[0, 0] = 160
    assert R.blur(g).tolist() == [[40, 20, 0], [20, 10, 0], [0, 0, 0]]
    one = np.array([[200]])
    assert R.blur(one).tolist() == [[200]]


def test_plateau_ridge_keeps_its_left_or_top_pixel():
    row = np.array([0, 0, 0, 0, 100, 200, 300, 300, 300, 300])
    b = np.tile(row, (6, 1))
    dx, _ = R.sobel(b)
    assert list(dx[2, 3:7]) == [400, 800, 800, 400]
    cand, strong = R.classes(b, 100, 200)
    assert np.array_equal(np.nonzero(cand.any(axis=0))[0], [4]) and cand[:, 4].all() and strong[:, 4].all()
    cand_t, _ = R.classes(b.T, 100, 200)
    assert np.array_equal(cand_t, cand.T)


def test_weak_diagonal_chain_needs_a_strong_pixel():
    cand = np.zeros((8, 8), bool)
    for k in range(7):
        cand[k, k] = True                                   # 8-connected through corners only
    cand[0, 7] = True                                       # an unrelated weak pixel
    strong = np.zeros_like(cand)
    strong[6, 6] = True
    e = R.hysteresis(cand, strong)
    assert [bool(e[k, k]) for k in range(7)] == [True] * 7 and e[0, 7] == 0 and e.sum() == 7 * 255
    assert not R.hysteresis(cand, np.zeros_like(cand)).any()


def test_thresholds_swap_and_floor():
    assert R.thresholds(200, 100) == (100, 200) and R.thresholds(100.5, 200.9) == (100, 200)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    ref = R.canny(img, 100, 200)
    assert ref.any() and np.array_equal(R.canny(img, 200, 100), ref) and np.array_equal(R.canny(img, 100.5, 200.9), ref)
    assert not np.array_equal(R.canny(img, 10, 20), ref)


def test_ivice_is_zero_on_edges_and_one_elsewhere():
    e = np.array([[0, 255], [255, 0]], np.uint8)
    v = R.ivice(e)
    assert v.dtype == np.float32 and v.tolist() == [[1.0, 0.0], [0.0, 1.0]]


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


def test_canny_symbols_are_exported(L):
    handle = C.CDLL(L.LIB_PATH)
    for name in ("dflow_canny_workspace_bytes", "dflow_canny_edges"):
        assert hasattr(handle, name) and name in L.SYMBOLS


def test_canny_workspace_size_and_validation(L):
    lib = L.lib()
    assert lib.dflow_canny_workspace_bytes(1, 1) > 0
    n = 375 * 1242
    assert 6 * n <= lib.dflow_canny_workspace_bytes(375, 1242) <= 6 * n + 1024
    for h, w in ((0, 5), (5, 0), (-1, 5), (8193, 5), (5, 8193)):
        assert lib.dflow_canny_workspace_bytes(h, w) == 0
        assert b"image size" in lib.dflow_last_error()
    assert lib.dflow_canny_workspace_bytes(8192, 8192) > 0


def test_canny_edges_rejects_bad_calls_before_any_launch(L):
    lib = L.lib()
    ws = lib.dflow_canny_workspace_bytes(20, 30)
    assert lib.dflow_canny_edges(0, 30, 1, 100.0, 200.0, 1, None, 1, ws, None) == -1 and b"image size" in lib.dflow_last_error()
    assert lib.dflow_canny_edges(20, 30, None, 100.0, 200.0, 1, None, 1, ws, None) == -1 and b"NULL" in lib.dflow_last_error()
    assert lib.dflow_canny_edges(20, 30, 1, 100.0, 200.0, None, 1, 1, ws, None) == -1 and b"d_edges" in lib.dflow_last_error()
    assert lib.dflow_canny_edges(20, 30, 1, 100.0, 200.0, 1, None, 1, ws - 1, None) == -2 and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_canny_edges(20, 30, 1, 100.0, 200.0, 1, None, None, ws, None) == -2
    for lo, hi in ((float("nan"), 200.0), (100.0, float("inf")), (-1.0, 200.0)):
        assert lib.dflow_canny_edges(20, 30, 1, lo, hi, 1, None, 1, ws, None) == -1 and b"threshold" in lib.dflow_last_error()


def test_edge_module_explains_sed():
    edge = pkg("edge")
    with pytest.raises(NotImplementedError, match="model.yml"):
        edge.sed_ivice("a.png", "ivice.bin")
