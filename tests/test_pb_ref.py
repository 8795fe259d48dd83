"""The definition of dflow_pb_edges in numpy (pb_ref.py) against the properties it must have, the argument parsing of the two
CLIs that take the new edge kind, and every rejection of the C-ABI entry (they return before anything is launched).  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import pb_ref as R
from conftest import pkg


@pytest.fixture(scope="module")
def L():
    lib = pkg("_lib")
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib


@pytest.fixture(scope="module")
def two_region():
    img = R.two_region_frame()                               # 40x56, boundary between columns 27 and 28, default_rng(0)
    return img, R.pb_both(img, 5)


def test_channels_are_bytes():
    rng = np.random.default_rng(1)
    c = R.channels(rng.integers(0, 256, (64, 64, 3)).astype(np.uint8))
    assert c.min() >= 0 and c.max() <= 255
    ends = R.channels(np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [255, 255, 255], [0, 0, 0]]], np.uint8))
    assert ends[1].max() == 255 and ends[1].min() == 0 and ends[2].max() == 255 and ends[2].min() == 0
    grey = R.channels(np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2))
    assert np.array_equal(grey[0][0], np.arange(256)) and (grey[1] == 127).all() and (grey[2] == 127).all()


@pytest.mark.parametrize("radius", range(1, 8))
def test_both_sides_hold_the_same_number_of_offsets(radius):
    counts = R.side_counts(radius)
    assert len(counts) == 8
    for a, b in counts:
        assert a == b and a >= 1
    assert len(R.offsets(radius)) == len(set(R.offsets(radius))) and (0, 0) not in R.offsets(radius)


@pytest.mark.parametrize("radius", [1, 5, 7])
def test_constant_image_is_exactly_zero(radius):
    for v in ((0, 0, 0), (255, 255, 255), (17, 130, 240)):
        img = np.empty((9, 11, 3), np.uint8)
        img[:] = v
        for dtype in (np.float64, np.float32):
            e, m = R.pb(img, radius, dtype)
            assert e.shape == (9, 11) and m.shape == (9, 11, 8) and e.dtype == dtype
            assert not e.any() and not m.any()


def test_range_and_float32_against_float64(two_region):
    rng = np.random.default_rng(2)
    cases = [(two_region[0], 5, two_region[1])]
    for img, radius in ((rng.integers(0, 256, (23, 31, 3)).astype(np.uint8), 7), (R.boundary_frame(17, 19), 5),
                        (rng.integers(0, 256, (3, 3, 3)).astype(np.uint8), 5), (R.boundary_frame(1, 9), 2)):
        cases.append((img, radius, R.pb_both(img, radius)))
    for img, radius, ((e64, m64), (e32, m32)) in cases:
        for e, m in ((e64, m64), (e32, m32)):
            assert e.min() >= 0 and e.max() <= 1 and m.min() >= 0 and m.max() <= 1
            assert np.array_equal(e, m.max(axis=-1))
        assert e32.dtype == np.float32 and m32.dtype == np.float32
        assert np.abs(e32 - e64).max() <= 1e-5 and np.abs(m32 - m64).max() <= 1e-5
    assert cases[1][2][0][0].max() > 0.5          # random bytes: half-discs differ everywhere


def test_two_region_boundary_stands_out(two_region):
    _, ((e, _), _) = two_region
    boundary, interior = e[:, 27:29].mean(), e[:, 5:20].mean()
    print("boundary %.4f interior %.4f ratio %.2f" % (boundary, interior, boundary / interior))
    assert boundary >= 3 * interior


def test_spremi_za_epic_parses_pb_and_refuses_unknown_kinds(capsys):
    spz = pkg("spremiZaEpic")
    six = ["a.png", "b.png", "f.npy", "b.npy", "3"]
    for kind in ("canny", "sed", "pb"):
        assert spz.parse(six + [kind]) == (six + [kind], False, False, False)
    assert spz.parse(six + ["pb", "--gpu-epic", "--prefilter", "--refine"]) == (six + ["pb"], True, True, True)
    assert spz.parse(six + ["pb", "--gpu-epic"]) == (six + ["pb"], True, False, False)
    capsys.readouterr()
    for kind in ("pB", "soft", ""):
        assert spz.parse(six + [kind]) == 2 and spz.main(six + [kind]) == 2
        assert "edge kind must be 'canny' or 'sed'" in capsys.readouterr().err
    assert spz.parse(six + ["pb", "--refine"]) == 2


def test_run_batch_parses_edge_kind(capsys):
    ap = pkg("run_batch").parser()
    assert ap.parse_args([]).edge_kind == "canny"
    assert ap.parse_args(["--edges", "--edge-kind", "pb"]).edge_kind == "pb"
    assert ap.parse_args(["--edge-kind", "canny"]).edge_kind == "canny"
    for bad in ("sed", "soft"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--edge-kind", bad])
        assert e.value.code == 2
    capsys.readouterr()


def test_abi_rejections_happen_before_any_launch(L):
    lib = L.lib()
    EINVAL, ENOSPC = -1, -2
    P = 1 << 20                                         # a stand-in float plane on its 4-byte boundary
    for h, w in ((0, 8), (8, 0), (-1, 8), (8193, 8), (8, 8193)):
        assert lib.dflow_pb_workspace_bytes(h, w) == 0 and b"image size" in lib.dflow_last_error()
        assert lib.dflow_pb_edges(h, w, 1, 5, P, P, 1, 1 << 40, None) == EINVAL and b"image size" in lib.dflow_last_error()
    assert lib.dflow_pb_workspace_bytes(1, 1) > 0 and lib.dflow_pb_workspace_bytes(8192, 8192) >= 2 * 8192 * 8192
    wsb = lib.dflow_pb_workspace_bytes(40, 56)
    assert wsb >= 2 * 40 * 56
    for radius in (0, -1, 8, 100):
        assert lib.dflow_pb_edges(40, 56, 1, radius, P, P, 1, wsb, None) == EINVAL and b"radius" in lib.dflow_last_error()
    assert lib.dflow_pb_edges(40, 56, None, 5, P, P, 1, wsb, None) == EINVAL and b"d_bgr is NULL" in lib.dflow_last_error()
    assert lib.dflow_pb_edges(40, 56, 1, 5, None, P, 1, wsb, None) == EINVAL and b"d_strength is NULL" in lib.dflow_last_error()
    assert lib.dflow_pb_edges(40, 56, 1, 5, P, None, None, wsb, None) == ENOSPC and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_pb_edges(40, 56, 1, 5, P, None, 1, wsb - 1, None) == ENOSPC and b"workspace" in lib.dflow_last_error()
    assert lib.dflow_pb_edges(40, 56, 1, 5, P, P, 1, 0, None) == ENOSPC
