"""The front end's merged launches against what they replace, bit for bit:

* dflow_daisy_pair (both images of a pair in one set of 7 launches) against two dflow_daisy calls;
* the kNN stage with both images prepared by one knn_prep_kernel launch and the exact fallback (knn_fix_kernel) run by teams
  of 4 waves, against the brute-force kernel (DFLOW_FLAG_KNN_EXACT): no fallback item, and a few lists;
* DiscreteFlow.run against a run whose descriptors come from two single-image calls.

There is no case for the whole-pass path of knn_fix_kernel (flags & 1): only a basis that fails its orthogonality check sets
the flag, and knn_cov_kernel replaces non-finite and absurd samples (|v| >= 1e4) by zero before they reach the basis, so no
descriptor values drive a pass there at any size; that path shares the item loop with the per-list path below and differs
only in how an item is decoded.

Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

OUTPUTS = ("proposals", "lcosts", "nprop", "bestlabels")
# (H, W, cellh, cellw): ragged 7 x 6 cells of 63 points (a 64-query wave that is not full; last column 16 wide, last row 10
# high: cells of 112, 90 and 160 points) and 2 x 2 cells of 1728 points, the bench's cell size (27 query waves, 62 chunks of the
# fix kernel's LDS streaming per cell)
GEOMS = [(45, 70, 7, 9), (54, 128, 27, 64)]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def make(H, W, ch, cw, f16=False, seed=0):
    L = pkg("_lib")
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed, flags=L.FLAG_DESCR_F16 if f16 else 0)


def bits(t):
    """A descriptor plane as integers: float32 -> int32, binary16 -> int16 (NaN-proof, sign-of-zero-proof equality)."""
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------- DAISY
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", [(40, 56), (97, 131)])
def test_daisy_pair_equals_two_single_calls(torch_, synth, shape, f16):
    """97 x 131 is no multiple of the 32 x 8 / 32 x 16 tiles nor of the 4-wide stores.  The two images differ, so a scratch
    plane shared between them, or outputs swapped, would show; the planes are poisoned with different values first, so an
    element the pair call does not write would show too (binary16 rows: their 4 pads must be written as zeros)."""
    torch = torch_
    L = pkg("_lib")
    H, W = shape
    img1, img2, _ = synth.make_pair(H, W, seed=H + W, amp_x=5, amp_y=3)
    assert not np.array_equal(img1, img2)
    df = make(H, W, max(5, H // 8), max(5, W // 8), f16)
    a, b = torch.from_numpy(img1).to(df.device), torch.from_numpy(img2).to(df.device)
    want1, want2 = df.izracunajDaisy(a).clone(), df.izracunajDaisy(b).clone()
    assert not torch.equal(bits(want1), bits(want2))
    df.ws.fill_(0x7F)
    df.descrs1.fill_(7.0); df.descrs2.fill_(-7.0)
    df.load_pair(a, b)
    assert torch.equal(bits(df.descrs1), bits(want1)), "image 1"
    assert torch.equal(bits(df.descrs2), bits(want2)), "image 2"
    # host images go through two staging buffers
    df.descrs1.fill_(7.0); df.descrs2.fill_(-7.0)
    df.load_pair(img1, img2)
    assert torch.equal(bits(df.descrs1), bits(want1)) and torch.equal(bits(df.descrs2), bits(want2))
    # the same image twice: two identical planes
    df.descrs1.fill_(7.0); df.descrs2.fill_(-7.0)
    df.load_pair(a, a)
    assert torch.equal(bits(df.descrs1), bits(want1)) and torch.equal(bits(df.descrs2), bits(want1))
    # the single call still needs only its own part of the workspace, the pair call twice that, and refuses one output plane
    lib, n = L.lib(), H * W * 16
    one = lambda nbytes: lib.dflow_daisy(C.byref(df.p), a.data_ptr(), df.descrs1.data_ptr(), df.ws.data_ptr(), nbytes, L.stream(df.device))
    two = lambda nbytes, o2: lib.dflow_daisy_pair(C.byref(df.p), a.data_ptr(), b.data_ptr(), df.descrs1.data_ptr(), o2, df.ws.data_ptr(),
                                                  nbytes, L.stream(df.device))
    assert one(6 * n + 1024) == 0 and one(6 * n - 1) == -2
    assert two(12 * n + 2048, df.descrs2.data_ptr()) == 0 and two(12 * n - 1, df.descrs2.data_ptr()) == -2
    assert two(df.ws_bytes, df.descrs1.data_ptr()) == -1 and b"same plane" in lib.dflow_last_error()
    assert two(df.ws_bytes, None) == -1 and b"NULL" in lib.dflow_last_error()
    torch.cuda.synchronize()
    assert df.ws_bytes >= 12 * n


# ------------------------------------------------------------------------------------------------------------------ kNN
def knn_both(df, d1, d2):
    """generisi on (d1, d2), screened and brute force, outputs and workspace poisoned before each: the screened pass's statistics
    after asserting that the two agree bit for bit."""
    L = pkg("_lib")
    keep = df.p.flags & ~L.FLAG_KNN_EXACT
    out = []
    for mode in (0, L.FLAG_KNN_EXACT):
        df.p.flags = keep | mode
        df.set_descriptors(d1, d2)
        df.ws.fill_(1)
        df.proposals.fill_(0x7FFF7FFF); df.lcosts.fill_(float("nan")); df.nprop.fill_(-1); df.bestlabels.fill_(-1)
        df.generisi()
        if mode == 0:
            stats = df.knn_stats()
        out.append([bits(t).clone() if t.dtype.is_floating_point else t.clone() for t in (df.proposals, df.lcosts, df.nprop, df.bestlabels)])
    df.p.flags = keep
    for a, b, name in zip(out[0], out[1], OUTPUTS):
        assert bool((a == b).all()), (name, stats)
    return stats


@pytest.fixture(scope="module")
def knn_case(torch_, synth):
    """(pass, descriptors of image 1, of image 2) per (geometry, storage): real DAISY of a synthetic pair, computed once."""
    cache = {}

    def get(geom, f16):
        if (geom, f16) not in cache:
            H, W, ch, cw = geom
            img1, img2, _ = synth.make_pair(H, W, seed=H * W, amp_x=0.1 * W, amp_y=0.1 * H)
            df = make(H, W, ch, cw, f16)
            df.load_pair(img1, img2)
            cache[(geom, f16)] = (df, df.descriptors_f32(0).clone(), df.descriptors_f32(1).clone())
        return cache[(geom, f16)]
    return get


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("geom", GEOMS)
def test_knn_plain_pair_has_no_fix_item(knn_case, geom, f16):
    """(a) both images through the one prep launch; the fix launch finds nothing to do."""
    df, d1, d2 = knn_case(geom, f16)
    stats = knn_both(df, d1, d2)
    assert stats["lists_exact"] == 0 and stats["flags"] == 0 and stats["bad_queries"] == 0, stats


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("geom", GEOMS)
def test_knn_few_lists_through_the_fix_kernel(knn_case, geom, f16):
    """(b) rows outside the screen's range (a value the f16 rows cannot hold; binary16 planes hold it) send the lists they take
    part in to knn_fix_kernel one by one: a query in the first cell (63 points at 45 x 70: the 64-query wave is not full; the
    last wave of a 1728-point cell at 54 x 128), a query in the last, largest cell, and a candidate in the last cell row (the
    larger cells at 45 x 70), whose lists come from every query wave with that cell in its window."""
    df, d1, d2 = knn_case(geom, f16)
    H, W, ch, cw = geom
    q, c = d1.clone(), d2.clone()
    q[ch - 1, cw - 1, 7] = 2000.0               # the last point of cell (0, 0)
    q[H - 1, W - 1, 60] = 3000.0                # the last point of the last cell
    c[H - 2, W // 2, 11] = 2500.0               # a candidate in the last cell row
    stats = knn_both(df, q, c)
    assert stats["flags"] == 0 and stats["bad_queries"] == 2, stats
    assert 0 < stats["lists_exact"] < stats["lists"], stats


# ------------------------------------------------------------------------------------------------------------- pipeline
def test_run_equals_run_on_descriptors_of_single_calls(torch_, synth):
    torch = torch_
    H, W, ch, cw = 54, 128, 27, 64
    img1, img2, _ = synth.make_pair(H, W, seed=11, amp_x=9, amp_y=4)
    df = make(H, W, ch, cw, seed=3)
    flow = df.run(img1, img2, 2).clone()
    labels = df.bestlabels.clone()
    ref = make(H, W, ch, cw, seed=3)
    ref.izracunajDaisy(img1, out=ref.descrs1)
    ref.izracunajDaisy(img2, out=ref.descrs2)
    assert torch.equal(bits(ref.descrs1), bits(df.descrs1)) and torch.equal(bits(ref.descrs2), bits(df.descrs2))
    ref.generisi(); ref.nasumicni(); ref.ceoBCD(2)
    assert torch.equal(ref.vratiKonacniFlow(), flow) and torch.equal(ref.bestlabels, labels)
    assert float(flow.abs().max()) > 0
