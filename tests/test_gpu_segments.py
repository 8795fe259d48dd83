"""dflow_segment_filter on the device against its numpy definition (tests/segments_ref.py), bit for bit: the filtered field, the
segment ids, the sizes and the counts; and the layers above it: pipeline.segment_filter, spremiZaEpic.py --segments,
run_batch.py --segments and the calls they issue.  The kernels' tiles are 32 x 8 pixels: every size but 1x1 has more than one
tile, 45x35, 17x40 and 33x65 have ragged ones.  Everything here needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import segments_ref as R
from call_log import BATCH_FLOWS, record_calls
from conftest import pkg
from segments_ref import golden_fields, uvv

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 64), (64, 1), (45, 35), (17, 40), (33, 65), (96, 128)]
TW, TH = 32, 8                                            # SEG_TW, SEG_TH of csrc/segments.hip


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


# ---- contents
def blocks(h, w, pvalid, seed):
    """A random field as oracle/gen_golden_extras.py makes them: 4x4 blocks of one vector plus 0 or 1 per pixel and component."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    f = np.zeros((h, w, 3), np.float32)
    base = rng.integers(-3, 4, size=(h // 4 + 1, w // 4 + 1, 2)).astype(np.float32)
    f[..., :2] = np.kron(base, np.ones((4, 4, 1), np.float32))[:h, :w] + rng.integers(0, 2, size=(h, w, 2))
    f[..., 2] = rng.random((h, w)) < pvalid
    f[..., :2] *= f[..., 2:3]
    return f


def serpentine(h, w):
    """Even rows full, odd rows joined to them at alternating ends only: one segment that snakes through every row.  The rest of
    an odd row carries another vector: a segment of its own per odd row."""
    f = uvv(np.full((h, w), 2.0), np.full((h, w), -1.0))
    for y in range(1, h, 2):
        f[y, :, 0] = 50.0
        f[y, w - 1 if y % 4 == 1 else 0, 0] = 2.0
    return f


def spiral(h, w):
    """A one-pixel path that winds inwards from (0,0), one pixel of wall between its turns."""
    m = np.zeros((h, w), bool)
    y = x = d = 0
    m[0, 0] = True
    turned = 0
    while turned < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
            y, x, turned = ny, nx, 0
            m[y, x] = True
        else:
            d, turned = (d + 1) % 4, turned + 1
    return uvv(np.full((h, w), 1.0), np.full((h, w), 3.0), m)


def comb(h, w):
    """Teeth in the even columns that meet only in the last row."""
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    m[h - 1] = True
    return uvv(np.full((h, w), -2.0), np.full((h, w), 0.5), m)


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return uvv((yy + xx) % 2)


def halves(h, w, axis, at):
    """Two halves of one vector each, one pixel apart in U, that meet at row or column `at`."""
    U = np.zeros((h, w), np.float32)
    if axis == 0:
        U[at:] = 1
    else:
        U[:, at:] = 1
    return uvv(U)


def as_dydx(f):
    """The same members in the [dy,dx] layout: a pixel that is not valid gets a NaN, in either component by turns."""
    d = np.ascontiguousarray(f[..., 1::-1])
    bad = np.argwhere(~(f[..., 2] > 0.5))
    d[bad[:, 0], bad[:, 1], (bad[:, 0] + bad[:, 1]) % 2] = np.nan
    return d


_REF = {}


def reference(key, flow, thresh, min_size, flags=0):
    """tests/segments_ref.py on a field, computed once per (key, parameters); the results are shared and never written to."""
    k = (key, float(thresh), int(min_size), flags)
    if k not in _REF:
        _REF[k] = R.segment_filter(flow, thresh, min_size, flags)
    return _REF[k]


def device(flow, thresh, min_size, keep=False):
    out, seg, size, cnt = pkg("pipeline").segment_filter(flow, thresh, min_size, keep_singletons=keep, segments=True, sizes=True, counts=True)
    return out.cpu().numpy(), seg.cpu().numpy(), size.cpu().numpy(), cnt.cpu().tolist()


def same(got, want, what):
    assert got[3] == list(want[3]), (what, "counts", got[3], want[3])
    for g, w, name in zip(got[:3], want[:3], ("out", "segment", "size")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


# ---- against the reference
@pytest.mark.parametrize("name,field,thresh,min_size", golden_fields(), ids=[g[0].replace(" ", "-") for g in golden_fields()])
def test_golden_fields(torch_, name, field, thresh, min_size):
    for keep in (False, True):
        want = reference(name, field, thresh, min_size, int(keep))
        assert keep or 0 < want[3][1] < want[3][0]
        same(device(field, thresh, min_size, keep), want, name)
    same(device(as_dydx(field), thresh, min_size), reference(name, field, thresh, min_size), name + " dydx")


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("layout", ["uvv", "dydx"])
def test_random_block_fields(torch_, size, layout):
    h, w = size
    for k, pvalid in enumerate((0.6, 0.75, 0.9)):
        f = blocks(h, w, pvalid, 11 + k)
        thresh, min_size = (1.0, 2.0, 3.0)[k], (6, 12, 40)[k]
        for keep in (False, True):
            want = reference(("blocks", h, w, k), f, thresh, min_size, int(keep))
            same(device(f if layout == "uvv" else as_dydx(f), thresh, min_size, keep), want, (size, layout, pvalid, keep))
        if h * w > 1000:
            assert 0 < want[3][1] < want[3][0], "segments are both removed and kept"


def test_one_by_one(torch_):
    for valid, min_size, keep, want in ((1, 0, False, [1, 0, 1, 0]), (1, 5, False, [1, 1, 1, 1]), (1, 5, True, [1, 0, 1, 0]), (0, 5, False, [0, 0, 0, 0])):
        f = uvv([[3.0]], [[-4.0]], valid)
        got = device(f, 1.0, min_size, keep)
        same(got, R.segment_filter(f, 1.0, min_size, int(keep)), (valid, min_size, keep))
        assert got[3] == want


def test_serpentine(torch_):
    h, w = 33, 65
    f = serpentine(h, w)
    want = reference("serpentine", f, 1.0, 100)
    snake = 17 * w + 16
    assert want[1][0, 0] == 0 and want[2][0, 0] == snake and want[1][h - 1, w - 1] == 0, "one segment through every row"
    assert want[3] == [17, 16, h * w, 16 * (w - 1)]
    same(device(f, 1.0, 100), want, "serpentine")
    same(device(f, 1.0, snake), reference("serpentine", f, 1.0, snake), "size == min_size is kept")
    same(device(f, 1.0, snake + 1), reference("serpentine", f, 1.0, snake + 1), "everything removed")
    # upside down the snake's root is no longer the first pixel of the first tile
    g = np.ascontiguousarray(f[::-1, ::-1])
    same(device(g, 1.0, 100), reference("serpentine flipped", g, 1.0, 100), "serpentine flipped")


@pytest.mark.parametrize("size", [(45, 35), (33, 65), (96, 128)], ids=lambda s: "%dx%d" % s)
def test_spiral_and_comb(torch_, size):
    h, w = size
    f = spiral(h, w)
    want = reference(("spiral", size), f, 0.0, 2)
    assert want[3][0] == 1 and want[3][2] > h * w // 3, "the spiral is one segment"
    same(device(f, 0.0, 2), want, "spiral")
    g = np.ascontiguousarray(f[::-1, ::-1])                 # the root at the inner end
    same(device(g, 0.0, 2), reference(("spiral flipped", size), g, 0.0, 2), "spiral flipped")
    f = comb(h, w)
    want = reference(("comb", size), f, 0.0, 2)
    assert want[3][:2] == [1, 0] and want[2][0, 0] == (h - 1) * ((w + 1) // 2) + w
    same(device(f, 0.0, 2), want, "comb")
    f[h - 1, 1::2, 2] = 0                                   # without the last row's links: one segment per tooth
    want = reference(("teeth", size), f, 0.0, h + 1)
    assert want[3] == [(w + 1) // 2, (w + 1) // 2, h * ((w + 1) // 2), h * ((w + 1) // 2)]
    same(device(f, 0.0, h + 1), want, "teeth")


@pytest.mark.parametrize("size", SIZES[1:], ids=["%dx%d" % s for s in SIZES[1:]])
def test_checkerboard_is_all_singletons(torch_, size):
    h, w = size
    f = checkerboard(h, w)
    for min_size, keep, removed in ((2, False, h * w), (2, True, 0), (1, False, 0)):
        got = device(f, 0.0, min_size, keep)
        assert got[3] == [h * w, removed, h * w, removed]
        assert np.array_equal(got[1].ravel(), np.arange(h * w)) and (got[2] == 1).all()
        assert np.array_equal(got[0].view(np.uint32), (f if not removed else np.zeros_like(f)).view(np.uint32))
    # at thresh 1 the board is one segment
    assert device(f, 1.0, h * w)[3] == [1, 0, h * w, 0]


def test_one_segment_over_the_whole_frame(torch_):
    h, w = 96, 128
    f = uvv(np.full((h, w), 7.0), np.full((h, w), -7.0))
    n = h * w
    for min_size, removed in ((0, 0), (1, 0), (2, 0), (n, 0), (n + 1, 1), (2 ** 31 - 1, 1)):
        for keep in (False, True):
            out, seg, size, cnt = device(f, 0.0, min_size, keep)
            assert cnt == [1, removed, n, removed * n], (min_size, cnt)
            assert (seg == 0).all() and (size == n).all(), "the whole size is reached at one root"
            assert np.array_equal(out.view(np.uint32), (np.zeros_like(f) if removed else f).view(np.uint32))


def test_min_size_boundaries_on_a_random_field(torch_):
    f = blocks(45, 35, 0.8, 3)
    biggest = int(reference("bounds", f, 2.0, 0)[2].max())
    assert biggest > 2
    for min_size in (0, 1, 2, biggest, biggest + 1, 2 ** 31 - 1):
        for keep in (False, True):
            want = reference("bounds", f, 2.0, min_size, int(keep))
            same(device(f, 2.0, min_size, keep), want, (min_size, keep))
        kept = int(want[0][..., 2].sum())                   # with keep
        assert (min_size <= biggest) == (kept > int((want[2] == 1).sum())), "the largest segment stays exactly up to its size"


@pytest.mark.parametrize("case", ["column-45x35", "column-33x65", "row-17x40", "row-45x35"])
def test_halves_that_meet_on_a_tile_border(torch_, case):
    axis, (h, w) = (1 if case.startswith("column") else 0), (int(v) for v in case.split("-")[1].split("x"))
    for at in ((TW, TW - 1, TW + 1) if axis else (TH, TH - 1, 2 * TH)):
        f = halves(h, w, axis, at)
        first = at * (h if axis else w)
        apart = device(f, 0.5, first + 1)                   # two segments; the first has `first` pixels and goes
        same(apart, R.segment_filter(f, 0.5, first + 1), (case, at, "apart"))
        assert apart[3][:2] == [2, 1 if h * w - first > first else 2] and apart[1].max() == (at if axis else at * w)
        joined = device(f, 1.0, h * w)                      # one segment across the border
        same(joined, R.segment_filter(f, 1.0, h * w), (case, at, "joined"))
        assert joined[3] == [1, 0, h * w, 0]


def test_special_values(torch_):
    """NaN, Inf and valid = 0.5 are no members; a difference that overflows does not join; thresh is inclusive to the ulp."""
    f = blocks(17, 40, 0.9, 8)
    f[3, 5, 0], f[4, 6, 1], f[5, 7, 2], f[6, 8, 2] = np.nan, np.inf, 0.5, np.nan
    f[7, 31], f[7, 32] = (3e38, 0, 1), (-3e38, 0, 1)       # across a tile border
    f[9, 3], f[9, 4] = (3e38, 3e38, 1), (-3e38, -3e38, 1)
    t = np.float32(0.7)
    f[12, 30:34] = [(0, 0, 1), (t, 0, 1), (t, np.nextafter(t, np.float32(1)), 1), (t, 0, 1)]
    f[11, 30:34, 2] = f[13, 30:34, 2] = 0
    f[12, 29, 2] = f[12, 34, 2] = 0
    want = R.segment_filter(f, t, 2)
    assert want[1][12, 30:34].tolist() == [12 * 40 + 30, 12 * 40 + 30, 12 * 40 + 32, 12 * 40 + 33]
    assert want[1][3, 5] == want[1][4, 6] == want[1][5, 7] == want[1][6, 8] == -1 and want[1][7, 32] == 7 * 40 + 32
    same(device(f, t, 2), want, "special values")
    same(device(f, 3.4e38, 2), R.segment_filter(f, 3.4e38, 2), "a huge thresh")
    d = as_dydx(f)
    d[2, 2] = (np.inf, -np.inf)
    same(device(d, t, 2, True), R.segment_filter(d, t, 2, R.KEEP_SINGLETONS), "special values, dydx")


# ---- invariants
def raw_call(torch_, flow_t, thresh, min_size, flags, out_t):
    """dflow_segment_filter itself, so that d_out can be d_flow."""
    L = pkg("_lib")
    h, w, c = flow_t.shape
    ws, ws_bytes = L.workspace("dflow_segment_filter_workspace_bytes", h, w, flow_t.device)
    cnt = torch_.empty(4, dtype=torch_.int32, device=flow_t.device)
    L.call("dflow_segment_filter", h, w, flow_t.data_ptr(), L.EVAL_UVV if c == 3 else L.EVAL_DYDX, float(thresh), int(min_size), flags,
           out_t.data_ptr(), None, None, cnt.data_ptr(), ws.data_ptr(), ws_bytes, L.stream(flow_t.device))
    return cnt.cpu().tolist()


@pytest.mark.parametrize("size", [(45, 35), (33, 65), (96, 128)], ids=lambda s: "%dx%d" % s)
def test_invariants(torch_, size):
    h, w = size
    P = pkg("pipeline")
    f = blocks(h, w, 0.75, 21)
    want = reference(("invariants", size), f, 1.0, 8)
    first = device(f, 1.0, 8)
    same(first, want, "out of place")
    # two calls give identical bytes
    second = device(f, 1.0, 8)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], second[:3])) and first[3] == second[3]
    # in place (UVV) equals out of place
    t = torch_.from_numpy(f).cuda()
    cnt = raw_call(torch_, t, 1.0, 8, 0, t)
    assert cnt == first[3] and t.cpu().numpy().tobytes() == first[0].tobytes()
    # the filter applied to its own output changes nothing: removing segments joins no others
    again = device(first[0], 1.0, 8)
    assert again[0].tobytes() == first[0].tobytes() and again[3][1] == 0 and again[3][3] == 0
    assert again[3][0] == first[3][0] - first[3][1] and again[3][2] == first[3][2] - first[3][3]
    # on torch's current stream, from a device tensor, without the optional planes
    st = torch_.cuda.Stream()
    with torch_.cuda.stream(st):
        plain = P.segment_filter(torch_.from_numpy(f).cuda(), 1.0, 8)
    st.synchronize()
    assert isinstance(plain, torch_.Tensor) and tuple(plain.shape) == (h, w, 3) and plain.cpu().numpy().tobytes() == first[0].tobytes()
    r = P.segment_filter(f, 1.0, 8, sizes=True)
    assert len(r) == 2 and r[1].dtype == torch_.int32 and r[1].cpu().numpy().tobytes() == first[2].tobytes()
    r = P.segment_filter(f, 1.0, 8, segments=True, counts=True)
    assert len(r) == 3 and r[1].cpu().numpy().tobytes() == first[1].tobytes() and r[2].cpu().tolist() == first[3]
    # in place is refused under DYDX, and a short workspace whatever the layout
    d = torch_.from_numpy(as_dydx(f)).cuda()
    with pytest.raises(pkg("_lib").DflowError, match="d_flow and d_out overlap"):
        raw_call(torch_, d, 1.0, 8, 0, d)


def test_a_larger_random_field(torch_):
    h, w = 218, 512
    f = blocks(h, w, 0.7, 5)
    want = R.segment_filter(f, 1.0, 50)
    assert 0 < want[3][1] < want[3][0]
    same(device(f, 1.0, 50), want, "218x512")


# ---- the command lines
def test_spremi_za_epic_segments(torch_, synth, tmp_path, monkeypatch, capsys):
    spz = pkg("spremiZaEpic")
    h, w = 40, 48
    rng = np.random.default_rng(12)
    fwd = np.zeros((h, w, 2))
    fwd[:, w // 2:, 1] = 1                                  # two regions one pixel apart: joined at T = 1
    bwd = np.where(rng.random((h, w, 1)) < 0.62, -fwd, 7.0)  # the others fail the check
    img1 = synth.make_pair(h, w, seed=13)[0]
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    Image.fromarray(img1[..., ::-1].copy()).save("a.png")
    Image.fromarray(img1[..., ::-1].copy()).save("b.png")
    np.save("fwd.npy", fwd)
    np.save("bwd.npy", bwd)
    six = ["a.png", "b.png", "fwd.npy", "bwd.npy", "3", "canny"]
    names = record_calls(monkeypatch)
    for natural, check in (([], "dflow_fb_consistency"), (["--natural-check"], "dflow_flow_consistency")):
        del names[:]
        assert spz.main(six + natural) == 0
        assert names == [check, "dflow_canny_edges"], "without the tokens: the launches it always issued"
        unfiltered = np.load("sparse_field.npy")
        del names[:]
        assert spz.main(six + natural + ["--segments", "20", "1"]) == 0
        assert names == [check, "dflow_segment_filter", "dflow_canny_edges"]
        want = R.segment_filter(unfiltered, 1.0, 20)
        assert 0 < want[3][1] < want[3][0], "segments are both removed and kept"
        got = np.load("sparse_field.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
        pkg("evaluate").parovi(want[0], "want.txt")
        assert open("parovi.txt").read() == open("want.txt").read()
    del names[:]
    assert spz.main(six + ["--natural-check", "--segments", "20", "1", "--gpu-epic"]) == 0
    assert names[:2] == ["dflow_flow_consistency", "dflow_segment_filter"] and "dflow_epic_interpolate" in names
    epic = pkg("flowio").read_flo("epic.flo")
    ivice = pkg("edge").canny_ivice_tensor("a.png")
    assert np.array_equal(epic[..., ::-1], pkg("pipeline").epic_interpolate(want[0], ivice).cpu().numpy())
    assert np.array_equal(np.load("sparse_field.npy"), want[0])
    capsys.readouterr()


def test_run_batch_segments(torch_, tmp_path, monkeypatch, capsys):
    import json
    flowio, rb = pkg("flowio"), pkg("run_batch")
    base = ["--pairs", "1", "--size", "40x48", "--cell", "5x6", "--bcd-times", "2", "--thresh", "2", "--check", "natural"]
    names = record_calls(monkeypatch)
    rb.main(base + ["--out", str(tmp_path / "a")])
    assert names == BATCH_FLOWS + ["dflow_flow_consistency"], "without the option: the launches it always issued"
    del names[:]
    capsys.readouterr()
    rb.main(base + ["--out", str(tmp_path / "b"), "--segments", "20", "1", "--eval"])
    assert names[:len(BATCH_FLOWS) + 2] == BATCH_FLOWS + ["dflow_flow_consistency", "dflow_segment_filter"]
    assert names.count("dflow_segment_filter") == 1
    for d in (0, 1):
        assert np.array_equal(np.load(tmp_path / "b" / flowio.flow_name(0, d, 2)), np.load(tmp_path / "a" / flowio.flow_name(0, d, 2)))
    unfiltered = np.load(tmp_path / "a" / "sparse_field_00.npy")
    want = R.segment_filter(unfiltered, 1.0, 20)
    got = np.load(tmp_path / "b" / "sparse_field_00.npy")
    assert want[3][2] > 0 and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    pkg("evaluate").parovi(got, str(tmp_path / "want.txt"))
    assert open(tmp_path / "b" / "parovi_00.txt").read() == open(tmp_path / "want.txt").read()
    printed = capsys.readouterr().out
    assert "pair 0: %d segments, %d removed; %d consistent pixels, %d removed" % tuple(want[3]) in printed
    assert "pair 0: %.1f%% of the forward flow survives" % (100.0 * got[..., 2].mean()) in printed
    ev = json.load(open(tmp_path / "b" / "eval.json"))
    assert ev["segments"] == [20, 1.0] and ev["pairs"][0]["sparse"]["n_test_valid"] == int(got[..., 2].sum())
