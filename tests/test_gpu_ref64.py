"""The HIP path against the float64 references of tests/ref64.py, not against the oracle: a mistake the oracle and the kernels
share fails here.  Needs a real MI355X: run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import ref64 as R
from conftest import pkg

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "f16")
DAISY_SHAPES = [(8, 8), (9, 13), (40, 56), (97, 131), (436, 1024), (375, 1242)]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def new_pass(H, W, ch, cw, storage="f32", seed=0, **over):
    L = pkg("_lib")
    flags = L.FLAG_DESCR_F16 if storage == "f16" else 0
    return pkg("pipeline").DiscreteFlow(H, W, ch, cw, seed=seed, flags=flags, **over)


def gpu_daisy(img, storage="f32"):
    H, W = img.shape[:2]
    df = new_pass(H, W, max(1, H // 4), max(5, W // 4), storage)          # cells of at least knn = 5 points
    df.izracunajDaisy(img, out=df.descrs1)
    return df.descriptors_f32(0).cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def image(H, W, style):
    return pkg("synth").make_pair(H, W, seed=H + W, style=style)[0]


@functools.lru_cache(maxsize=None)
def daisy_ref(H, W, style):
    return R.daisy64(image(H, W, style))


# ---------------------------------------------------------------------------------------------------------------- DAISY

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", DAISY_SHAPES)
def test_daisy_within_float64_bound(torch_, shape, storage):
    """f32 planes within R.DAISY_ATOL of daisy64; binary16 planes within half an ulp of binary16 plus that (R.f16_bound)."""
    H, W = shape
    for style in ("dense", "low_texture"):
        ref = daisy_ref(H, W, style)
        got = gpu_daisy(image(H, W, style), storage)
        bound = R.DAISY_ATOL if storage == "f32" else R.f16_bound(ref)
        err = np.abs(got - ref) - bound
        assert err.max() <= 0, (style, np.unravel_index(err.argmax(), err.shape), got.flat[err.argmax()], ref.flat[err.argmax()])


@pytest.mark.parametrize("storage", STORAGES)
def test_daisy_of_a_constant_image_is_zero(torch_, storage):
    """Blurs of a constant are the same constant at every pixel (replicate borders), so every difference is exactly 0."""
    img = np.full((37, 53, 3), (10, 200, 77), np.uint8)
    assert not gpu_daisy(img, storage).any()


@pytest.mark.parametrize("storage", STORAGES)
def test_daisy_of_ramps(torch_, storage):
    """B=G=R=x with W <= 256: gray = x/255 exactly (the weights sum to 2^14), a unit-slope ramp of 1/255 per px.  Away from
    the replicated borders every blur keeps it, the central difference is 1/255, and every interior histogram is
    (1/255, 0, 0, 0); the vertical ramp gives (0, 1/255, 0, 0)."""
    H, W = 60, 200
    m = 24                                                        # clears the blur radii, the grid radius and the zeroing
    for axis, want in ((1, [1, 0, 0, 0]), (0, [0, 1, 0, 0])):
        n = W if axis == 1 else H
        ramp = np.arange(n, dtype=np.uint8)
        img = np.broadcast_to(ramp[None, :, None] if axis == 1 else ramp[:, None, None], (H, W, 3)).copy()
        d = gpu_daisy(img, storage).reshape(H, W, 17, 4)[m:H - m, m:W - m]
        exp = np.broadcast_to(np.array(want, np.float64) / 255.0, d.shape)
        bound = R.DAISY_ATOL if storage == "f32" else R.f16_bound(exp)
        assert (np.abs(d - exp) <= bound).all(), (axis, np.abs(d - exp).max())


def perm_descr(d, layers, angles):
    """Descriptor (H,W,68) with histogram bins permuted by `layers` and the ring angles of every ring by `angles`."""
    d = d.reshape(d.shape[:2] + (17, 4))[..., layers]
    regions = [0] + [1 + 4 * r + angles[a] for r in range(4) for a in range(4)]
    return d[:, :, regions].reshape(d.shape[:2] + (68,))


# Each image transform maps gradients and grid offsets the same way.  Bins are the layers max(0, cos(l 90deg) dx +
# sin(l 90deg) dy) = (+dx, +dy, -dx, -dy); ring angle a sits at offset (dy, dx) = r (sin, cos)(a 90deg) = +x, +y, -x, -y.
#   horizontal flip: dx -> -dx and x offsets negate: layers 0<->2, angles 0<->2
#   vertical flip:   dy -> -dy and y offsets negate: layers 1<->3, angles 1<->3
#   transpose:       dx <-> dy and offsets swap axes: layers 0<->1, 2<->3, angles 0<->1, 2<->3
#   rot90 (np.rot90 = vertical flip of the transpose): transpose, then vertical flip
HFLIP = (lambda a: a[:, ::-1], [2, 1, 0, 3])
VFLIP = (lambda a: a[::-1], [0, 3, 2, 1])
TRANSPOSE = (lambda a: a.transpose(1, 0, 2), [1, 0, 3, 2])
TRANSFORMS = {"transpose": [TRANSPOSE], "hflip": [HFLIP], "vflip": [VFLIP], "rot90": [TRANSPOSE, VFLIP]}


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_daisy_commutes_with_flips_and_rotations(torch_, name, storage):
    """DAISY(T(img)) = T(P(DAISY(img))) with P the bin/angle permutation of T, on the interior: 24 px clear the blur radii
    (2 + 1 + 3 + 1 + 2 + 3 + 4), the grid radius 5 and the 2-px zeroing."""
    H, W, m = 70, 90, 24
    img = image(H, W, "dense")
    d = gpu_daisy(img, storage)
    timg, want = img, d
    for spatial, perm in TRANSFORMS[name]:
        timg = np.ascontiguousarray(spatial(timg))
        want = np.ascontiguousarray(spatial(perm_descr(want, perm, perm)))
    if name == "rot90":
        assert np.array_equal(timg, np.rot90(img))
    got = gpu_daisy(timg, storage)
    assert got.shape == want.shape
    g, w = got[m:-m, m:-m], want[m:-m, m:-m]
    bound = 2 * R.DAISY_ATOL if storage == "f32" else 2 * R.f16_bound(w)
    assert (np.abs(g - w) <= bound).all(), np.abs(g - w).max()


# ------------------------------------------------------------------------------------------------------- kNN, neighbours

def knn_pass(H, W, ch, cw, storage="f32", d=None, seed=0):
    """A pass with its kNN stage run; returns (df, d1, d2, host state), d1/d2 the planes the kernels read, as float32."""
    df = new_pass(H, W, ch, cw, storage, seed=seed)
    if d is None:
        img1, img2, _ = pkg("synth").make_pair(H, W, seed=H * W + 1, amp_x=0.1 * W, amp_y=0.1 * H)
        df.load_pair(img1, img2)
    else:
        df.set_descriptors(*d)
    df.generisi()
    d1, d2 = df.descriptors_f32(0).cpu().numpy(), df.descriptors_f32(1).cpu().numpy()
    return df, d1, d2, df.host_state()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("geom", [(45, 70, 7, 9), (11, 17, 2, 3), (8, 23, 1, 5), (40, 48, 5, 6), (64, 200, 10, 12)])
def test_knn_and_neighbour_stage_whole_frames(torch_, geom, storage):
    H, W, ch, cw = geom
    df, d1, d2, st = knn_pass(H, W, ch, cw, storage)
    g = R.Geom(H, W, ch, cw)
    assert R.knn_check(d1, d2, g, st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"]) == []
    df.nasumicni()
    nb = df.host_state()
    rng = np.random.default_rng(H)
    pix = (rng.integers(0, H, 300), rng.integers(0, W, 300))
    assert R.neighbour_check(d1, d2, g, nb["proposals"], nb["lcosts"], nb["nprop"], st["bestlabels"], df.p.ngauss, pix) == []


def test_knn_at_the_bench_geometry(torch_):
    """1024x436 with 64x27 cells: 436 = 16 x 27 + 4, the last cell row absorbs 4 rows.  Every group that searches that row
    (all pixels of the three cell rows whose window reaches it), the four corners and 2 000 seeded pixels in full."""
    H, W, ch, cw = 436, 1024, 27, 64
    df, d1, d2, st = knn_pass(H, W, ch, cw)
    g = R.Geom(H, W, ch, cw)
    args = (d1, d2, g, st["proposals"], st["lcosts"], st["nprop"])
    yy, xx = np.meshgrid(np.arange((g.ncy - 1 - g.window) * ch, H), np.arange(W), indexing="ij")
    bottom = {(ci, g.ncy - 1) for ci in range(g.ncx)}
    assert R.knn_check(*args, None, pixels=(yy.ravel(), xx.ravel()), cells=bottom) == []
    rng = np.random.default_rng(436)
    ys = np.concatenate([[0, 0, H - 1, H - 1], rng.integers(0, H, 2000)])
    xs = np.concatenate([[0, W - 1, 0, W - 1], rng.integers(0, W, 2000)])
    assert R.knn_check(*args, st["bestlabels"], pixels=(ys, xs)) == []


@pytest.mark.parametrize("storage", STORAGES)
def test_knn_in_the_largest_screened_cell(torch_, storage):
    """255x257 as one cell: 65 535 points, the most the MFMA screen takes; sampled queries, the last row included."""
    H, W = 255, 257
    img1, img2, _ = pkg("synth").make_pair(H, W, seed=41, amp_x=1.5, amp_y=1.0)
    df = new_pass(H, W, H, W, storage, seed=3)
    df.load_pair(img1, img2)
    df.generisi()
    d1, d2, st = df.descriptors_f32(0).cpu().numpy(), df.descriptors_f32(1).cpu().numpy(), df.host_state()
    rng = np.random.default_rng(5)
    ys = np.concatenate([[0, H - 1, H - 1], np.full(8, H - 1), rng.integers(0, H, 150)])
    xs = np.concatenate([[0, 0, W - 1], rng.integers(0, W, 8), rng.integers(0, W, 150)])
    assert R.knn_check(d1, d2, R.Geom(H, W, H, W), st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"],
                       pixels=(ys, xs)) == []


@pytest.mark.parametrize("case", ("near_ties", "zeros", "large_rows"))
def test_knn_on_adversarial_descriptors(torch_, case):
    """Descriptors uploaded with set_descriptors: candidates 1 ulp apart in one coordinate, all-zero rows (exact ties), and
    rows with |x|^2 >= 30 000, outside the f16 screen's range."""
    H, W, ch, cw = 30, 44, 6, 8
    rng = np.random.default_rng(("near_ties", "zeros", "large_rows").index(case))
    d1 = rng.uniform(0, 0.05, (H, W, 68)).astype(np.float32)
    d2 = rng.uniform(0, 0.05, (H, W, 68)).astype(np.float32)
    if case == "near_ties":
        base = rng.uniform(0, 0.05, 68).astype(np.float32)
        d2[:] = base
        k = rng.integers(0, 68, (H, W))
        v = d2[np.arange(H)[:, None], np.arange(W)[None], k]
        d2[np.arange(H)[:, None], np.arange(W)[None], k] = np.nextafter(v, np.float32(1))
        d1[::2] = base
    elif case == "zeros":
        d1[rng.random((H, W)) < 0.3] = 0
        d2[rng.random((H, W)) < 0.3] = 0
    else:
        big = rng.random((H, W)) < 0.2
        d2[big] = rng.uniform(20.0, 25.0, (int(big.sum()), 68)).astype(np.float32)
        d1[rng.random((H, W)) < 0.1] = 22.0
    df, e1, e2, st = knn_pass(H, W, ch, cw, d=(d1, d2))
    assert np.array_equal(e1, d1) and np.array_equal(e2, d2)
    assert R.knn_check(d1, d2, R.Geom(H, W, ch, cw), st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"]) == []


# ------------------------------------------------------------------------------------------------------------------ BCD

def run_phases(df, phases, chains=None):
    """Run `phases` one at a time, checking each against the float64 Viterbi (R.bcd_phase_check)."""
    st = df.host_state()
    pr, lc, npr = st["proposals"], st["lcosts"], st["nprop"]
    bl = st["bestlabels"]
    for k, phase in enumerate(phases):
        df.bcd_phase(phase)
        after = df.bestlabels.cpu().numpy().astype(np.int64)
        assert R.bcd_phase_check(pr, lc, npr, bl, after, phase, lamda=df.p.lamda, tpsi=df.p.tpsi,
                                 chains=None if chains is None else chains(phase)) == [], k
        bl = after
    return bl


@pytest.mark.parametrize("case", ("all_compatible", "ties", "sparse_labels", "mixed_lengths"))
def test_bcd_adversarial_states_at_pitch_160(torch_, case):
    """The adversarial label sets at label pitch 160, lists up to 160 long.  all_compatible needs about 30x more 160-bit rows
    than the pool holds, so most rows are rebuilt one predecessor at a time; mixed_lengths exceeds the per-wave block caps.
    Two sweeps, every chain of every phase at its Viterbi minimum."""
    from test_ref64 import BCD_CASES, adversarial_state
    H, W, ch, cw = 40, 44, 8, 11
    pr, lc, npr, bl = adversarial_state(case, H, W, 160, BCD_CASES.index(case) + 1)
    df = new_pass(H, W, ch, cw, seed=1, maxnprop=160)
    df.set_host_state(pr, lc, npr, bl)
    run_phases(df, list(range(4)) * 2)


def real_pass(H, W, ch, cw, seed=0):
    img1, img2, _ = pkg("synth").make_pair(H, W, seed=seed + H, amp_x=0.08 * W, amp_y=0.08 * H)
    df = new_pass(H, W, ch, cw, seed=seed)
    df.load_pair(img1, img2)
    df.generisi()
    df.nasumicni()
    return df


def test_bcd_real_pass(torch_):
    run_phases(real_pass(96, 128, 12, 16), list(range(4)))


def test_bcd_chains_of_8192(torch_):
    """8x8192: the row phases run chains of 8 192 pixels (all checked); of the 4 096 column chains, 64 spread ones."""
    run_phases(real_pass(8, 8192, 4, 512), list(range(4)), lambda phase: None if phase % 2 else np.arange(0, 4096, 64))


def test_bcd_batch_of_nine_passes(torch_):
    """ceoBCD_batch over 9 passes (two launches, the second of one pass): every pass's labels after one sweep equal its own
    phase-by-phase run, whose every chain is checked against the Viterbi minimum."""
    pl = pkg("pipeline")
    H, W, ch, cw = 24, 40, 6, 8
    passes = [real_pass(H, W, ch, cw, seed=k) for k in range(9)]
    singles = [real_pass(H, W, ch, cw, seed=k) for k in range(9)]
    pl.ceoBCD_batch(passes, 1)
    for k, (a, b) in enumerate(zip(passes, singles)):
        want = run_phases(b, list(range(4)))
        assert np.array_equal(a.bestlabels.cpu().numpy(), want), k


def test_bcd_bench_geometry_four_sweeps(torch_):
    """1024x436, cells 64x27, 4 sweeps: every phase leaves the labels off its chains alone, and 3 chains per phase (first,
    middle, last) reach their Viterbi minimum."""
    df = real_pass(436, 1024, 27, 64)

    def chains(phase):
        n = len(R.phase_chains(436, 1024, phase)[0])
        return [0, n // 2, n - 1]
    run_phases(df, list(range(4)) * 4, chains)
