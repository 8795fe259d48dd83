"""The CPU oracle against the float64 references of tests/ref64.py, at the shapes the golden fixtures lack: ragged cell grids,
frames up to 436x1024, label pitch 160.  No GPU needed."""
import numpy as np
import pytest

import ref64 as R

SHAPES = [(8, 8), (9, 13), (40, 56), (97, 131), (436, 1024), (375, 1242)]


@pytest.fixture
def O(oracle):
    oracle.set_threads(8)
    try:
        yield oracle
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_daisy_within_tolerance(O, synth, shape):
    """Measured max |oracle - daisy64| (dense / low-texture pair, image 1): 8x8 2.1e-8 / 2.8e-8, 9x13 1.3e-8 / 2.5e-8,
    40x56 1.6e-8 / 2.6e-8, 97x131 2.2e-8 / 2.3e-8, 436x1024 3.7e-8 / 2.9e-8, 375x1242 3.0e-8 / 3.3e-8, for descriptor values
    up to 0.17.  R.DAISY_ATOL = 1.5e-7 is 4x the largest (3.7e-8); it is absolute, which is also its floor near zero."""
    H, W = shape
    for style in ("dense", "low_texture"):
        img, _, _ = synth.make_pair(H, W, seed=H + W, style=style)
        err = np.abs(O.daisy(img).astype(np.float64) - R.daisy64(img))
        assert err.max() <= R.DAISY_ATOL, (style, err.max(), np.unravel_index(err.argmax(), err.shape))


def test_daisy_column0_drops_the_270_degree_ring(O, synth):
    """The ring points at 270 degrees sit at (y - 1.25 (r+1), x + 1.25 (r+1) cos(3pi/2)), and cos(3pi/2) = -1.8e-16 in
    double: in column 0 the float32 x coordinate is negative and the inside test drops all four points, in column 1 it does
    not.  The oracle does this, daisy64 with the libm offsets does this, and exact offsets would keep the points."""
    H, W = 40, 48
    img, _, _ = synth.make_pair(H, W, seed=7)
    d = O.daisy(img).reshape(H, W, 17, 4)
    ring270 = [1 + 4 * r + 3 for r in range(4)]
    rows = slice(6, H - 2)                                  # y - 5 >= 0 for every ring, and clear of the bottom zeroing
    assert not d[rows, 0][:, ring270].any()
    assert (d[rows, 1][:, ring270].sum(-1) > 0).all()
    exact = R.daisy64(img, exact_grid=True).reshape(H, W, 17, 4)
    assert (exact[rows, 0][:, ring270].sum(-1) > 0).all()
    libm = R.daisy64(img).reshape(H, W, 17, 4)
    assert not libm[rows, 0][:, ring270].any()
    assert np.abs(libm - d).max() <= R.DAISY_ATOL


# (H, W, cellh, cellw): ragged in x, in y, in both, single-pixel-high cells, and the benchmark's 27x64 cells on a frame
# whose last cell row absorbs 5 rows and last cell column 10 columns
KNN_GEOMS = [(45, 70, 7, 9), (11, 17, 2, 3), (8, 23, 1, 5), (40, 48, 5, 6), (140, 330, 27, 64)]


@pytest.mark.parametrize("geom", KNN_GEOMS)
def test_oracle_knn_and_neighbour_stage(O, synth, geom):
    H, W, ch, cw = geom
    img1, img2, _ = synth.make_pair(H, W, seed=H * W, amp_x=0.1 * W, amp_y=0.1 * H)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    p = O.make_params(H, W, ch, cw, seed=5)
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    g = R.Geom(H, W, ch, cw)
    assert R.knn_check(d1, d2, g, pr, lc, npr, bl) == []
    wta = bl.copy()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    rng = np.random.default_rng(H)
    pix = (rng.integers(0, H, 300), rng.integers(0, W, 300))
    assert R.neighbour_check(d1, d2, g, pr, lc, npr, wta, p.ngauss, pix) == []


def adversarial_state(case, H, W, L, seed):
    """The label sets of test_gpu_parity.py::test_bcd_adversarial_label_sets_match_oracle, at label pitch L (lists up to L
    long): every label compatible with every neighbour label, exact cost ties, very short lists next to full ones, and
    clusters of every size 1..41."""
    rng = np.random.default_rng(seed)
    proposals = np.full((H, W, L, 2), -1, np.int64)
    lcosts = np.full((H, W, L), 1000.0, np.float64)
    nprop = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if case == "all_compatible":          # all flows inside a 3x3 box: |d|_1 <= 4 < tpsi for every pair
                n = L
                f = rng.integers(-1, 2, size=(n, 2))
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            elif case == "ties":
                n = int(rng.integers(L - 50, L + 1))
                f = rng.integers(-6, 7, size=(n, 2)) * np.array([1, 2])
                c = rng.choice(np.array([0.5, 1.0, 2.5], np.float32), n)
            elif case == "sparse_labels":
                n = int(rng.choice([1, 2, 5, L]))
                f = rng.integers(-30, 31, size=(n, 2))
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            else:                                 # mixed_lengths: clusters of growing size
                n = L
                f = np.zeros((n, 2), np.int64)
                k = cl = 0
                while k < n:
                    m = min(n - k, cl % 41 + 1)
                    f[k:k + m] = np.array([40 * (cl % 7) - 120, 30 * (cl // 7) - 60]) + rng.integers(-1, 2, size=(m, 2))
                    k += m
                    cl += 1
                c = rng.uniform(0.0, 2.5, n).astype(np.float32)
            proposals[y, x, :n] = f
            lcosts[y, x, :n] = c.astype(np.float64)
            nprop[y, x] = n
    bestlabels = rng.integers(0, nprop)
    return proposals, lcosts, nprop, bestlabels


BCD_CASES = ("all_compatible", "ties", "sparse_labels", "mixed_lengths")


@pytest.mark.parametrize("case", BCD_CASES)
def test_oracle_bcd_phases_reach_the_chain_minimum_at_pitch_160(O, case):
    H, W = 12, 16
    pr, lc, npr, bl = adversarial_state(case, H, W, 160, BCD_CASES.index(case) + 1)
    p = O.make_params(H, W, 4, 4, maxnprop=160)
    for phase in range(4):
        before = bl.copy()
        O.bcd_phase(p, pr, lc, npr, bl, phase)
        assert R.bcd_phase_check(pr, lc, npr, before, bl, phase) == [], (case, phase)


def test_oracle_bcd_phases_on_a_real_pass(O, synth):
    H, W, ch, cw = 45, 70, 7, 9
    img1, img2, _ = synth.make_pair(H, W, seed=3, amp_x=5.0, amp_y=3.0)
    p = O.make_params(H, W, ch, cw, seed=2)
    ref = O.full_pass(p, img1, img2, 0)
    pr, lc, npr, bl = ref["proposals"], ref["lcosts"], ref["nprop"], ref["bestlabels"]
    for sweep in range(2):
        for phase in range(4):
            before = bl.copy()
            O.bcd_phase(p, pr, lc, npr, bl, phase)
            assert R.bcd_phase_check(pr, lc, npr, before, bl, phase) == [], (sweep, phase)


def test_bcd_check_rejects_a_suboptimal_chain(O, synth):
    """The Viterbi check is not vacuous: one chain label moved to another label is caught unless the energy is tied."""
    H, W = 12, 16
    pr, lc, npr, bl = adversarial_state("sparse_labels", H, W, 160, 3)
    p = O.make_params(H, W, 4, 4, maxnprop=160)
    before = bl.copy()
    O.bcd_phase(p, pr, lc, npr, bl, 0)
    y = int(np.flatnonzero(npr[:, 0] == 160)[0])
    vmin, e = R.chain_energies(pr, lc, npr, before, bl, 0, chains=[0])
    worse = bl.copy()
    worse[y, 0] = (bl[y, 0] + 1) % 160
    vmin2, e2 = R.chain_energies(pr, lc, npr, before, worse, 0, chains=[0])
    assert vmin2[0] == vmin[0] and e[0] == pytest.approx(vmin[0], rel=1e-12) and e2[0] > vmin[0] + 1e-6
    assert R.bcd_phase_check(pr, lc, npr, before, worse, 0) != []
