"""The CPU oracle against the float64 references of tests/ref64.py away from the reference's constants: tpsi 1..8, lamda from 0
to the largest value the C-ABI accepts, tphi from 0 to above every L1 distance, window 0 and 1, ngauss 0 and 64, and the law
of the neighbour sampler's draws.  tests/test_gpu_ref64_params.py runs the same grid on the HIP path; a failure here and not
there is the oracle's, one there and not here the kernels'.  No GPU needed."""
import math

import numpy as np
import pytest

import ref64 as R
from test_ref64 import BCD_CASES, adversarial_state

DP_SENTINEL = 800000.0
"""The reference's start value of permmincost and of the end label's minimum (python bcd.py:152-157, :231), DFLOW_DP_SENTINEL."""

TPSIS = (1, 2, 3, 5, 7, 8)
LAMDAS = (0.0, 0.05, 1.0, "largest")
TPHIS = (0.0, 0.75, 2.5, 100.0)
WINDOW_NGAUSS = ((0, 0), (0, 64), (1, 25), (1, 64), (2, 0))
SAMPLER_SIGMAS = (8.0, 2.5, 0.5)
SAMPLER_SEEDS = (7, 0x9E3779B97F4A7C15)          # the second has a non-zero high word (the Philox key's second half)
SAMPLER_N = 512
SAMPLER_MAXKNN = 45                                # window 1: 9 cells of K = 5


def dp_bound(n, tpsi, lamda, tphi):
    """max(pich, picw) * (3 tpsi + lamda tphi) as dflow_check_params computes it: double, tphi widened from float32."""
    return n * (3.0 * tpsi + lamda * float(np.float32(tphi)))


def largest_lamda(n, tpsi, tphi):
    """The largest double lamda the C-ABI accepts for chains of n pixels: dp_bound(n, tpsi, lamda, tphi) < DP_SENTINEL."""
    lam = (DP_SENTINEL / n - 3.0 * tpsi) / float(np.float32(tphi))
    while dp_bound(n, tpsi, lam, tphi) >= DP_SENTINEL:
        lam = float(np.nextafter(lam, -math.inf))
    while dp_bound(n, tpsi, float(np.nextafter(lam, math.inf)), tphi) < DP_SENTINEL:
        lam = float(np.nextafter(lam, math.inf))
    return lam


def lamda_value(lamda, n, tpsi=8, tphi=2.5):
    return largest_lamda(n, tpsi, tphi) if lamda == "largest" else lamda


def check_phases(O, p, pr, lc, npr, bl, phases, chains=None):
    """Run `phases` of the oracle one at a time, each checked against the float64 Viterbi of its chains; returns the labels."""
    for k, phase in enumerate(phases):
        before = bl.copy()
        O.bcd_phase(p, pr, lc, npr, bl, phase)
        assert R.bcd_phase_check(pr, lc, npr, before, bl, phase, lamda=p.lamda, tpsi=p.tpsi,
                                 chains=None if chains is None else chains(phase)) == [], (k, phase)
    return bl


@pytest.fixture
def O(oracle):
    oracle.set_threads(8)
    try:
        yield oracle
    finally:
        oracle.set_threads(1)


def oracle_pass(O, synth, H, W, ch, cw, seed=0, **over):
    img1, img2, _ = synth.make_pair(H, W, seed=seed + H, amp_x=0.08 * W, amp_y=0.08 * H)
    p = O.make_params(H, W, ch, cw, seed=seed, **over)
    r = O.full_pass(p, img1, img2, 0)
    return p, r


# ------------------------------------------------------------------------------------------------------------ the grid

@pytest.mark.parametrize("tpsi", TPSIS)
def test_oracle_bcd_across_tpsi(O, synth, tpsi):
    """tpsi = 1: only identical flows are compatible; 7 and 8 fill the 3-bit cost field of the kernel's records.  A real pass
    and the four adversarial states at label pitch 160, one sweep each, every chain at its Viterbi minimum."""
    p, r = oracle_pass(O, synth, 45, 70, 7, 9, seed=tpsi, tpsi=tpsi)
    check_phases(O, p, r["proposals"], r["lcosts"], r["nprop"], r["bestlabels"], range(4))
    for case in BCD_CASES:
        pr, lc, npr, bl = adversarial_state(case, 12, 16, 160, BCD_CASES.index(case) + 1)
        check_phases(O, O.make_params(12, 16, 4, 4, maxnprop=160, tpsi=tpsi), pr, lc, npr, bl, range(4))


@pytest.mark.parametrize("lamda", LAMDAS)
def test_oracle_bcd_across_lamda(O, synth, lamda):
    H, W = 45, 70
    lam = lamda_value(lamda, max(H, W))
    p, r = oracle_pass(O, synth, H, W, 7, 9, seed=3, lamda=lam)
    check_phases(O, p, r["proposals"], r["lcosts"], r["nprop"], r["bestlabels"], list(range(4)) * 2)


def assert_tphi_above_every_l1(d1, d2, tphi):
    """No L1 distance between a descriptor of image 1 and one of image 2 reaches tphi (the triangle bound)."""
    assert np.abs(d1).sum(-1).max() + np.abs(d2).sum(-1).max() < tphi


@pytest.mark.parametrize("tphi", TPHIS)
def test_oracle_stages_across_tphi(O, synth, tphi):
    """kNN costs min(tphi, L1), the WTA label, the neighbour stage's costs and one BCD sweep.  tphi = 0: every cost is 0
    and the WTA label is slot 0; tphi = 100: no cost is clipped."""
    H, W, ch, cw = 40, 56, 8, 8
    img1, img2, _ = synth.make_pair(H, W, seed=11, amp_x=4.0, amp_y=3.0)
    p = O.make_params(H, W, ch, cw, seed=4, tphi=tphi)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    if tphi == TPHIS[-1]:
        assert_tphi_above_every_l1(d1, d2, tphi)
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    g = R.Geom(H, W, ch, cw, tphi=tphi)
    assert R.knn_check(d1, d2, g, pr, lc, npr, bl) == []
    wta = bl.copy()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    rng = np.random.default_rng(H)
    pix = (rng.integers(0, H, 300), rng.integers(0, W, 300))
    assert R.neighbour_check(d1, d2, g, pr, lc, npr, wta, p.ngauss, pix) == []
    check_phases(O, p, pr, lc, npr, bl, range(4))


@pytest.mark.parametrize("window,ngauss", WINDOW_NGAUSS)
def test_oracle_knn_and_neighbours_across_window_and_ngauss(O, synth, window, ngauss):
    """maxnprop = (2 window + 1)^2 K + ngauss, the least the ABI accepts: a pixel whose draws all land fills its list."""
    H, W, ch, cw = 45, 70, 7, 9
    img1, img2, _ = synth.make_pair(H, W, seed=window * 100 + ngauss, amp_x=5.0, amp_y=3.0)
    maxnprop = (2 * window + 1) ** 2 * 5 + ngauss
    p = O.make_params(H, W, ch, cw, seed=9, window=window, ngauss=ngauss, maxnprop=maxnprop)
    d1, d2 = O.daisy(img1), O.daisy(img2)
    pr, lc, npr, bl = O.knn_proposals(p, d1, d2)
    g = R.Geom(H, W, ch, cw, window=window)
    assert R.knn_check(d1, d2, g, pr, lc, npr, bl) == []
    wta = bl.copy()
    O.neighbour_proposals(p, d1, d2, pr, lc, npr, bl)
    rng = np.random.default_rng(window + ngauss)
    pix = (rng.integers(0, H, 300), rng.integers(0, W, 300))
    assert R.neighbour_check(d1, d2, g, pr, lc, npr, wta, ngauss, pix) == []
    if ngauss:
        assert (npr > g.nknn(*np.indices((H, W)))).mean() > 0.99


def near_bound_state(st, tphi):
    """A real pass's state with every used cost set to tphi (float32-exact), the largest each stage can write."""
    pr, lc, npr, bl = (st[k] for k in ("proposals", "lcosts", "nprop", "bestlabels"))
    lc = lc.copy()
    lc[np.arange(lc.shape[2])[None, None, :] < npr[..., None]] = float(np.float32(tphi))
    return pr, lc, npr, bl.copy()


def test_oracle_bcd_near_the_sentinel(O, synth):
    """8x1024, every used cost = tphi and lamda the largest accepted: the row chains' DP climbs past 0.9 x 800000 and every
    chain still reaches its Viterbi minimum (the sentinels never bind)."""
    H, W, tphi = 8, 1024, 2.5
    lam = largest_lamda(W, 8, tphi)
    p, r = oracle_pass(O, synth, H, W, 4, 128, seed=1, lamda=lam)
    pr, lc, npr, bl = near_bound_state(r, tphi)
    vmin, _ = R.chain_energies(pr, lc, npr, bl, bl, 1, lamda=lam, tpsi=8)
    assert vmin.min() > 0.9 * DP_SENTINEL and vmin.max() < DP_SENTINEL
    check_phases(O, p, pr, lc, npr, bl, range(4), lambda phase: None if phase % 2 else np.arange(0, W // 2, 16))


# --------------------------------------------------------------------------------------------------- the sampler's law

def sampler_draws(neighbour, sigma, seed, n=SAMPLER_N):
    """Run a neighbour stage `neighbour(params, d1, d2, proposals, lcosts, nprop, bestlabels)` (the oracle's signature) on
    R.sampler_state at n x n with cells of 64 x 64, window 1 (maxknn = 45), ngauss 1 and maxnprop 48 (the lists this test
    needs, a third of the host memory of 160); returns the (n,n,2) positions it appended."""
    pr, lc, npr, bl = R.sampler_state(n, n, SAMPLER_MAXKNN, 48)
    d = np.zeros((n, n, 68), np.float32)
    neighbour(dict(window=1, ngauss=1, maxnprop=48, sigma=sigma, seed=seed), d, d, pr, lc, npr, bl)
    assert (npr == SAMPLER_MAXKNN + 2).all(), "every pixel appends exactly one label"
    return pr[:, :, SAMPLER_MAXKNN + 1]


def oracle_neighbour(O, n=SAMPLER_N):
    def run(over, d1, d2, pr, lc, npr, bl):
        O.neighbour_proposals(O.make_params(n, n, 64, 64, **over), d1, d2, pr, lc, npr, bl)
    return run


@pytest.mark.parametrize("seed", SAMPLER_SEEDS)
@pytest.mark.parametrize("sigma", SAMPLER_SIGMAS)
def test_oracle_sampler_follows_the_truncated_normal_law(O, sigma, seed):
    """The oracle's draws against R.gauss_offset_law by G-tests (R.sampler_law_check): the interior joint law of (dy, dx) and
    the law of the drawn row / column at distances 0..15 from the top and left borders.  Fails for a threshold table shifted
    by one, floor() instead of int() truncation, a wrong sigma and correlated coordinates."""
    bad, res = R.sampler_law_check(sampler_draws(oracle_neighbour(O), sigma, seed), sigma)
    assert bad == [], bad
    assert res[0][2] >= (3 if sigma < 1 else 100)          # the interior test has degrees of freedom to speak of


def test_gauss_offset_law_by_simulation():
    """gauss_offset_law against int(c + sigma z) of 2e6 numpy normals, and the G-test machinery on data drawn from the law
    itself (accepts) and from floor() instead of int() (rejects)."""
    rng = np.random.default_rng(0)
    z = rng.standard_normal(2_000_000)
    for sigma, c in ((8.0, 0), (8.0, 5), (2.5, 0), (2.5, 3), (0.5, 0), (0.5, 1)):
        v = (c + sigma * z).astype(np.int64)                  # numpy's float -> int cast truncates toward zero, like int()
        v = v[(v >= 0) & (v < 64)]
        law, clip = R.gauss_offset_law(c, 64, sigma)
        assert clip < 2e-15
        G, df = R.g_test(np.bincount(v, minlength=64), law)
        assert G <= R.chi2_upper_quantile(df, R.SAMPLER_ALPHA), (sigma, c, G, df)
        f = np.floor(c + sigma * z).astype(np.int64)
        f = f[(f >= 0) & (f < 64)]
        G, df = R.g_test(np.bincount(f, minlength=64), law)
        assert G > R.chi2_upper_quantile(df, R.SAMPLER_ALPHA), (sigma, c, G, df)
    # the Wilson-Hilferty quantile against the exact chi-square(2) one, -2 ln(alpha): within 10 %, on the safe side
    exact = -2 * math.log(R.SAMPLER_ALPHA)
    assert exact <= R.chi2_upper_quantile(2, R.SAMPLER_ALPHA) <= 1.1 * exact
