"""The HIP path against the float64 references of tests/ref64.py away from the reference's constants: the grid of
tests/test_ref64_params.py (tpsi 1..8, lamda 0 .. the largest the C-ABI accepts, tphi 0 .. above every L1 distance, window 0
and 1, ngauss 0 and 64, both descriptor storages), chains of 8192 whose DP comes within a factor 1.6 of the reference's
800000 sentinels, and the law of the neighbour sampler's draws.  Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import ref64 as R
from conftest import pkg
from test_gpu_ref64 import STORAGES, new_pass, run_phases
from test_ref64 import BCD_CASES, adversarial_state
from test_ref64_params import (LAMDAS, SAMPLER_SEEDS, SAMPLER_SIGMAS, TPHIS, TPSIS, WINDOW_NGAUSS, DP_SENTINEL,
                               assert_tphi_above_every_l1, lamda_value, largest_lamda, near_bound_state, sampler_draws)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def real_pass(H, W, ch, cw, seed=0, storage="f32", **over):
    """A pass through DAISY, kNN and the neighbour stage on a synthetic pair; returns (df, d1, d2, host state after kNN)."""
    img1, img2, _ = pkg("synth").make_pair(H, W, seed=seed + H, amp_x=0.08 * W, amp_y=0.08 * H)
    df = new_pass(H, W, ch, cw, storage, seed=seed, **over)
    df.load_pair(img1, img2)
    df.generisi()
    knn = df.host_state()
    df.nasumicni()
    return df, df.descriptors_f32(0).cpu().numpy(), df.descriptors_f32(1).cpu().numpy(), knn


def check_stages(df, d1, d2, knn, g, npix=300):
    """The kNN stage's state `knn` (every pixel; the WTA label against the kNN costs) and the labels the neighbour stage
    appended since, at npix seeded pixels; returns the state after the neighbour stage."""
    wta = knn["bestlabels"]
    assert R.knn_check(d1, d2, g, knn["proposals"], knn["lcosts"], knn["nprop"], wta) == []
    st = df.host_state()
    rng = np.random.default_rng(g.H + g.W)
    pix = (rng.integers(0, g.H, npix), rng.integers(0, g.W, npix))
    assert R.neighbour_check(d1, d2, g, st["proposals"], st["lcosts"], st["nprop"], wta, df.p.ngauss, pix) == []
    return st


# ------------------------------------------------------------------------------------------------------------ the grid

@pytest.mark.parametrize("tpsi", TPSIS)
def test_bcd_across_tpsi(torch_, tpsi):
    """tpsi = 1: only identical flows are compatible; 7 and 8 fill the 3-bit cost field of the chain kernel's records.  A real
    pass and the four adversarial states at label pitch 160, one sweep each, every chain at its Viterbi minimum."""
    df, _, _, _ = real_pass(64, 96, 8, 12, seed=tpsi, tpsi=tpsi)
    run_phases(df, range(4))
    for case in BCD_CASES:
        H, W = 24, 32
        st = adversarial_state(case, H, W, 160, BCD_CASES.index(case) + 1)
        df = new_pass(H, W, 8, 8, seed=1, maxnprop=160, tpsi=tpsi)
        df.set_host_state(*st)
        run_phases(df, range(4))


@pytest.mark.parametrize("lamda", LAMDAS)
def test_bcd_across_lamda(torch_, lamda):
    """lamda = 0: the data term drops out and only the smoothness terms decide; the largest accepted for the frame makes the
    data term dominate.  Two sweeps, every chain at its Viterbi minimum."""
    H, W = 64, 96
    df, _, _, _ = real_pass(H, W, 8, 12, seed=3, lamda=lamda_value(lamda, max(H, W)))
    run_phases(df, list(range(4)) * 2)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("tphi", TPHIS)
def test_stages_across_tphi(torch_, tphi, storage):
    """kNN costs min(tphi, L1) and the WTA label, the neighbour stage's costs, and one BCD sweep.  tphi = 0: every cost is 0
    and the WTA label is slot 0; tphi = 100: no cost is clipped."""
    H, W, ch, cw = 48, 64, 8, 8
    df, d1, d2, knn = real_pass(H, W, ch, cw, seed=11, storage=storage, tphi=tphi)
    if tphi == TPHIS[-1]:
        assert_tphi_above_every_l1(d1, d2, tphi)
    if tphi == 0:
        assert not knn["bestlabels"].any()
    check_stages(df, d1, d2, knn, R.Geom(H, W, ch, cw, tphi=tphi))
    run_phases(df, range(4))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("window,ngauss", WINDOW_NGAUSS)
def test_knn_and_neighbours_across_window_and_ngauss(torch_, window, ngauss, storage):
    """maxnprop = (2 window + 1)^2 K + ngauss, the least the ABI accepts, at label pitch 160."""
    H, W, ch, cw = 45, 70, 7, 9
    maxnprop = (2 * window + 1) ** 2 * 5 + ngauss
    df, d1, d2, knn = real_pass(H, W, ch, cw, seed=9, storage=storage, window=window, ngauss=ngauss, maxnprop=maxnprop)
    g = R.Geom(H, W, ch, cw, window=window)
    st = check_stages(df, d1, d2, knn, g)
    if ngauss:
        assert (st["nprop"] > g.nknn(*np.indices((H, W)))).mean() > 0.99


def test_bcd_near_the_sentinel(torch_, oracle):
    """8x8192 uploaded with set_host_state, every used cost = tphi and lamda the largest the ABI accepts for 8192-pixel chains
    (29.46): the row chains' Viterbi minimum exceeds 5e5, within a factor 1.6 of the 800000 sentinels.  All four phases reach
    the Viterbi minimum (every row chain, 64 spread column chains) and equal the oracle's labels bit for bit."""
    H, W, tphi = 8, 8192, 2.5
    lam = largest_lamda(W, 8, tphi)
    df, _, _, _ = real_pass(H, W, 4, 512, seed=2, lamda=lam)
    pr, lc, npr, bl = near_bound_state(df.host_state(), tphi)
    df.set_host_state(pr, lc, npr, bl)
    vmin, _ = R.chain_energies(pr, lc, npr, bl, bl, 1, lamda=lam, tpsi=8)
    assert vmin.min() > 5e5 and vmin.max() < DP_SENTINEL
    after = run_phases(df, range(4), lambda phase: None if phase % 2 else np.arange(0, W // 2, 64))
    O = oracle
    O.set_threads(8)
    try:
        p = O.make_params(H, W, 4, 512, seed=2, lamda=lam)
        for phase in range(4):
            O.bcd_phase(p, pr, lc, npr, bl, phase)
    finally:
        O.set_threads(1)
    assert np.array_equal(after, bl)


# --------------------------------------------------------------------------------------------------- the sampler's law

def gpu_neighbour(storage="f32"):
    """The neighbour stage of a DiscreteFlow in the oracle's signature (see test_ref64_params.sampler_draws)."""
    def run(over, d1, d2, pr, lc, npr, bl):
        H, W = npr.shape
        df = new_pass(H, W, 64, 64, storage, label_pitch=48, **over)
        df.set_descriptors(d1, d2)
        df.set_host_state(pr, lc, npr, bl)
        df.nasumicni()
        st = df.host_state()
        pr[...], lc[...], npr[...] = st["proposals"], st["lcosts"], st["nprop"]
    return run


@pytest.mark.parametrize("seed", SAMPLER_SEEDS)
@pytest.mark.parametrize("sigma", SAMPLER_SIGMAS)
def test_sampler_follows_the_truncated_normal_law(torch_, sigma, seed):
    """DiscreteFlow.nasumicni's draws against R.gauss_offset_law by G-tests (R.sampler_law_check), on the state of
    R.sampler_state at 512x512: the interior joint law of (dy, dx), and the drawn row / column at distances 0..15 from the
    top and left borders, where int() truncation shows."""
    bad, res = R.sampler_law_check(sampler_draws(gpu_neighbour(), sigma, seed), sigma)
    assert bad == [], bad
