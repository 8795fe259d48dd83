"""pyramid_ref.compose, the coarse-to-fine run on the CPU (the oracle's stages, pyramid_ref, prior_ref), on the reach case: it
regenerates REACH_PIXELS, the number tests/test_gpu_pyramid.py compares the device with (CPU only, a few seconds)."""
import numpy as np

import pyramid_ref as R
from conftest import pkg


def test_reach_pixels_is_what_the_cpu_composition_gives(oracle, synth):
    c, shift = R.REACH["cell"], R.REACH["shift"]
    H, W = R.REACH["H"], R.REACH["W"]
    img1, img2 = R.reach_pair(synth)
    assert np.array_equal(img2[:, shift:], img1[:, :W - shift]) and (img2[:, :shift] == img1[:, :1]).all()
    levels = pkg("pipeline").pyramid_levels
    threads = oracle.get_threads()
    oracle.set_threads(8)
    try:
        two = R.compose(oracle, levels(H, W, 2, c, c, window=1), img1, img2, R.REACH["sweeps"], seed=R.REACH["seed"])
    finally:
        oracle.set_threads(threads)

    def at_shift(flow):
        return int(((flow[..., 0] == 0) & (flow[..., 1] == shift)).sum())
    assert np.abs(two[1]["flow"][..., 1]).max() <= 2 * c - 1, "a level reaches 15 px: the coarse level holds the shift as (0,12)"
    assert at_shift(two[0]["flow"]) == R.REACH_PIXELS
    assert R.REACH_PIXELS > H * (W - shift) // 2
    assert sum(two[0]["upsample_counts"]) == H * W and sum(two[0]["prior_counts"]) == 5 * H * W
