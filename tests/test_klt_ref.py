"""tests/klt_ref.py, the numpy restatement of include/dflow_klt.h, against the truth: a pure shift, the smooth warps of
synth.make_pair with their ground truth, large motion with and without the pyramid, and the properties the definition promises.
The bounds are the issue's, from the prototype the definition was settled on; the figures this restatement reaches are printed, and
stand in DESIGN.md "Sparse feature tracking".  CPU only."""
import numpy as np
import pytest

import klt_ref as R

F = R.F
# the prototype's values
ARGS = dict(r=7, iters=20, eps=0.01, min_eig=1e-3, fb=0.5)
CORNER_ARGS = dict(rc=2, min_dist=4, quality=0.01)


def follow(img1, img2, levels, border=4):
    """Corners of img1 followed into img2: (positions, klt_ref.track's result)."""
    p1, p2 = R.pyramid(img1, levels), R.pyramid(img2, levels)
    _, mask, _, _ = R.corners(p1[0], border=border, **CORNER_ARGS)
    pos = R.corner_positions(mask)
    return pos, R.track(p1, p2, pos, np.full(len(pos), R.LIVE, np.int32), **ARGS)


@pytest.fixture(scope="module")
def warps(synth):
    """The three smooth warps, each followed once: seed -> (pos, result, gt)."""
    out = {}
    for seed in range(3):
        img1, img2, gt = synth.make_pair(192, 256, seed, amp_x=6, amp_y=4)
        out[seed] = follow(img1, img2, 3) + (gt,)
    return out


def test_pure_shift(synth):
    img1 = synth.make_pair(96, 128, 0)[0]
    img2 = np.roll(img1, (2, 3), (0, 1))
    pos, (pos_out, state, err, back, counts) = follow(img1, img2, 3, border=12)
    dev = np.abs((pos_out - pos) - np.array([3, 2], F)).max()
    print("pure shift: %d corners, largest deviation %.4f px, largest err %.5f" % (len(pos), dev, err.max()))
    assert len(pos) > 20 and (state == R.LIVE).all()
    assert dev <= 0.01 and err.max() <= 0.01 and err.min() >= 0
    assert counts.tolist()[:6] == [len(pos), 0, 0, 0, 0, 0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_smooth_warp(warps, seed):
    pos, (pos_out, state, err, back, counts), gt = warps[seed]
    live = state == R.LIVE
    truth = gt[pos[:, 1].astype(int), pos[:, 0].astype(int)][:, ::-1]                  # [dy,dx] -> [dx,dy]
    epe = np.linalg.norm((pos_out - pos).astype(np.float64) - truth, axis=1)[live]
    print("warp seed %d: %d corners, %.1f %% pass, %.1f %% of them within 1 px, median %.3f px"
          % (seed, len(pos), 100 * live.mean(), 100 * (epe < 1).mean(), np.median(epe)))
    assert len(pos) >= 250
    assert live.mean() >= 0.95
    assert (epe < 1).mean() >= 0.97
    assert np.median(epe) <= 0.35


@pytest.mark.parametrize("seed", [0, 1])
def test_the_pyramid_keeps_large_motion(synth, seed):
    img1, img2, _ = synth.make_pair(192, 256, seed, amp_x=16, amp_y=8)
    kept = {levels: int((follow(img1, img2, levels)[1][1] == R.LIVE).sum()) for levels in (4, 1)}
    print("large motion seed %d: %d consistent tracks with 4 levels, %d with 1" % (seed, kept[4], kept[1]))
    assert kept[4] > kept[1] > 0


def test_slots_that_are_not_live_and_starts_outside(synth):
    img1, img2, _ = synth.make_pair(64, 80, 3, amp_x=2, amp_y=2)
    p1, p2 = R.pyramid(img1, 2), R.pyramid(img2, 2)
    c = R.corner_positions(R.corners(p1[0], border=10)[1])
    pos = np.array([c[0], [np.nan, 5], [79.5, 10], [-0.25, 3], [30, 63.5], c[len(c) // 2] + F(0.25), [7, 7], [50, 30]], F)
    state = np.array([R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LEFT, R.FREE], np.int32)
    pos[6] = np.nan                                                                  # whatever an ended slot holds
    pos_out, st, err, back, counts = R.track(p1, p2, pos, state, **ARGS)
    assert st[1:5].tolist() == [R.LEFT] * 4 and st[6] == R.LEFT and st[7] == R.FREE and st[0] == R.LIVE and st[5] == R.LIVE
    assert np.array_equal(pos_out[[1, 2, 3, 4, 6, 7]].view(np.uint32), pos[[1, 2, 3, 4, 6, 7]].view(np.uint32))
    assert (err[[1, 2, 3, 4, 6, 7]] == -1).all() and (err[[0, 5]] >= 0).all() and np.isnan(back[[1, 2, 3, 4, 6, 7]]).all()
    assert counts[:6].sum() == len(pos) and counts.tolist()[:6] == [2, 4, 0, 0, 0, 2] and counts[7] == 0


def test_a_constant_image_is_flat_and_has_no_corner():
    img = np.full((40, 50, 3), 93, np.uint8)
    pyr = R.pyramid(img, 3)
    assert all((L == pyr[0][0, 0]).all() for L in pyr)
    resp, mask, counts, rmax = R.corners(pyr[0], quality=0.0)
    assert rmax == 0 and not resp.any() and not mask.any() and counts.tolist() == [0, 0, 0, 0]
    pos = np.array([[10, 10], [25.5, 20.25], [0, 0]], F)
    pos_out, st, err, back, counts = R.track(pyr, pyr, pos, np.full(3, R.LIVE, np.int32), **ARGS)
    assert (st == R.FLAT).all() and np.array_equal(pos_out, pos) and counts.tolist() == [0, 0, 3, 0, 0, 0, 0, 0] and (err == -1).all()


def test_corners_keep_their_distance_and_live_tracks_suppress(synth):
    img = synth.make_pair(96, 128, 5)[0]
    Y = R.grey(img)
    for min_dist in (1, 4, 9):
        _, mask, counts, _ = R.corners(Y, min_dist=min_dist, border=3)
        ys, xs = np.nonzero(mask)
        assert len(ys) == counts[3] > 5 and counts[1] == counts[3] and counts[2] == 0 and counts[0] >= counts[1]
        assert ys.min() >= 3 and xs.min() >= 3 and ys.max() <= 96 - 4 and xs.max() <= 128 - 4
        cheb = np.maximum(np.abs(ys[:, None] - ys[None]), np.abs(xs[:, None] - xs[None]))
        np.fill_diagonal(cheb, 10 ** 6)
        assert cheb.min() >= min_dist + 1
    # a live track on every other corner (a quarter pixel off), an ended one and one beyond n on two more
    _, mask, counts, _ = R.corners(Y)
    pos = R.corner_positions(mask)
    n = len(pos)
    state = np.full(n, R.LIVE, np.int32)
    state[1::2] = R.FREE
    state[3] = R.LEFT
    tracks = ((pos + F(0.25)), state, n - 2)
    _, mask2, counts2, _ = R.corners(Y, tracks=tracks)
    gone = np.zeros(n, bool)
    gone[0:n - 2:2] = True
    assert counts2[1] == counts[1] and counts2[2] == gone.sum() and counts2[3] == n - gone.sum()
    assert np.array_equal(R.corner_positions(mask2), pos[~gone])
    # quality 1 keeps the strongest response alone
    resp, mask1, counts1, rmax = R.corners(Y, quality=1.0, border=0)
    assert counts1[0] == (resp == rmax).sum() and counts1[3] >= 1 and (resp[mask1 != 0] == rmax).all()


def test_the_pyramid_is_pyr_down_of_the_grey_image(synth):
    import pyramid_ref
    img = synth.make_pair(33, 65, 2)[0]
    pyr = R.pyramid(img, 4)
    assert [L.shape for L in pyr] == R.level_sizes(33, 65, 4) == [(33, 65), (17, 33), (9, 17), (5, 9)]
    for a, b in zip(pyr, pyr[1:]):
        assert np.array_equal(pyramid_ref.pyr_down(np.repeat(a[..., None], 3, 2))[..., 0], b)
    offs, total = R.level_offsets(33, 65, 4)
    assert offs == [0, 2145, 2145 + 561, 2145 + 561 + 153] and total == 2145 + 561 + 153 + 45
    back = R.unpack(R.pack(pyr), 33, 65, 4)
    assert all(np.array_equal(a, b) for a, b in zip(pyr, back))
    b, g, r = (int(v) for v in img[7, 9])
    assert pyr[0][7, 9] == (29 * b + 150 * g + 77 * r + 128) >> 8
