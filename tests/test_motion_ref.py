"""Properties of the definition of dflow_motion_fit, on its restatement (tests/motion_ref.py; CPU only): a planted model is
recovered, degenerate fields give no model, the polish never loses inliers, exclude / lo_rounds / step mean what the header says,
two planted motions come apart, and the polish sums stay inside int64.  The seeds and n_hyp are chosen so that the restatement
itself satisfies the recovery: a condition on the inputs, not a tolerance on the code under test."""
import numpy as np
import pytest

import motion_ref as R

F = np.float32
H, W = 33, 65


def test_philox_is_the_oracles(oracle):
    for c0, c1, seed in ((0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 17, 0x9E3779B97F4A7C15), (65535, (4 * 4 + 3) * 16 + 15, 1 << 32)):
        assert R.philox(c0, c1, seed & R.M32, seed >> 32) == int(oracle.philox(c0, c1, seed)[0])


@pytest.mark.parametrize("kind,model,polish", (("affine", R.AFFINE, 2), ("homography", R.HOMOGRAPHY, 0)))
def test_a_planted_model_is_recovered(kind, model, polish):
    f, planted, _ = R.field(H, W, 1, kind, outliers=0.4)
    assert 0.3 * H * W < planted.sum() < 0.6 * H * W
    got = R.fit(f, model, thresh=1.0, n_hyp=96, lo_rounds=1, polish=polish, seed=0)
    assert (got["cls"][planted] == 1).all(), "every planted pixel is an inlier of the final model"
    assert got["counts"][1] >= planted.sum() and got["counts"][3] >= 0 and got["counts"][4] >= 0
    assert R.corner_shift(got["model"], R.PLANTED[kind], H, W) < 1.0, "every frame corner lands within thresh of the planted one"
    if model == R.AFFINE:
        assert got["model"][6:].tolist() == [0.0, 0.0, 1.0] and (got["models"][:, 6:] == [0, 0, 1]).all()
        assert got["counts"][6] >= 1, "a polish step was accepted"
    else:
        assert got["counts"][6] == 0 and R.fit(f, model, n_hyp=96, polish=4, seed=0)["model"].tobytes() == got["model"].tobytes(), \
            "a homography is not polished"
    # the model's flow and the residual: planted pixels have next to no residual
    r = got["residual"][planted]
    assert (r[:, 2] == 1).all() and np.abs(r[:, :2]).max() < 0.05
    good = R.Field(f).good.reshape(H, W)
    assert (got["residual"][~good] == 0).all() and (got["model_flow"][..., 2] == 1).all()


@pytest.mark.parametrize("model", (R.AFFINE, R.HOMOGRAPHY))
def test_degenerate_fields_give_no_model(model):
    fields = [R.field(1, 1, 2, "affine", outliers=0, dirty=False)[0], R.field(1, 7, 2, "affine", outliers=0, dirty=False)[0],
              R.field(17, 19, 2, "collinear")[0], R.field(7, 1, 2, "collinear")[0], R.field(9, 9, 2, "allbad")[0]]
    for f in fields:
        got = R.fit(f, model, n_hyp=40, lo_rounds=2, polish=2, seed=5)
        assert got["key"] == 0 and got["counts"][2:7] == [3 * 40, -1, -1, 0, 0]
        assert np.array_equal(got["model"], R.IDENTITY) and not got["hyp_counts"].any() and (got["models"] == R.IDENTITY).all()
        assert (got["model_flow"] == [0, 0, 1]).all(), "the identity's flow"


def test_the_polish_never_lowers_the_inlier_count():
    for seed in range(6):
        f, _, ex = R.field(H, W, 10 + seed, "affine", outliers=0.5)
        # one hypothesis, a wide threshold: a poor start the polish can improve
        for n_hyp, thresh in ((1, 3.0), (4, 1.0), (64, 0.25)):
            got = R.fit(f, R.AFFINE, thresh=thresh, n_hyp=n_hyp, lo_rounds=0, polish=4, seed=seed, exclude=ex)
            assert got["steps"] == sorted(got["steps"]) and got["counts"][1] == got["steps"][-1]
            assert got["counts"][6] <= 4 and got["steps"][0] == got["counts"][5]


def test_exclude_is_honoured_in_sampling_scoring_and_classes():
    f, planted, ex = R.field(H, W, 20, "affine")
    fd = R.Field(f, ex)
    for j in range(64):
        pts = R.draw_points(fd, R.HOMOGRAPHY, F(1.0), 9, 0, j, R.IDENTITY)
        for x, y, _, _ in pts or ():
            assert not ex[int(y), int(x)] and fd.good[int(y) * W + int(x)]
        assert pts is None or len({(float(x), float(y)) for x, y, _, _ in pts}) == 4, "the points of a sample differ"
    got = R.fit(f, R.AFFINE, n_hyp=64, seed=9, exclude=ex)
    # excluding a pixel equals removing its vector, but for the class it gets
    holes = f.copy()
    holes[ex != 0, 2] = 0
    ref = R.fit(holes, R.AFFINE, n_hyp=64, seed=9)
    for k in ("model", "models", "hyp_counts", "model_flow"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert got["key"] == ref["key"] and got["counts"] == ref["counts"]
    assert got["counts"][0] == int(fd.part.sum()) < int(fd.good.sum())
    mask = (ex != 0) & fd.good.reshape(H, W)
    assert (got["cls"][mask] == 3).all() and (ref["cls"][mask] == 0).all() and np.array_equal(got["cls"][~mask], ref["cls"][~mask])
    assert (got["residual"][mask][:, 2] == 1).all(), "an excluded good pixel still has a residual"


def test_later_rounds_draw_only_from_inliers():
    f, planted, ex = R.field(H, W, 30, "affine")
    fd = R.Field(f, ex)
    first = R.fit(f, R.AFFINE, n_hyp=32, lo_rounds=0, polish=0, seed=4, exclude=ex)
    assert first["key"]
    for r in (1, 2):
        for j in range(32):
            pts = R.draw_points(fd, R.AFFINE, F(1.0), 4, r, j, first["model"])
            for x, y, tx, ty in pts or ():
                assert R.inlier(first["model"], x, y, tx, ty, F(1.0))
    # so every hypothesis of a later round that exists is made of inliers, and the best count cannot fall
    more = R.fit(f, R.AFFINE, n_hyp=32, lo_rounds=2, polish=0, seed=4, exclude=ex)
    assert more["counts"][5] >= first["counts"][5]
    assert more["key"] >> 32 > first["key"] >> 32 or more["key"] == first["key"], "at equal counts the earlier round stays"


def test_step_changes_what_is_scored_not_what_is_classified():
    f, planted, ex = R.field(H, W, 40, "affine")
    good = R.Field(f).good.reshape(H, W)
    for step in (1, 2, 3, 64):
        got = R.fit(f, R.AFFINE, n_hyp=64, seed=2, step=step, exclude=ex)
        fd = R.Field(f, ex, step)
        assert got["counts"][0] == int((fd.part & fd.on_grid).sum()) == fd.scored.size
        assert ((got["cls"] == 0) == ~good).all() and (got["cls"][good & (ex != 0)] == 3).all()
        if step <= 3:
            assert (got["cls"][planted & (ex == 0)] == 1).all(), "pixels off the grid are classified too"
            assert got["counts"][1] <= got["counts"][0] < (got["cls"] == 1).sum() + (got["cls"] == 2).sum() or step == 1
    assert R.fit(f, R.AFFINE, n_hyp=64, seed=2, step=2)["models"].tobytes() == R.fit(f, R.AFFINE, n_hyp=64, seed=2)["models"].tobytes(), \
        "round 0 samples every pixel whatever the step"


def test_two_planted_motions_come_apart():
    f, which = R.two_motions(H, W)
    models, layer = R.layers(f, 2, n_hyp=64, seed=1)
    assert np.array_equal(layer, which), "the larger motion is layer 1, the other layer 2"
    assert R.corner_shift(models[0], R.PLANTED["affine"], H, W) < 1.0 and R.corner_shift(models[1], R.PLANTED["affine2"], H, W) < 1.0
    models, layer = R.layers(f, 3, n_hyp=64, seed=1)
    assert (layer != 3).all() and np.array_equal(models[2], R.IDENTITY), "nothing is left for a third fit"


def test_the_polish_sums_fit_int64_at_the_largest_frame():
    w = h = 8192
    worst = [0] * 12
    for x, y in ((0, 0), (w - 1, h - 1), (0, h - 1)):
        for tx, ty in ((32768.0, 32768.0), (-32768.0, 32768.0), (-32768.0, -32768.0)):
            S = R.polish_sums(w, h, [x], [y], [F(tx)], [F(ty)])
            worst = [max(a, abs(b)) for a, b in zip(worst, S)]
    assert worst[1] == worst[2] == 8191 and worst[6] == worst[9] == 1 << 21
    assert all(v * (1 << 26) < 1 << 60 for v in worst), "2^26 pixels of the largest terms"
    assert np.nextafter(F(32768.0), F(np.inf)) > R.POLISH_RANGE, "the next float is outside the range"
    # and the solve takes such sums: a pure translation of every pixel of a 64 x 64 corner at the far end
    xs, ys = np.meshgrid(np.arange(w - 64, w), np.arange(h - 64, h))
    S = R.polish_sums(w, h, xs.ravel(), ys.ravel(), (xs.ravel() + 2.5).astype(F), (ys.ravel() - 1.25).astype(F))
    m = R.polish_solve(w, h, S)
    assert np.allclose(m, [1, 0, 2.5, 0, 1, -1.25, 0, 0, 1], atol=1e-3)
    assert R.polish_solve(w, h, R.polish_sums(w, h, [1, 2], [1, 2], [F(1), F(2)], [F(1), F(2)])) is None, "N < 3"
    assert R.polish_solve(w, h, R.polish_sums(w, h, [1, 2, 3], [1, 2, 3], [F(1), F(2), F(3)], [F(1), F(2), F(3)])) is None, "a line"
