"""The restatement of dflow_epipolar_fit (tests/epipolar_ref.py) against things it was not written from: an SVD / numpy.roots
solver, planted scenes with a rectangle that moves on its own, the planted focus of expansion, the fields that can have no
model; and the mutations of the definition that these must catch (CPU only; the device is compared with the restatement bit for
bit in test_gpu_epipolar.py).

Figures measured on the samples below (300 per scene, 900 in all), restatement against the independent solver, models scaled to
unit Frobenius norm: largest entry difference 1.3e-12 (median 2.5e-14); largest |det| 1.5e-16; largest sample residual
|(p,q,1) F (a,b,1)^T| 5.6e-17; no sample with a different number of models, none degenerate.  The bounds are 100 times these:
the error is governed by how close a root lies to a double root, which varies by orders of magnitude between seeds."""
import numpy as np
import pytest

import epipolar_ref as R
from conftest import pkg

F = np.float32
ENTRY_BOUND = 1.3e-10          # 100 x 1.3e-12
DET_BOUND = 1.5e-14            # 100 x 1.5e-16
RESIDUAL_BOUND = 5.6e-15       # 100 x 5.6e-17
N_SAMPLES = 300


def independent(rows):
    """The models of a sample by numpy.linalg.svd and numpy.roots, unit Frobenius norm: nothing of the restatement in it."""
    A = np.array([[p * a, p * b, p, q * a, q * b, q, a, b, 1.0] for a, b, p, q in rows])
    v = np.linalg.svd(A)[2]
    v1, v2 = v[7].reshape(3, 3), v[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    coeffs = np.polyfit(xs, [np.linalg.det(x * v1 + v2) for x in xs], 3)
    out = []
    for r in np.roots(coeffs):
        if abs(r.imag) <= 1e-9 * (1 + abs(r.real)):
            m = r.real * v1 + v2
            out.append((m / np.linalg.norm(m)).reshape(-1))
    return out


def samples(name, noise=0.1):
    f, _ = R.scene(name, seed=1, noise=noise, moving=False)
    fd = R.Field(f)
    co = R.Coords(fd, 0.5)
    rng = np.random.RandomState(5)
    for _ in range(N_SAMPLES):
        idx = rng.choice(fd.n, 7, replace=False)
        yield R.sample_rows(co, [(fd.xf[i], fd.yf[i], fd.tx[i], fd.ty[i]) for i in idx])


def against_the_independent_solver(name, noise=0.1, **mut):
    """-> (largest entry difference, largest |det|, largest sample residual, samples left out, degenerate samples)."""
    worst = worst_det = worst_res = 0.0
    left_out = degenerate = 0
    for rows in samples(name, noise):
        mine = R.solve7(rows, **mut)
        if mine is None:
            degenerate += 1
            continue
        theirs = independent(rows)
        if len(mine) != len(theirs):
            left_out += 1
            continue
        for m in mine:
            m = np.array(m)
            m = m / np.linalg.norm(m)
            worst = max(worst, min(min(np.abs(m - o).max(), np.abs(m + o).max()) for o in theirs))
            worst_det = max(worst_det, abs(np.linalg.det(m.reshape(3, 3))))
            for a, b, p, q in rows:
                worst_res = max(worst_res, abs(np.array([p, q, 1.0]) @ m.reshape(3, 3) @ np.array([a, b, 1.0])))
    return worst, worst_det, worst_res, left_out, degenerate


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_the_solver_agrees_with_an_svd_and_numpy_roots(name):
    worst, det, res, left_out, degenerate = against_the_independent_solver(name)
    print("%s: entry %.3g det %.3g residual %.3g left out %d degenerate %d" % (name, worst, det, res, left_out, degenerate))
    assert left_out <= 0.02 * N_SAMPLES and degenerate == 0
    assert worst <= ENTRY_BOUND and det <= DET_BOUND and res <= RESIDUAL_BOUND


def test_mutations_of_the_solver_are_caught():
    # partial pivoting with fixed free columns: the noisy scenes lose five orders of magnitude, the exact forward scene models
    for name in sorted(R.SCENES):
        worst, _, _, left_out, _ = against_the_independent_solver(name, complete=False)
        assert worst > ENTRY_BOUND or left_out > 0.02 * N_SAMPLES, name
    worst, _, _, left_out, _ = against_the_independent_solver("forward", noise=0.0, complete=False)
    assert left_out > 0.02 * N_SAMPLES and worst > 1e-3
    # only the roots in [-1, 1]: a third of the samples lose a model
    for name in sorted(R.SCENES):
        assert against_the_independent_solver(name, both_branches=False)[3] > 0.02 * N_SAMPLES, name


def fractions(name, **kw):
    f, mask = R.scene(name, seed=0)
    got = R.fit(f, thresh=0.5, n_hyp=200, lo_rounds=1, seed=0, **kw)
    return float((got["cls"][~mask] == 1).mean()), float((got["cls"][mask] == 1).mean()), got


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_planted_scenes_static_pixels_agree_and_the_moving_rectangle_does_not(name):
    """Measured: sideways 100 % / 0 %, mixed 100 % / 0 %, forward 100 % / 35 %.  On the forward scene the rectangle's motion
    (+3, -4) px is partly along the epipolar lines through it, and no orientation test is made: the known blind spot."""
    static, moving, got = fractions(name)
    print("%s: static %.4f moving %.4f counts %s" % (name, static, moving, got["counts"]))
    assert static >= 0.99
    if name != "forward":
        assert moving <= 0.05
    assert got["counts"][3] >= 0 and got["counts"][5] == got["key"] >> 32 and got["counts"][6] > 1000


def test_the_focus_of_expansion_of_a_forward_motion():
    """Measured over 5 seeds without noise: at most 1.2e-4 px from the planted epipole, the principal point."""
    h, w = R.SCENES["forward"][:2]
    worst = 0.0
    for seed in range(5):
        f, _ = R.scene("forward", seed=seed, noise=0.0, moving=False)
        got = R.fit(f, thresh=0.5, n_hyp=200, lo_rounds=1, seed=0)
        for geo in (R.geometry(got["model"], h, w)[3], pkg("pipeline").epipolar_geometry(got["model"], h, w)["foe"]):
            assert geo is not None
            worst = max(worst, float(np.hypot(geo[0] - (w - 1) * 0.5, geo[1] - (h - 1) * 0.5)))
        assert (got["cls"] == 1).all()
    print("focus of expansion: worst distance %.3g px" % worst)
    assert worst <= 2.0
    # a sideways motion has its epipole at infinity, or as good as: hundreds of frame widths away
    f, _ = R.scene("sideways", seed=0, noise=0.0, moving=False)
    foe = pkg("pipeline").epipolar_geometry(R.fit(f, thresh=0.5, n_hyp=200, seed=0)["model"], h, w)["foe"]
    assert foe is None or abs(foe[0]) > 100 * w


def test_the_geometry_in_pixels_is_the_planted_one():
    """F in pixel coordinates annihilates the planted correspondences, and the package's function is the restatement's."""
    h, w, t, rot = R.SCENES["mixed"]
    f, _ = R.rigid_flow(h, w, 3, t, rot)
    got = R.fit(f.astype(F), thresh=0.5, n_hyp=100, seed=1)
    geo = pkg("pipeline").epipolar_geometry(got["model"], h, w)
    Fp, e1, e2, foe = R.geometry(got["model"], h, w)
    assert np.array_equal(geo["F"], Fp) and np.array_equal(geo["e1"], e1) and np.array_equal(geo["e2"], e2) and geo["foe"] == foe
    ys, xs = np.mgrid[0:h, 0:w]
    x1 = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64)
    x2 = x1 + np.concatenate([f[..., :2], np.zeros((h, w, 1))], -1)
    # the Sampson distance is the same number in pixels and in the normalised coordinates (T is a similarity): the float32
    # residual plane is the float64 distance under F in pixels, to float32 rounding of a cancelling sum of terms below 1
    l, lt = x1 @ Fp.T, x2 @ Fp
    e = (x2 * l).sum(-1)
    sampson = np.abs(e) / np.sqrt(l[..., 0] ** 2 + l[..., 1] ** 2 + lt[..., 0] ** 2 + lt[..., 1] ** 2)
    assert np.abs(got["residual"] - sampson).max() < 1e-3 and sampson.max() < 0.5 and (got["cls"] == 1).all()
    assert (sampson <= 0.5 + 1e-3).all()
    assert np.abs(Fp @ e1).max() <= 1e-9 * np.abs(Fp).max() * np.abs(e1).max()
    assert np.abs(Fp.T @ e2).max() <= 1e-9 * np.abs(Fp).max() * np.abs(e2).max()


def test_synth_rigid_flow_obeys_an_epipolar_geometry_and_make_pair_does_not():
    synth = pkg("synth")
    h, w = 48, 160
    f, mask = synth.rigid_flow(h, w, 0, (0.3, -0.1, 0.6), (0.004, -0.006, 0.003), objects=((12, 80, 28, 120, 3.0, -4.0),))
    assert f.shape == (h, w, 3) and f.dtype == np.float64 and mask.sum() == 16 * 40 and (f[..., 2] == 1).all()
    got = R.fit(f.astype(F), thresh=0.25, n_hyp=100, seed=2)
    assert (got["cls"][~mask] == 1).all() and (got["cls"][mask] == 1).mean() <= 0.05
    fwd, _ = synth.rigid_flow(33, 65, 1, (0.0, 0.0, 0.9), (0.0, 0.0, 0.0))
    foe = pkg("pipeline").epipolar_geometry(R.fit(fwd.astype(F), thresh=0.25, n_hyp=100, seed=2)["model"], 33, 65)["foe"]
    assert np.hypot(foe[0] - 32.0, foe[1] - 16.0) < 0.01
    warp = synth.forward_gt(h, w, 0)[..., ::-1]
    smooth = np.concatenate([warp, np.ones((h, w, 1))], -1).astype(F)
    assert (R.fit(smooth, thresh=0.25, n_hyp=100, seed=2)["cls"] == 1).mean() < 0.5, "a smooth warp is no rigid scene"
    with pytest.raises(ValueError, match="behind"):
        synth.rigid_flow(8, 8, 0, (0.0, 0.0, -20.0), (0.0, 0.0, 0.0))


def no_model(flow, exclude=None, n_hyp=20):
    got = R.fit(flow, n_hyp=n_hyp, lo_rounds=1, exclude=exclude)
    fd = R.Field(flow, exclude)
    assert got["key"] == 0 and not got["model"].any() and not got["models"].any() and not got["hyp_counts"].any()
    assert got["counts"][1:] == [0, 2 * 3 * n_hyp, -1, -1, 0, 0, 0] and got["counts"][0] == fd.scored.size
    assert (got["cls"].reshape(-1)[fd.good & ~fd.excluded] == 2).all() and (got["cls"].reshape(-1)[~fd.good] == 0).all()
    assert np.isinf(got["residual"].reshape(-1)[fd.good]).all() and (got["residual"].reshape(-1)[~fd.good] == -1).all()


def test_fields_that_have_no_model():
    still = np.zeros((9, 11, 3), F)
    still[..., 2] = 1
    no_model(still)                                         # a still camera: the system has rank 6
    f, _ = R.scene("mixed", moving=False)
    no_model(np.ascontiguousarray(f[:1, :9]))               # a line of pixels
    six = np.ascontiguousarray(f[:5, :7])
    six[..., 2] = 0
    six.reshape(-1, 3)[[0, 5, 9, 17, 22, 30], 2] = 1
    no_model(six)                                           # six participants
    seven = np.ascontiguousarray(f[:5, :7])
    ex = np.ones((5, 7), np.uint8)
    ex.reshape(-1)[[0, 5, 9, 17, 22, 30]] = 0
    no_model(seven, ex)                                     # and six by exclusion


def test_the_boundary_of_the_inlier_test_belongs_to_the_inliers():
    """A vector whose e*e equals (t*t)*den exactly is an inlier; `<` for `<=` loses it.  F = [0,0,0; 0,0,1; 0,0,0] has l1 = 1, den = 1
    and e = q, so q = t is the boundary."""
    m = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], F)
    t = F(0.5) * F(1 / 64)
    a = b = p = F(0.125)
    for q, want in ((t, True), (np.nextafter(t, F(1)), False), (-t, True), (F(0), True)):
        assert bool(R.inlier(m, a, b, p, q, F(t * t))) == want
    assert not R.inlier(m, a, b, p, t, F(t * t), strict=True), "the mutation is visible here"
    # a denominator that overflowed, or a NaN, is no inlier, whatever the threshold
    big = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
    assert not R.inlier(big, a, b, F(1e30), F(1e30), F(1.0)) and not R.inlier(big, a, b, F(np.nan), p, F(1.0))
    assert not R.inlier(np.zeros(9, F), a, b, p, p, F(1.0)), "den = 0: the all-zero model has no inliers"
    # and in a whole fit: a field that lies on the boundary everywhere
    h, w = 8, 8
    flow = np.zeros((h, w, 3), F)
    flow[..., 2] = 1
    fd = R.Field(flow)
    co = R.Coords(fd, 0.5)
    co.q = co.b + F(0.5) * F(co.s)                         # V = 0.5 px: e = q - b for the model below, den = 2
    side = np.array([0, 0, 0, 0, 0, 1, 0, -1, 0], F)
    ee, den = R.terms(side, co.a, co.b, co.p, co.q)
    assert (den == 2).all() and (ee == F(0.5 * co.s) ** 2).all()
    thresh2 = F(F(0.5) * F(co.s)) ** 2 / F(2)               # (t*t)*den == e*e exactly
    assert R.inlier(side, co.a, co.b, co.p, co.q, thresh2).all() and not R.inlier(side, co.a, co.b, co.p, co.q, thresh2, strict=True).any()


def test_the_restatement_is_deterministic_and_uses_every_argument():
    f, _ = R.scene("sideways", seed=2)
    f, ex = R.dirty(f, 3)
    a = R.fit(f, thresh=0.5, n_hyp=40, lo_rounds=2, step=2, seed=(7 << 32) | 5, exclude=ex)
    b = R.fit(f, thresh=0.5, n_hyp=40, lo_rounds=2, step=2, seed=(7 << 32) | 5, exclude=ex)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
    assert a["counts"][0] == int((R.Field(f, ex, 2).part & R.Field(f, ex, 2).on_grid).sum()) and (a["cls"][ex != 0] != 1).all()
    for kw in (dict(seed=5), dict(step=1), dict(thresh=0.4), dict(exclude=None), dict(lo_rounds=0)):
        c = R.fit(f, **dict(dict(thresh=0.5, n_hyp=40, lo_rounds=2, step=2, seed=(7 << 32) | 5, exclude=ex), **kw))
        assert c["key"] != a["key"] or c["counts"] != a["counts"], kw
    assert np.isfinite(f[..., :2][a["cls"] == 1]).all() and (np.abs(f[..., :2][a["cls"] == 1]) < 1e20).all()
