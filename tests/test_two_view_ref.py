"""The restatement of dflow_two_view (tests/two_view_ref.py) pinned by hand, on the CPU: with the exact F^ of a known (R, t, K),
computed here with np.linalg and cast to float32, every candidate index is reached, a pixel without parallax and a thing that
moves against the epipolar direction get their classes, the pose and the depths are the planted ones, inputs without a pose
answer NO POSE, and each mutation of the definition fails one of these checks.  And synth.rigid_depth against synth.rigid_flow.

Accuracy, measured with the restatement over the three scenes and the seeds 0..5 (float32 flows, float32 F^): the rotation is off
by at most 1.64e-7 degrees, |t - t_true/|t_true|| is at most 7.75e-9, and the relative depth error Z1 |t_true| / Z - 1 over
the pixels of class 1 is at most 2.25e-5 (set by the float32 flow where the parallax is smallest, next to the focus of
expansion).  The bounds are four times these, the project's convention: 6.6e-7 degrees, 3.1e-8 and 9.0e-5."""
import itertools

import numpy as np
import pytest

import epipolar_ref as E
import two_view_ref as T
from conftest import pkg

F = np.float32
ROT_BOUND_DEG, T_BOUND, DEPTH_BOUND = 6.6e-7, 3.1e-8, 9.0e-5
AGAINST = (-6.0, 0.0)               # px, against the sideways camera's +3 px


def sign_cases():
    for name in ("sideways", "forward", "mixed"):
        h, w, t, rot = E.SCENES[name]
        for ts, fs in itertools.product((1.0, -1.0), (1.0, -1.0)):
            yield name, h, w, tuple(ts * v for v in t), rot, fs


def check_candidates(**mut):
    """Negating F^ swaps R_a and R_b, negating t the sign: each index wins once per scene, with every vote."""
    won = {}
    for name, h, w, t, rot, fs in sign_cases():
        flow = T.camera_flow(h, w, 0, t, rot)[0].astype(F)
        out = T.two_view(flow, T.exact_model(h, w, t, rot, sign=fs), **mut)
        cand = out["counts"][3]
        assert cand >= 0, (name, t, fs, "no pose")
        assert sum(out["votes"]) == out["votes"][cand] == out["counts"][1], (name, t, fs, out["votes"])
        assert out["counts"][1] >= out["counts"][0] - 1, "every voter with parallax votes for the winner"
        assert T.rotation_error_deg(out["pose"][:9], rot) < 1e-4 and np.linalg.norm(out["pose"][9:12] - np.array(t) / np.linalg.norm(t)) < 1e-6
        won.setdefault(name, []).append(cand)
    assert all(sorted(v) == [0, 1, 2, 3] for v in won.values()), won
    return won


def test_each_candidate_index_is_reached():
    won = check_candidates()
    assert won["sideways"] == [0, 2, 1, 3] and won["forward"] == [0, 2, 1, 3] and won["mixed"] == [3, 1, 2, 0]


def test_no_parallax_at_the_focus_of_expansion():
    h, w, t, rot = E.SCENES["forward"]
    flow = T.camera_flow(h, w, 0, t, rot)[0].astype(F)
    assert not flow[16, 32, :2].any(), "the focus of expansion has no flow"
    out = T.two_view(flow, T.exact_model(h, w, t, rot))
    assert out["cls"][16, 32] == 3 and out["depth"][16, 32] == 0 and np.isposinf(out["err"][16, 32])
    assert out["counts"] == [h * w, h * w - 1, 0, 0, h * w - 1, 0, 1, 0], "it is a voter and votes for nobody"
    assert (out["cls"] == 1).sum() == h * w - 1


def against_scene():
    h, w, t, rot = E.SCENES["sideways"]
    box = (h // 4, w // 2, h // 4 + h // 3, w // 2 + w // 4)
    flow, Z, mask = T.camera_flow(h, w, 0, t, rot, objects=(box + AGAINST,))
    assert (flow[..., 0][~mask] > 2.0).all() and (flow[..., 0][mask] < -1.0).all(), "the camera's +2 .. +5 px, the rectangle 6 px against it"
    return h, w, t, rot, flow.astype(F), mask


def check_object_against_the_epipolar_direction(**mut):
    h, w, t, rot, flow, mask = against_scene()
    model = T.exact_model(h, w, t, rot)
    # it lies on its epipolar line: the fit cannot tell it from the scene
    co = E.Coords(E.Field(flow), 0.01)
    assert E.inlier(model, co.a, co.b, co.p, co.q, co.t2).all()
    out = T.two_view(flow, model, **mut)
    assert (out["cls"][mask] == 2).all() and (out["cls"][~mask] == 1).all(), "class 2 everywhere inside, nowhere outside"
    assert (out["depth"][mask] < 0).all() and (out["depth"][~mask] > 0).all()
    assert out["counts"][3] == 0 and out["counts"][1:3] == [int((~mask).sum()), int(mask.sum())], "the rectangle votes for (R_a, -t)"
    # one voter of the scene and one of the rectangle: a tie, which goes to the smaller index
    part = np.zeros((h, w), np.uint8)
    part[0, 0] = part[h // 4 + 1, w // 2 + 1] = 1
    tie = T.two_view(flow, model, part=part, **mut)
    assert tie["votes"] == [1, 1, 0, 0] and tie["counts"][:4] == [2, 1, 1, 0]
    assert np.array_equal(tie["cls"], out["cls"]) and tie["pose"].tobytes() == out["pose"].tobytes()
    # bytes other than 1 do not vote
    part[1, :] = 2
    part[2, :] = 255
    assert T.two_view(flow, model, part=part, **mut)["votes"] == [1, 1, 0, 0]


def test_an_object_that_moves_against_the_epipolar_direction_is_class_2():
    check_object_against_the_epipolar_direction()


def check_accuracy(**mut):
    worst = [0.0, 0.0, 0.0]
    for name in ("sideways", "forward", "mixed"):
        h, w, t, rot = E.SCENES[name]
        model, tl = T.exact_model(h, w, t, rot), float(np.linalg.norm(t))
        for seed in range(6):
            flow, Z, _ = T.camera_flow(h, w, seed, t, rot)
            out = T.two_view(flow.astype(F), model, **mut)
            ok = out["cls"] == 1
            assert ok.sum() >= h * w - 1
            got = [T.rotation_error_deg(out["pose"][:9], rot), float(np.linalg.norm(out["pose"][9:12] - np.array(t) / tl)),
                   float(np.abs(out["depth"][ok].astype(np.float64) * tl / Z[ok] - 1.0).max())]
            worst = [max(a, b) for a, b in zip(worst, got)]
            # the planted point reprojects onto the float32 target
            assert out["err"][ok].max() < 1e-4
    print("worst rotation error %.3g deg, translation error %.3g, relative depth error %.3g" % tuple(worst))
    assert worst[0] <= ROT_BOUND_DEG and worst[1] <= T_BOUND and worst[2] <= DEPTH_BOUND, worst
    return worst


def test_the_pose_and_the_depths_are_the_planted_ones():
    worst = check_accuracy()
    assert worst[2] > DEPTH_BOUND / 8, "the bound is four times what was measured, not more"


def test_other_intrinsics():
    h, w, t, rot = E.SCENES["mixed"]
    K = (170.0, 131.5, 90.25, 17.75)                                # fx != fy, an off-centre principal point
    flow, Z, _ = T.camera_flow(h, w, 2, t, rot, *K)
    out = T.two_view(flow.astype(F), T.exact_model(h, w, t, rot, *K), *K)
    tl = np.linalg.norm(t)
    ok = out["cls"] == 1
    assert ok.all() and out["counts"][3] >= 0
    assert T.rotation_error_deg(out["pose"][:9], rot) <= 4 * ROT_BOUND_DEG and np.linalg.norm(out["pose"][9:12] - np.array(t) / tl) <= 4 * T_BOUND
    assert np.abs(out["depth"].astype(np.float64) * tl / Z - 1.0).max() <= DEPTH_BOUND
    # the wrong camera gives another answer: the intrinsics are used
    wrong = T.two_view(flow.astype(F), T.exact_model(h, w, t, rot, *K))
    assert wrong["counts"][3] < 0 or T.rotation_error_deg(wrong["pose"][:9], rot) > 1e-3
    # steps: the grid pixels alone vote, every pixel is classified
    for step in (3, 64):
        o = T.two_view(flow.astype(F), T.exact_model(h, w, t, rot, *K), *K, step=step)
        assert o["counts"][0] == len(range(0, h, step)) * len(range(0, w, step)) == o["counts"][1] and o["counts"][4] == h * w
        assert o["pose"].tobytes() == out["pose"].tobytes() and o["depth"].tobytes() == out["depth"].tobytes()


def test_the_decomposition_is_the_singular_value_decomposition():
    """The Jacobi chain against np.linalg, which is no part of it."""
    rng = np.random.RandomState(3)
    for _ in range(20):
        M = rng.standard_normal((3, 3))
        S = M.T @ M
        lam, V = T.jacobi([list(r) for r in S])
        V = np.array(V)
        assert np.allclose(V.T @ V, np.eye(3), atol=1e-14) and np.allclose(V @ np.diag(lam) @ V.T, S, atol=1e-13)
        assert np.allclose(sorted(lam), np.linalg.eigvalsh(S), atol=1e-13)
    h, w, t, rot = E.SCENES["mixed"]
    dec = T.decompose(T.exact_model(h, w, t, rot), h, w, 160.0, 160.0, 79.5, 23.5)
    for R in (dec["Ra"], dec["Rb"]):
        R = np.array(R).reshape(3, 3)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
    assert abs(np.linalg.norm(dec["t"]) - 1.0) < 1e-15 and dec["sigma"][0] == 1.0 and abs(dec["sigma"][1] - 1.0) < 1e-6 and dec["sigma"][2] < 1e-7
    # an exactly diagonal E^T E: every pair is skipped, and equal eigenvalues keep their order
    lam, V = T.jacobi([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 5.0]])
    assert lam == [2.0, 2.0, 5.0] and V == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    # an off-diagonal so small that the quotient overflows: the identity rotation, and no exception
    lam, V = T.jacobi([[1e300, 1e-300, 0.0], [1e-300, -1e300, 0.0], [0.0, 0.0, 1.0]])
    assert lam == [1e300, -1e300, 1.0] and V == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def check_no_pose(**mut):
    h, w = 33, 65
    scene = E.scene("mixed")[0][:h, :w].copy()
    still = np.zeros((h, w, 3), F)
    still[..., 2] = 1
    rank1 = np.outer([1, 0.5, -0.25], [0.5, 1, 0.125]).astype(F).reshape(-1)
    fitted = E.fit(still, n_hyp=8, lo_rounds=0)["model"]
    assert not fitted.any(), "a still camera's flow has no fundamental matrix"
    for what, flow, model in (("a zero F^", scene, np.zeros(9, F)), ("the identity as F^", still, np.eye(3, dtype=F).reshape(-1)),
                              ("an F^ of rank 1", scene, rank1), ("a still camera's flow", still, fitted)):
        out = T.two_view(flow, model, **mut)
        assert out["pose"].tolist() == [0.0] * 15 + [-1.0] and out["counts"] == [h * w, 0, 0, -1, 0, 0, h * w, 0], what
        assert (out["cls"] == 3).all() and not out["depth"].any() and np.isposinf(out["err"]).all(), what
    holes = scene.copy()
    holes[::2, :, 2] = 0
    holes[1, :, 0] = np.nan
    out = T.two_view(holes, np.zeros(9, F), **mut)
    assert (out["cls"][::2] == 0).all() and (out["err"][::2] == -1).all() and (out["cls"][1] == 0).all() and (out["cls"][3] == 3).all()


def test_inputs_without_a_pose():
    check_no_pose()


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_each_mutation_fails_a_check(mutation):
    failed = []
    for check in (check_candidates, check_object_against_the_epipolar_direction, check_accuracy, check_no_pose):
        try:
            check(**{mutation: True})
        except AssertionError:
            failed.append(check.__name__)
    assert failed, "the mutation %s passes every check" % mutation
    want = {"w_twice": "check_candidates", "vote_z1_only": "check_candidates", "tie_larger": "check_object_against_the_epipolar_direction",
            "den32": "check_accuracy", "u3_from_E": "check_candidates"}[mutation]
    assert want in failed, failed


def test_rigid_depth_is_the_scene_of_rigid_flow():
    synth = pkg("synth")
    H, W, seed, t, rot = 37, 53, 5, (0.3, -0.1, 0.6), (0.004, -0.006, 0.003)
    Z, (fx, fy, cx, cy) = synth.rigid_depth(H, W, seed)
    assert Z.shape == (H, W) and Z.dtype == np.float64 and (fx, fy, cx, cy) == (53.0, 53.0, 26.0, 18.0) and 4.5 <= Z.min() and Z.max() <= 12.5
    flow, mask = synth.rigid_flow(H, W, seed, t, rot)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = np.stack([(xx - cx) / fx * Z, (yy - cy) / fy * Z, Z], axis=-1)
    Y = X @ E.rotation(rot).T + np.asarray(t)
    rebuilt = np.stack([fx * Y[..., 0] / Y[..., 2] + cx - xx, fy * Y[..., 1] / Y[..., 2] + cy - yy, np.ones((H, W))], axis=-1)
    assert rebuilt.tobytes() == flow.tobytes() and not mask.any()
    assert not np.array_equal(Z, synth.rigid_depth(H, W, seed + 1)[0])
    # and the restatement finds that depth in that flow
    out = T.two_view(flow.astype(F), T.exact_model(H, W, t, rot))
    assert np.abs(out["depth"].astype(np.float64) * np.linalg.norm(t) / Z - 1.0).max() <= DEPTH_BOUND and (out["cls"] == 1).all()
