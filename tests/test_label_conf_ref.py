"""tests/label_conf_ref.py, the numpy restatement of dflow_label_confidence and dflow_flow_gate, on cases worked by hand, and the
random states of tests/test_gpu_label_conf.py: that they really hold every class the GPU test means to compare (CPU only)."""
import numpy as np
import pytest

from label_conf_ref import COMBOS, DATA, LOCAL, SHAPES, THRESH, flow_gate_ref, gpu_state, label_conf_ref

INF = np.float32(np.inf)


def one_pixel(label, nprop=4):
    """1 x 1, no neighbours, lamda 2: slot 0 (0,0) cost 1, slot 1 its duplicate at cost 0.5, slots 2 (2,0) and 3 (0,3) at cost 0.75:
    e = [2, 1, 1.5, 1.5]."""
    flows = np.array([[[[0, 0], [0, 0], [2, 0], [0, 3]]]])
    costs = np.array([[[1.0, 0.5, 0.75, 0.75]]], np.float32)
    return lambda **kw: label_conf_ref(flows, costs, np.array([[nprop]]), np.array([[label]]), tpsi=8, lamda=2.0, **kw)


def test_one_pixel_ties_duplicates_and_an_empty_set():
    run = one_pixel(0)
    r = run(min_sep=0, thresh=-1.0)
    assert np.array_equal(r["energy"][0, 0], [2.0, 1.0, 1.5, 1.5])
    # the duplicate (distance 0) does not compete although it is the cheapest; slots 2 and 3 tie, the smaller index wins
    assert r["alt"][0, 0] == 2 and r["margin"][0, 0] == np.float32(-0.5) and r["margin"].dtype == np.float32
    assert r["counts"] == [1, 0, 0, 1, 0, 1] and np.array_equal(r["sparse"][0, 0], [0, 0, 1])
    assert run(min_sep=0, thresh=-0.25)["counts"] == [1, 0, 0, 1, 0, 0]
    # min_sep 2 excludes slot 2 (distance 2), min_sep 3 everything: no alternative
    r = run(min_sep=2)
    assert r["alt"][0, 0] == 3 and r["margin"][0, 0] == np.float32(-0.5)
    r = run(min_sep=3, thresh=1e30)
    assert r["alt"][0, 0] == -1 and r["margin"][0, 0] == INF and r["counts"] == [1, 0, 1, 0, 0, 1]
    # a slot at or beyond nprop is no alternative: with nprop 3, slot 3 is gone
    r = one_pixel(0, nprop=3)(min_sep=2)
    assert r["alt"][0, 0] == -1 and r["margin"][0, 0] == INF
    # chosen slot 1: the margin to slot 2 is 1.5 - 1 = 0.5
    r = one_pixel(1)(min_sep=1, thresh=0.5)
    assert r["alt"][0, 0] == 2 and r["margin"][0, 0] == np.float32(0.5) and r["counts"] == [1, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("label", (-1, 4, 1000))
def test_one_pixel_with_a_bad_label(label):
    r = one_pixel(label)(min_sep=0, thresh=-np.inf)
    assert r["alt"][0, 0] == -1 and r["margin"][0, 0] == -INF
    assert r["counts"] == [0, 1, 0, 0, 0, 0] and not r["sparse"].any()


def two_pixels(label1):
    """1 x 2, tpsi 2, lamda 1.  Pixel 0: slots (0,0) cost 1 and (0,5) cost 0.25, label 0.  Pixel 1: slots (0,5) cost 2 and (0,1) cost 1."""
    flows = np.array([[[[0, 0], [0, 5]], [[0, 5], [0, 1]]]])
    costs = np.array([[[1.0, 0.25], [2.0, 1.0]]], np.float32)
    return lambda **kw: label_conf_ref(flows, costs, np.array([[2, 2]]), np.array([[0, label1]]), tpsi=2, lamda=1.0, **kw)


def test_two_pixels_local_against_data():
    r = two_pixels(0)(mode=LOCAL, min_sep=1)
    # pixel 0 against g = (0,5): s = [min(2,5), 0] = [2, 0], e = [3, 0.25]; pixel 1 against g = (0,0): s = [2, 1], e = [4, 2]
    assert np.array_equal(r["energy"][0], [[3.0, 0.25], [4.0, 2.0]])
    assert np.array_equal(r["margin"][0], np.float32([-2.75, -2.0])) and np.array_equal(r["alt"][0], [1, 1])
    r = two_pixels(0)(mode=DATA, min_sep=1)
    assert np.array_equal(r["energy"][0], [[1.0, 0.25], [2.0, 1.0]])
    assert np.array_equal(r["margin"][0], np.float32([-0.75, -1.0]))


def test_two_pixels_a_bad_label_at_the_neighbour_adds_nothing():
    r = two_pixels(-1)(mode=LOCAL, min_sep=1, thresh=-1.0)
    assert np.array_equal(r["energy"][0, 0], [1.0, 0.25])                  # s = 0: LOCAL equals DATA here
    assert r["margin"][0, 0] == np.float32(-0.75) and r["margin"][0, 1] == -INF and np.array_equal(r["alt"][0], [1, -1])
    assert r["counts"] == [1, 1, 0, 1, 0, 1]
    assert np.array_equal(r["sparse"][0], [[0, 0, 1], [0, 0, 0]])


def test_three_by_three_centre_with_four_neighbours():
    """tpsi 3, lamda 2.  The centre has slots (0,0), (1,1), (1,1), all cost 0.5, label 0; its neighbours chose up (0,0), left (1,1),
    right (1,1), down (3,2); every other pixel has the one slot it chose."""
    flows = np.zeros((3, 3, 3, 2), np.int64)
    flows[0, 1, 0], flows[1, 0, 0], flows[1, 2, 0], flows[2, 1, 0] = (0, 0), (1, 1), (1, 1), (3, 2)
    flows[1, 1] = [(0, 0), (1, 1), (1, 1)]
    costs = np.full((3, 3, 3), 0.5, np.float32)
    nprop = np.ones((3, 3), np.int64)
    nprop[1, 1] = 3
    r = label_conf_ref(flows, costs, nprop, np.zeros((3, 3), np.int64), tpsi=3, lamda=2.0, min_sep=1, thresh=-1.0)
    # s_0 = 0 + 2 + 2 + min(3, 5) = 7, s_1 = s_2 = 2 + 0 + 0 + min(3, 3) = 5; e = [8, 6, 6]: slots 1 and 2 tie
    assert np.array_equal(r["energy"][1, 1], [8.0, 6.0, 6.0])
    assert r["alt"][1, 1] == 1 and r["margin"][1, 1] == np.float32(-2.0)
    others = np.ones((3, 3), bool)
    others[1, 1] = False
    assert (r["margin"][others] == INF).all() and (r["alt"][others] == -1).all()
    assert r["counts"] == [9, 0, 8, 1, 0, 8]
    assert np.array_equal(r["sparse"][1, 1], [0, 0, 0]) and np.array_equal(r["sparse"][2, 1], [2, 3, 1]) and np.array_equal(r["sparse"][1, 2], [1, 1, 1])
    # the data cost alone: all three slots cost the same, the margin is 0
    r = label_conf_ref(flows, costs, nprop, np.zeros((3, 3), np.int64), tpsi=3, lamda=2.0, mode=DATA, min_sep=1, thresh=0.0)
    assert r["alt"][1, 1] == 1 and r["margin"][1, 1] == 0 and r["counts"] == [9, 0, 8, 0, 1, 9]


def test_the_margin_is_rounded_once_from_the_double_difference():
    flows = np.array([[[[0, 0], [0, 9]]]])
    costs = np.array([[[0.1, 0.7]]], np.float32)
    r = label_conf_ref(flows, costs, np.array([[2]]), np.array([[0]]), tpsi=8, lamda=0.05, min_sep=1)
    e = [0.05 * float(np.float32(0.1)) + 0.0, 0.05 * float(np.float32(0.7)) + 0.0]
    assert r["margin"][0, 0] == np.float32(e[1] - e[0])


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_the_random_states_hold_every_class(shape):
    """A condition on the inputs of the GPU test: in the states built for them, no-alternative, margin < 0, margin == 0 (where the
    energies are integers), not-labelled and both sides of the threshold each occur."""
    seen_zero = False
    for lp, maxnprop, tpsi, min_sep, mode, lamda, quantised in COMBOS:
        s = gpu_state(shape, lp, maxnprop, quantised)
        r = s.ref(tpsi, lamda, mode=mode, min_sep=min_sep, thresh=THRESH)
        labelled, not_labelled, no_alt, negative, zero, kept = r["counts"]
        what = (shape, lp, tpsi, min_sep, mode, lamda)
        assert labelled + not_labelled == shape[0] * shape[1], what
        assert not_labelled > 0 and negative > 0 and 0 < kept < labelled, what
        assert (s.labels == -1).any() and (s.labels >= s.nprop).any() and (s.labels >= s.label_pitch).any(), what
        if min_sep == 3 or lp == 16:
            assert no_alt > 0, what
        if quantised or lamda == 0.0:
            # integer energies: ties with the chosen label occur; in a frame of 70 pixels not under every combination
            assert zero > 0 or shape[0] * shape[1] < 2000, what
            seen_zero = seen_zero or zero > 0
        assert np.isfinite(r["margin"]).any() and (r["margin"] == INF).any() == (no_alt > 0)
        assert (r["alt"] < s.nprop)[r["alt"] >= 0].all(), "slots at or beyond nprop are never the alternative"
    assert seen_zero, shape


def test_flow_gate_ref_on_a_written_out_field():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    uvv = np.array([[[1, 2, 1], [3, 4, 1], [5, 6, 0], [nan, 1, 1], [7, 8, 1], [9, 1, 1], [2, 2, 1], [-0.0, 3, 1]]], np.float32)
    score = np.array([[0.5, 2.0, 1.0, 1.0, nan, -inf, 1.0, 0.25]], np.float32)
    out, counts = flow_gate_ref(uvv, score, lo=0.25, hi=1.0)
    keep = [1, 0, 0, 0, 0, 0, 1, 1]                  # above hi; invalid; NaN vector; NaN score; below lo; at hi; at lo
    assert counts == [6, 3]
    for i, k in enumerate(keep):
        assert np.array_equal(out[0, i].view(np.uint32), (np.float32([uvv[0, i, 0], uvv[0, i, 1], 1]) if k else np.zeros(3, np.float32)).view(np.uint32))
    dydx = np.array([[[2, 1], [4, 3]]], np.float32)
    out, counts = flow_gate_ref(dydx, np.array([[inf, -inf]], np.float32))
    assert counts == [2, 2] and np.array_equal(out[0], [[1, 2, 1], [3, 4, 1]])
