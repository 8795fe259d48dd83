"""The numpy definitions of dflow_prior_proposals and dflow_flow_advance (tests/prior_ref.py) against hand-worked cases (CPU
only).  The GPU tests compare the device with these definitions; these tests pin the definitions themselves."""
import numpy as np
import pytest

import prior_ref as R

FILL_LABEL, FILL_COST = 0xFFFFFFFF, np.float32(1000.0)


def blank_state(H, W, LP):
    """Every pixel holds the one label (0,0) at cost 0.5; descr1 is zero and descr2[y,x] = [0.25 x + y, 0, ...], so the cost
    of a label with target (ty,tx) is 0.25 tx + ty."""
    packed = np.full((H, W, LP), FILL_LABEL, np.uint32)
    lcosts = np.full((H, W, LP), FILL_COST, np.float32)
    packed[..., 0] = R.pack(0, 0)
    lcosts[..., 0] = 0.5
    nprop = np.ones((H, W), np.int64)
    best = np.zeros((H, W), np.int64)
    d1 = np.zeros((H, W, 68), np.float32)
    d2 = np.zeros((H, W, 68), np.float32)
    d2[..., 0] = 0.25 * np.arange(W)[None, :] + np.arange(H)[:, None]
    return packed, lcosts, nprop, best, d1, d2


def test_hand_worked_3x4_frame():
    H, W, LP, L, tphi = 3, 4, 16, 3, 2.5
    packed, lcosts, nprop, best, d1, d2 = blank_state(H, W, LP)
    # pixel (0,0) is full and does not hold (0,1); pixel (1,1) holds (0,1) already, at slot 1
    packed[0, 0, 1:3] = (R.pack(1, 1), R.pack(0, 2)); lcosts[0, 0, 1:3] = (0.75, 1.0); nprop[0, 0] = 3
    packed[1, 1, 1] = R.pack(0, 1); lcosts[1, 1, 1] = 0.125; nprop[1, 1] = 2
    prior = np.zeros((H, W, 2), np.float32)
    prior[..., 1] = 1.0                                   # [dy,dx] = (0,+1) everywhere ...
    prior[2, 3] = np.nan                                  # ... but here
    counts = R.prior_proposals(packed, lcosts, nprop, best, d1, d2, prior, 0, R.SEED_LABELS, L, tphi)
    # the last column points outside the frame (its last pixel is not finite either): 3 skipped; (0,0) is full; (1,1) found
    assert counts == [7, 1, 1, 3]
    assert nprop.tolist() == [[3, 2, 2, 1], [2, 2, 2, 1], [2, 2, 2, 1]]
    assert best.tolist() == [[0, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]]
    lab01 = R.pack(0, 1)
    assert lab01 == 0x00010000
    exp_slot1 = [[R.pack(1, 1), lab01, lab01, FILL_LABEL], [lab01, lab01, lab01, FILL_LABEL], [lab01, lab01, lab01, FILL_LABEL]]
    assert packed[..., 1].tolist() == exp_slot1
    # cost = min(tphi, 0.25 (x+1) + y); (2,1) gives exactly tphi, (2,2) is truncated to it
    exp_cost1 = [[0.75, 0.5, 0.75, 1000.0], [1.25, 0.125, 1.75, 1000.0], [2.25, 2.5, 2.5, 1000.0]]
    assert lcosts[..., 1].tolist() == exp_cost1
    assert (packed[..., 0] == 0).all() and (lcosts[..., 0] == 0.5).all()
    assert packed[0, 0, 2] == R.pack(0, 2) and (packed[..., 3:] == FILL_LABEL).all() and (lcosts[..., 3:] == FILL_COST).all()
    assert (np.delete(packed[..., 2].ravel(), 0) == FILL_LABEL).all()
    # a second identical call finds what the first appended and changes nothing
    before = [a.copy() for a in (packed, lcosts, nprop, best)]
    assert R.prior_proposals(packed, lcosts, nprop, best, d1, d2, prior, 0, R.SEED_LABELS, L, tphi) == [0, 8, 1, 3]
    for a, b in zip(before, (packed, lcosts, nprop, best)):
        assert a.tobytes() == b.tobytes()


def test_constant_field_appends_one_label_and_seeding_is_optional():
    H, W, LP, L = 5, 6, 16, 8
    packed, lcosts, nprop, best, d1, d2 = blank_state(H, W, LP)
    prior = np.zeros((H, W, 3), np.float32)
    prior[..., 0], prior[..., 1], prior[..., 2] = 1.0, -1.0, 1.0          # U = dx = +1, V = dy = -1, valid
    counts = R.prior_proposals(packed, lcosts, nprop, best, d1, d2, prior, 1, 0, L, 2.5)
    assert sum(counts) == H * W * 5
    inside = (np.arange(H)[:, None] >= 1) & (np.arange(W)[None, :] <= W - 2)       # the target is inside the frame
    assert (nprop == 1 + inside).all() and counts[0] == inside.sum() == 20 and counts[2] == 0
    assert (packed[..., 1][inside] == R.pack(-1, 1)).all() and (best == 0).all(), "no seed flag: bestlabels untouched"
    # per pixel with an inside target: its own candidate appended, every in-frame neighbour's found
    srcs_in_frame = sum(0 <= y + oy < H and 0 <= x + ox < W for y in range(H) for x in range(W) if inside[y, x]
                        for oy, ox in R.OFFSETS)
    assert counts[1] == srcs_in_frame - 20 and counts[3] == H * W * 5 - srcs_in_frame


@pytest.mark.parametrize("stride", [0, 1, 3])
@pytest.mark.parametrize("layout", ["dydx", "uvv"])
def test_counter_identities_on_random_fields(stride, layout):
    rng = np.random.default_rng(5 + stride)
    H, W, LP, L = 7, 9, 16, 4
    packed, lcosts, nprop, best, d1, d2 = blank_state(H, W, LP)
    d1[:] = rng.standard_normal(d1.shape).astype(np.float32) * 0.01
    prior = rng.integers(-3, 4, (H, W, 2)).astype(np.float32) + rng.choice([0.0, 0.5], (H, W, 2)).astype(np.float32)
    if layout == "uvv":
        prior = np.concatenate([prior[..., ::-1], (rng.random((H, W, 1)) > 0.3).astype(np.float32)], axis=-1)
    n_before = nprop.copy()
    counts = R.prior_proposals(packed, lcosts, nprop, best, d1, d2, prior, stride, R.SEED_LABELS, L, 2.5)
    assert sum(counts) == H * W * (5 if stride else 1) and all(c >= 0 for c in counts)
    assert (nprop - n_before).sum() == counts[0] and nprop.max() <= L
    used = np.arange(LP)[None, None, :] < nprop[..., None]
    assert (packed[~used] == FILL_LABEL).all() and (lcosts[~used] == FILL_COST).all()
    assert (lcosts[used] >= 0).all() and (lcosts[used] <= np.float32(2.5)).all()
    assert ((best >= 0) & (best < nprop)).all()
    for y in range(H):                                     # no label twice in a row
        for x in range(W):
            row = packed[y, x, :nprop[y, x]].tolist()
            assert len(set(row)) == len(row)


def test_rounding_table():
    table = [(0.5, 0), (-0.5, 0), (1.5, 2), (2.5, 2), (-2.5, -2), (32767.4, 32767), (-32767.4, -32767), (32767.6, None),
             (32767.5, None), (32768.0, None), (-32768.0, None), (1e9, None), (np.nan, None), (np.inf, None), (-np.inf, None)]
    for value, want in table:
        f = np.zeros((1, 1, 2), np.float32)
        f[0, 0, 0] = value
        got = R.usable_vector(f, R.DYDX, 0, 0)
        assert got == (None if want is None else (want, 0)), (value, got)
        g = np.array([[[value, 0.0, 1.0]]], np.float32)    # the same as U
        got = R.usable_vector(g, R.UVV, 0, 0)
        assert got == (None if want is None else (0, want)), (value, got)
    for valid, ok in ((0.0, False), (0.5, False), (0.50001, True), (1.0, True), (np.nan, False)):
        g = np.array([[[2.0, 3.0, valid]]], np.float32)
        assert (R.usable_vector(g, R.UVV, 0, 0) == (3, 2)) == ok, valid
    # an unusable vector is a skipped candidate
    packed, lcosts, nprop, best, d1, d2 = blank_state(8, 8, 16)
    prior = np.zeros((8, 8, 2), np.float32)
    prior[3, 3, 1] = 32767.6
    assert R.prior_proposals(packed, lcosts, nprop, best, d1, d2, prior, 0, 0, 4, 2.5) == [0, 63, 0, 1]


def test_l1_cost_order_is_numpys_pairwise_sum():
    rng = np.random.default_rng(0)
    for _ in range(50):
        a = (rng.standard_normal(68) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
        b = rng.standard_normal(68).astype(np.float32)
        assert R.l1_cost(a, b).tobytes() == np.sum(np.absolute(a - b)).tobytes()
    a = np.zeros(68, np.float32)
    a[5] = np.nan
    assert np.isnan(R.l1_cost(a, np.zeros(68, np.float32)))


def test_flow_advance_all_sources_claim_one_pixel():
    H, W = 4, 5
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flow = np.stack([2 - yy, 3 - xx], axis=-1).astype(np.float32)        # everybody points at (2,3)
    out, counts = R.flow_advance(flow)
    assert counts == [1, H * W - 1, 0]
    exp = np.zeros((H, W, 3), np.float32)
    exp[2, 3] = (3.0, 2.0, 1.0)                                           # the winner is raster index 0: [dx, dy, 1] of pixel (0,0)
    assert out.tobytes() == exp.tobytes()
    out, counts = R.flow_advance(flow, R.NEGATE)
    exp[2, 3] = (-3.0, -2.0, 1.0)
    assert out.tobytes() == exp.tobytes() and counts == [1, H * W - 1, 0]


def test_flow_advance_negate_of_zero_flow_is_plus_zero():
    flow = np.zeros((3, 3, 2), np.float32)
    flow[1, 1] = (-0.0, -0.4)
    out, counts = R.flow_advance(flow, R.NEGATE)
    exp = np.zeros((3, 3, 3), np.float32)
    exp[..., 2] = 1.0
    assert out.view(np.uint32).tolist() == exp.view(np.uint32).tolist(), "+0.0 bits everywhere"
    assert counts == [9, 0, 0]


def test_flow_advance_holes_collisions_and_counts():
    flow = np.zeros((2, 3, 3), np.float32)
    flow[..., 2] = 1.0
    flow[0, 0, :2] = (1.0, 0.0)       # (0,0) -> (0,1), collides with (0,1) staying put and wins (smaller index)
    flow[0, 2, :2] = (1.0, 0.0)       # leaves the frame
    flow[1, 0, 2] = 0.5               # not valid
    flow[1, 1, :2] = (0.5, -1.5)      # rounds to (dx 0, dy -2): leaves the frame
    flow[1, 2, :2] = (-1.5, -0.5)     # rounds to (dx -2, dy 0): lands on (1,0)
    out, counts = R.flow_advance(flow)
    assert counts == [2, 1, 3]
    exp = np.zeros((2, 3, 3), np.float32)
    exp[0, 1] = (1.0, 0.0, 1.0)
    exp[1, 0] = (-2.0, 0.0, 1.0)
    assert out.tobytes() == exp.tobytes()
