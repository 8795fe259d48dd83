"""tests/track_ref.py, the numpy restatement of dflow_track_advance / _seed / _flow, against what the definitions promise: every
class of the advance is populated by the coverage case, an analytic rotation and a translation are followed, the seed's raster
order, mask, partial cells and cap, and the smallest index winning a pixel of the flow (CPU only)."""
import numpy as np
import pytest

import track_ref as R

F = np.float32


@pytest.fixture(scope="module")
def coverage():
    h, w, fwd, bwd, pos, state = R.coverage_case()
    return h, w, fwd, bwd, pos, state, R.advance(h, w, fwd, bwd, pos, state)


def test_the_coverage_case_populates_every_class(coverage):
    h, w, fwd, bwd, pos, state, (pos_out, state_out, err, counts) = coverage
    print("advance counts", counts.tolist())
    assert counts.sum() == len(state) and (counts >= 20).all(), counts          # a condition on the input: the seed is fixed for it
    assert (state == R.FREE).sum() == 1
    was_live = state == R.LIVE
    # a slot that was not live is copied through, position bits included
    assert (state_out[~was_live] == state[~was_live]).all() and pos_out[~was_live].tobytes() == pos[~was_live].tobytes()
    # a track that ends keeps its last position; one that lives moved to an inside position
    ended = was_live & (state_out != R.LIVE)
    assert pos_out[ended].tobytes() == pos[ended].tobytes()
    live = state_out == R.LIVE
    assert R.inside(pos_out[live, 0], pos_out[live, 1], h, w).all()
    # the error is formed exactly where the backward sample was good
    formed = was_live & np.isin(state_out, (R.LIVE, R.INCONSISTENT))
    assert (err[formed] >= 0).all() and (err[~formed] == -1).all()
    # the odd positions at the end: NaN, +-Inf, -1, 1e9 and the first float32 beyond the last pixel are LEFT, -0.0 is inside
    assert (state_out[1000:1008] == R.LEFT).all() and (state_out[1010:1012] == R.LEFT).all()
    assert R.inside(pos[1008:1010, 0], pos[1008:1010, 1], h, w).all() and not R.inside(pos[1000:1008, 0], pos[1000:1008, 1], h, w).any()
    # without the backward field nothing is NOBACK or INCONSISTENT, and the same tracks leave or meet no flow
    p2, s2, e2, c2 = R.advance(h, w, fwd, None, pos, state)
    assert c2[3] == 0 and c2[4] == 0 and (e2 == -1).all() and c2[1] == counts[1] and c2[2] == counts[2]
    assert c2[0] == counts[0] + counts[3] + counts[4]
    # the layout does not matter where the same vectors are good
    p3, s3, e3, c3 = R.advance(h, w, R.to_dydx(fwd), R.to_dydx(bwd), pos, state)
    assert p3.tobytes() == pos_out.tobytes() and (s3 == state_out).all() and e3.tobytes() == err.tobytes()


def test_integer_positions_read_one_corner():
    """A track on a pixel whose neighbours are all invalid still advances: corners of weight zero are not looked at."""
    h, w = 9, 11
    fwd = np.zeros((h, w, 3), F)
    fwd[4, 5] = (1.25, -0.5, 1)
    fwd[4, 6] = (2.0, 2.0, 1)
    pos = np.array([[5, 4], [5.5, 4], [5, 4.5]], F)
    p, s, e, c = R.advance(h, w, fwd, None, pos, np.full(3, R.LIVE, np.int32))
    assert s.tolist() == [R.LIVE, R.LIVE, R.NOFLOW] and p[0].tolist() == [6.25, 3.5] and p[1].tolist() == [5.5 + 1.625, 4 + 0.75]


def test_rotation_is_followed_for_eight_frames():
    h = w = 65
    for angle in (0.05, -0.05):
        fwd, bwd = R.rotation_field(h, w, angle), R.rotation_field(h, w, -angle)
        pos = R.grid_seeds(h, w, 4)
        state = np.full(len(pos), R.LIVE, np.int32)
        start = pos.astype(np.float64) - 32
        left_at = np.full(len(pos), -1)
        worst = 0.0
        for t in range(1, 9):
            pos, state, err, counts = R.advance(h, w, fwd, bwd, pos, state)
            c, s = np.cos(angle * t), np.sin(angle * t)
            exact = np.stack([c * start[:, 0] - s * start[:, 1], s * start[:, 0] + c * start[:, 1]], 1) + 32
            live = state == R.LIVE
            worst = max(worst, np.abs(pos[live] - exact[live]).max())
            out = (exact < 0).any(1) | (exact > 64).any(1)
            # a track leaves at the frame its analytic path leaves (no analytic position lies within the bound of the border)
            assert np.abs(np.minimum(exact, 64 - exact).min(1)[left_at < 0]).min() > 1e-3
            newly = (state == R.LEFT) & (left_at < 0)
            assert (newly == (out & (left_at < 0))).all(), t
            left_at[newly] = t
            assert set(np.unique(state)) <= {R.LIVE, R.LEFT}
        print("rotation %+.2f: worst %.3g px, %d left" % (angle, worst, (left_at > 0).sum()))
        # 8 steps of a few ulps at coordinate 64, where one ulp is 7.6e-6
        assert worst <= 1e-4
        assert (left_at > 0).sum() == 32


def test_translation_is_exact():
    h, w = 21, 33
    fwd = np.ones((h, w, 3), F)
    fwd[..., 0], fwd[..., 1] = 1.5, -0.75
    bwd = fwd.copy()
    bwd[..., :2] = -bwd[..., :2]
    pos = R.grid_seeds(h, w, 4)
    p, s = pos, np.full(len(pos), R.LIVE, np.int32)
    for t in range(1, 6):
        p, s, err, _ = R.advance(h, w, fwd, bwd, p, s)
        live = s == R.LIVE
        assert (p[live] == pos[live] + np.array([1.5 * t, -0.75 * t], F)).all() and (err[live] == 0).all()
    assert (s == R.LIVE).sum() > 20 and (s == R.LEFT).sum() > 10 and set(np.unique(s)) == {R.LIVE, R.LEFT}


def empty(cap):
    return np.zeros((cap, 2), F), np.zeros(cap, np.int32), np.zeros(cap, np.int32)


def test_seed_raster_order_partial_cells_and_large_steps():
    h, w = 7, 10
    pos, state, birth, n, counts = R.seed(h, w, 4, 3, None, *empty(10), 0)
    # gh = 2, gw = 3; the last cells are partial: their seed pixels are clamped into the frame
    assert n == 6 and counts.tolist() == [0, 6, 6, 0]
    assert pos[:6].tolist() == [[2, 2], [6, 2], [9, 2], [2, 6], [6, 6], [9, 6]]
    assert state[:6].tolist() == [R.LIVE] * 6 and state[6:].tolist() == [0] * 4 and birth[:6].tolist() == [3] * 6
    # step > h and step > w: one cell, its seed pixel the clamped centre
    pos, state, birth, n, counts = R.seed(h, w, 64, 0, None, *empty(4), 0)
    assert n == 1 and pos[0].tolist() == [9, 6] and counts.tolist() == [0, 1, 1, 0]
    assert R.scan_len(h, w, 64) == 1 + 1 + 1 and R.scan_len(1100, 1100, 1) == 1210000 + 1182 + 1


def test_seed_mask_cover_cap_and_n_out_of_range():
    h, w = 7, 10
    mask = np.ones((h, w), np.uint8)
    mask[2, 6] = 0                                   # the seed pixel of cell (0, 1)
    pos, state, birth = empty(8)
    pos[0], state[0] = (7.5, 2.5), R.LIVE            # covers cell (rint(2.5) = 2 -> 0, rint(7.5) = 8 -> 2): ties to even
    pos[1], state[1] = (1.0, 5.0), R.LEFT            # not live: covers nothing
    pos[2], state[2] = (np.nan, 5.0), R.LIVE         # not inside: covers nothing
    p, s, b, n, counts = R.seed(h, w, 4, 5, mask, pos, state, birth, 3)
    assert counts.tolist() == [1, 4, 4, 0] and n == 7
    assert p[3:7].tolist() == [[2, 2], [2, 6], [6, 6], [9, 6]] and b[3:7].tolist() == [5] * 4 and (p[:3].tobytes() == pos[:3].tobytes())
    # the live track beyond n is not seen: its cell is seeded again
    p, s, b, n, counts = R.seed(h, w, 4, 5, None, pos, state, birth, 0)
    assert counts.tolist() == [0, 6, 6, 0] and n == 6 and p[0].tolist() == [2, 2]
    # the cap is reached in the middle of a row: the rest is dropped, n stops at cap
    p, s, b, n, counts = R.seed(h, w, 4, 5, None, pos, state, birth, 4)
    assert counts.tolist() == [1, 5, 4, 1] and n == 8 and p[4:].tolist() == [[2, 2], [6, 2], [2, 6], [6, 6]]
    # *d_n out of range is clamped
    p, s, b, n, counts = R.seed(h, w, 4, 5, None, pos, state, birth, -7)
    assert n == 6 and counts.tolist() == [0, 6, 6, 0]
    p, s, b, n, counts = R.seed(h, w, 4, 5, None, pos, state, birth, 99)
    assert n == 8 and counts.tolist() == [1, 5, 0, 5] and p.tobytes() == pos.tobytes() and (s == state).all()


def test_flow_the_smallest_index_wins_a_shared_pixel():
    h, w = 6, 8
    pos_a = np.array([[2.4, 3.0], [1.6, 3.4], [2.0, 2.6], [7.0, 5.0], [np.nan, 1.0], [0.0, 0.0], [3.0, 3.0]], F)
    pos_b = pos_a + np.array([[1, 0.5]] * 7, F) * np.arange(1, 8, dtype=F)[:, None]
    state_a = np.array([R.LEFT, R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LIVE], np.int32)
    state_b = np.array([R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.LIVE, R.NOBACK, R.LIVE], np.int32)
    owner, out, counts = R.flow(h, w, pos_a, state_a, pos_b, state_b)
    # tracks 1 and 2 share pixel (3, 2): 1 wins; 0 and 5 are not live in both; 4 is not inside
    assert counts.tolist() == [3, 1, 3] and owner[3, 2] == 1 and owner[5, 7] == 3 and owner[3, 3] == 6
    assert (owner == R.NO_OWNER).sum() == h * w - 3
    assert out[3, 2].tolist() == [(pos_b[1, 0] - pos_a[1, 0]), (pos_b[1, 1] - pos_a[1, 1]), 1.0]
    assert (out[owner == R.NO_OWNER] == 0).all()
    # the other order of the snapshots: b's positions claim, and the vectors turn round
    owner2, out2, counts2 = R.flow(h, w, pos_b, state_b, pos_a, state_a)
    assert counts2.sum() == 7 and counts2[2] >= 3
    p = np.flatnonzero(owner2.ravel() != R.NO_OWNER)
    o = owner2.ravel()[p]
    assert (out2.reshape(-1, 3)[p, :2] == pos_a[o] - pos_b[o]).all()
