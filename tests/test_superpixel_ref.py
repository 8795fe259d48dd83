"""The numpy restatements of dflow_superpixels and dflow_segment_fit (tests/superpixel_ref.py) pinned by hand: cases whose answer
follows from the header's text without running anything, and the mutations of the restatement that each of them must notice
(CPU only)."""
import numpy as np
import pytest

import superpixel_ref as ref

F32 = np.float32


def test_uniform_image_the_labels_are_the_voronoi_cells_with_ties_to_the_smaller_k():
    h, w, S = 16, 24, 8
    img = np.full((h, w, 3), 77, np.uint8)
    gh, gw, K = ref.grid(h, w, S)
    assert (gh, gw, K) == (2, 3, 6)
    centres = [(gx * S + S // 2, gy * S + S // 2) for gy in range(gh) for gx in range(gw)]
    want = np.array([[min(range(K), key=lambda k: ((x - centres[k][0]) ** 2 + (y - centres[k][1]) ** 2, k)) for x in range(w)]
                     for y in range(h)], np.int32)
    assert want[0, 8] == 0 and want[8, 8] == 0 and want[8, 7] == 0 and want[8, 9] == 1, "the ties of column 8 and row 8 go to the smaller k"
    for m in (1, 10, 255):
        r = ref.superpixels(img, S, m, 1, 0)
        assert np.array_equal(r["slic"], want), m
        # Voronoi cells are connected, min_size 0 merges nothing and the cells appear in raster order: the numbers are the labels
        assert np.array_equal(r["label"], want) and list(r["counts"]) == [K, 0, K, 0, 0, K, int(np.bincount(want.ravel()).max()), 0]
        assert np.array_equal(r["centers"][:, 5], np.bincount(want.ravel(), minlength=K))
    # m = 0: every distance is zero and every pixel takes the smallest k of its neighbourhood
    r = ref.superpixels(img, S, 0, 1, 0)
    assert np.array_equal(r["slic"], np.array([[max(y // S - 1, 0) * gw + max(x // S - 1, 0) for x in range(w)] for y in range(h)]))
    assert not np.array_equal(ref.superpixels(img, S, 10, 1, 0, mutate="tie_larger")["slic"], want)


def two_colours():
    img = np.zeros((8, 16, 3), np.uint8)
    img[:, 5:] = 255
    img[3, 2, 0] = 2
    return img


def test_two_colours_the_boundary_lies_on_the_colour_edge_and_the_centres_are_rounded_means():
    img = two_colours()
    want = np.zeros((8, 16), np.int32)
    want[:, 5:] = 1                                    # column 5 is no cell border (S = 8)
    for iters in (1, 2, 5):
        r = ref.superpixels(img, 8, 0, iters, 0)
        assert np.array_equal(r["slic"], want) and np.array_equal(r["label"], want) and list(r["counts"][:6]) == [2, 0, 2, 0, 0, 2]
        # centre 0: 40 pixels, sum x = 8 * 10, sum y = 5 * 28, sum b = 2: (16 * 2 + 20) / 40 = 1; centre 1: 88 pixels, sum x = 8 * 110
        assert r["centers"].tolist() == [[32, 56, 1, 0, 0, 40, 0, 0], [160, 56, 4080, 4080, 4080, 88, 0, 0]]
    assert ref.superpixels(img, 8, 0, 1, 0, mutate="floor_div")["centers"][0, 2] == 0


CHAIN = np.array([[0, 0, 1, 1, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1, 1, 1, 1],
                  [1, 2, 3, 4, 1, 1, 1, 1],
                  [1, 2, 3, 4, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1, 1, 1, 1],
                  [5, 5, 5, 5, 6, 8, 8, 8]], np.int32)
CHAIN_WANT = np.array([[0, 0] + [1] * 6] + [[1] * 8] * 4 + [[2, 2, 2, 2, 2, 3, 3, 3]], np.int32)


def test_a_three_link_chain_and_a_small_component_that_holds_pixel_0():
    # min_size 3: the pair at pixel 0 is small and stays (no target); 4 -> 3 -> 2 -> the large 1 is three links; the single 6 joins
    # the 5 to its left, which is not small; the three 8 are not small
    out, tail = ref.merge_and_number(CHAIN, 3)
    assert np.array_equal(out, CHAIN_WANT)
    assert tail == [8, 5, 7, 4, 38]
    # min_size 0 and 1 merge nothing: eight segments in the order of their first pixels
    for ms in (0, 1):
        out, tail = ref.merge_and_number(CHAIN, ms)
        assert tail == [8, 0, 0, 8, 32]
        assert [int(out[y, x]) for y, x in ((0, 0), (0, 2), (2, 1), (2, 2), (2, 3), (5, 0), (5, 4), (5, 5))] == list(range(8))
    # everything small: one segment, the one that holds pixel 0
    out, tail = ref.merge_and_number(CHAIN, 1 << 26)
    assert not out.any() and tail == [8, 8, 46, 1, 48]
    # to the right, the single 6 would join the three 8
    out, _ = ref.merge_and_number(CHAIN, 3, mutate="target_right_down")
    assert out[5, 4] == 3 and not np.array_equal(out, CHAIN_WANT)


# ------------------------------------------------------------------------------------------------------------- the fit
LABELS = np.array([[0, 0, 2, 2, 2, -1],
                   [0, 5, 5, 1, 1, 9],
                   [4, 4, 4, 1, 3, 3],
                   [4, 4, 4, 4, 4, 1]], np.int32)
N_SEG = 6
MODEL_A = [0.5, 0.25, 1.0, -0.25, 0.5, -2.0]
MODEL_B = [-0.125, 0.0, 1.5, 0.0, 0.75, 0.015625]


def hand_flow():
    """(4,6,3) [U,V,valid]: segment 0 (3 pixels) and 1 (4 pixels) carry affine flows that are exact on the 1/64 grid, 2 is a row of
    three, 3 has two pixels, 4 no valid vector, 5 a NaN and a vector just outside the range; the two pixels whose label is out
    of range carry ordinary vectors."""
    f = np.zeros((4, 6, 3), F32)
    for (x, y), m in [((0, 0), MODEL_A), ((1, 0), MODEL_A), ((0, 1), MODEL_A), ((3, 1), MODEL_B), ((4, 1), MODEL_B), ((3, 2), MODEL_B),
                      ((5, 3), MODEL_B)]:
        f[y, x] = [m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5], 1]
    f[0, 2], f[0, 3], f[0, 4] = [0, 0, 1], [0, 0, 1], [4.5, 0, 1]
    f[2, 4], f[2, 5] = [1, 0.5, 1], [2, 0.5, 1]
    f[2, 0] = [3, 3, 0]                                # segment 4: not valid
    f[1, 1], f[1, 2] = [np.nan, 0, 1], [32768.5, 0, 1]
    f[0, 5], f[1, 5] = [1, 1, 1], [2, 2, 1]
    return f


def test_exact_affine_segments_the_translation_fallback_and_no_model():
    f = hand_flow()
    assert np.array_equal(f[..., :2] * 64, np.rint(f[..., :2] * 64), equal_nan=True)
    r = ref.segment_fit(f, LABELS, N_SEG, 1.0, 1)
    want = np.array([MODEL_A, MODEL_B, [0, 0, 1.5, 0, 0, 0], [0, 0, 1.5, 0, 0, 0.5], [0] * 6, [0] * 6], F32)
    assert r["models"].dtype == F32 and np.array_equal(r["models"], want)
    assert r["seg_counts"].tolist() == [[3, 3, 3, 2], [4, 4, 4, 2], [3, 3, 0, 1], [2, 2, 2, 1], [8, 0, 0, 0], [2, 0, 0, 0]]
    assert r["counts"].tolist() == [12, 9, 4, 2, 2, 2, 1, 0]
    cls = np.array([[1, 1, 2, 2, 2, 0], [1, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 1]], np.uint8)
    assert np.array_equal(r["cls"], cls)
    has = np.isin(LABELS, (0, 1, 2, 3))
    assert np.array_equal(r["out"][..., 2], has.astype(F32)) and not r["out"][~has].any()
    assert np.array_equal(r["out"][has & (LABELS < 2)][:, :2], f[has & (LABELS < 2)][:, :2]), "an exact model reproduces its vectors"
    assert np.array_equal(r["out"][0, 2:5, 0], [1.5, 1.5, 1.5]) and np.array_equal(r["out"][2, 4:, :2], [[1.5, 0.5], [1.5, 0.5]])
    # the other layout: [dy,dx], every vector valid, so segment 4's stand-ins become NaN
    g = np.ascontiguousarray(f[..., [1, 0]])
    g[f[..., 2] == 0] = np.nan
    r2 = ref.segment_fit(g, LABELS, N_SEG, 1.0, 1)
    assert all(np.array_equal(r[k], r2[k]) for k in r)


def test_the_rounds_halve_the_threshold_down_to_thresh_and_an_empty_round_keeps_the_model():
    f = hand_flow()
    # segment 2: U = 0, 0, 4.5 in a row, so every solve is the translation.  Round 0: 1.5.  R = 2: T_1 = 1, the residuals are 1.5,
    # 1.5 and 3: nothing agrees and the model of round 0 stays.  R = 3: T_1 = 2 keeps the two zeros, whose mean is 0, and so does T_2
    r = ref.segment_fit(f, LABELS, N_SEG, 1.0, 2)
    assert r["models"][2].tolist() == [0, 0, 1.5, 0, 0, 0] and r["seg_counts"][2].tolist() == [3, 3, 0, 1]
    assert np.array_equal(r["models"][[0, 1, 3]], np.array([MODEL_A, MODEL_B, [0, 0, 1.5, 0, 0, 0.5]], F32))
    r = ref.segment_fit(f, LABELS, N_SEG, 1.0, 3)
    assert r["models"][2].tolist() == [0] * 6 and r["seg_counts"][2].tolist() == [3, 3, 2, 1] and r["cls"][0, 2:5].tolist() == [1, 1, 2]
    assert ref.segment_fit(f, LABELS, N_SEG, 1.0, 2, mutate="t_power")["models"][2].tolist() == [0] * 6
    # a threshold so small that segment 3 (1.5 against 1 and 2) loses every pixel in round 1: its translation stays
    r = ref.segment_fit(f, LABELS, N_SEG, 0.125, 2)
    assert r["models"][3].tolist() == [0, 0, 1.5, 0, 0, 0.5] and r["seg_counts"][3].tolist() == [2, 2, 0, 1]


def test_the_solve_by_itself():
    # N = 0: nothing; N = 1 and 2: the mean; three pixels of a column: det == 0, the mean
    assert ref.solve(np.zeros(12, np.int64), 6, 4) == (0, None)
    k, m = ref.solve(np.array([1, 3, 1, 9, 3, 1, 65, 195, 65, -32, -96, -32], np.int64), 6, 4)
    assert k == 1 and m.tolist() == [0, 0, 65 / 64, 0, 0, -0.5]
    a, b, p = np.array([1, 1, 1]), np.array([-3, -1, 1]), np.array([64, 128, 192])
    S = [3, a.sum(), b.sum(), (a * a).sum(), (a * b).sum(), (b * b).sum(), p.sum(), (a * p).sum(), (b * p).sum(), 0, 0, 0]
    k, m = ref.solve(np.array(S, np.int64), 6, 4)
    assert k == 1 and m.tolist() == [0, 0, 2, 0, 0, 0]


@pytest.mark.parametrize("mutate", ["tie_larger", "floor_div", "target_right_down", "t_power"])
def test_a_mutation_changes_only_its_own_definition(mutate):
    """Each mutation is noticed by one of the tests above; the other definition does not look at it."""
    img = two_colours()
    same = {"tie_larger": "fit", "floor_div": "fit", "target_right_down": "fit", "t_power": "slic"}[mutate]
    if same == "fit":
        a, b = ref.segment_fit(hand_flow(), LABELS, N_SEG, 1.0, 3), ref.segment_fit(hand_flow(), LABELS, N_SEG, 1.0, 3, mutate=mutate)
    else:
        a, b = ref.superpixels(img, 8, 0, 2, 3), ref.superpixels(img, 8, 0, 2, 3, mutate=mutate)
    assert all(np.array_equal(a[k], b[k]) for k in a)
