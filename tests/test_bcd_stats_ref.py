"""tests/bcd_stats_ref.py, the numpy restatement of dflow_bcd_stats, against energies written out by hand and against an
independent double loop on the golden fixtures.  No GPU."""
import math

import numpy as np
import pytest

from bcd_stats_ref import bcd_stats_ref, energy
from conftest import GOLDEN_NAMES


def field(flows, costs, labels, nprop=None):
    """flows: (H,W,L,2), costs: (H,W,L) -> the arguments of bcd_stats_ref."""
    flows, costs, labels = np.asarray(flows, np.int64), np.asarray(costs, np.float32), np.asarray(labels, np.int64)
    if nprop is None:
        nprop = np.full(labels.shape, flows.shape[2], np.int64)
    return flows, costs, np.asarray(nprop, np.int64), labels


def test_two_by_two_by_hand():
    # chosen flows:  (0,0) (1,2)      costs: 0.5  2.5
    #                (5,5) (1,-3)            1.25 0.25
    # pairs: right of (0,0): |0-1|+|0-2| = 3; right of (1,0): |5-1|+|5+3| = 12 -> 8, truncated
    #        below (0,0): 10 -> 8, truncated; below (0,1): |1-1|+|2+3| = 5
    flows = [[[(9, 9), (0, 0)], [(1, 2), (9, 9)]], [[(5, 5), (7, 7)], [(7, 7), (1, -3)]]]
    costs = [[[9.0, 0.5], [2.5, 9.0]], [[1.25, 9.0], [9.0, 0.25]]]
    labels = [[1, 0], [0, 1]]
    st = bcd_stats_ref(*field(flows, costs, labels), tpsi=8, tphi=2.5)
    assert st["smooth_sum"] == 3 + 8 + 8 + 5 and st["n_pairs_trunc"] == 2
    assert st["data_sum"] == 0.5 + 2.5 + 1.25 + 0.25 and st["n_data_trunc"] == 1
    assert st["n_changed"] == 0 and st["n_bad_label"] == 0
    assert energy(st, 0.05) == 0.05 * 4.5 + 24
    # tpsi = 1: every pair with a difference is truncated to 1
    st = bcd_stats_ref(*field(flows, costs, labels), tpsi=1, tphi=0.25)
    assert st["smooth_sum"] == 4 and st["n_pairs_trunc"] == 4 and st["n_data_trunc"] == 4
    # labels that changed at two pixels
    st = bcd_stats_ref(*field(flows, costs, labels), tpsi=8, tphi=2.5, prev=np.array([[1, 1], [0, 0]]))
    assert st["n_changed"] == 2


def test_one_by_three_by_hand_with_a_bad_label():
    # one row, no lower pairs: flows (2,2) (2,3) (-4,3); pairs 1 and 6
    flows = [[[(2, 2)], [(2, 3)], [(-4, 3)]]]
    costs = [[[0.125], [1.0], [2.0]]]
    st = bcd_stats_ref(*field(flows, costs, [[0, 0, 0]]), tpsi=8, tphi=2.5)
    assert (st["smooth_sum"], st["n_pairs_trunc"], st["data_sum"], st["n_data_trunc"]) == (7, 0, 3.125, 0)
    # the middle label out of range: it takes both pairs and its cost with it, and counts as changed
    for bad in (-1, 1):
        st = bcd_stats_ref(*field(flows, costs, [[0, bad, 0]]), tpsi=8, tphi=2.5, prev=np.array([[0, bad, 0]]))
        assert (st["smooth_sum"], st["n_pairs_trunc"], st["data_sum"]) == (0, 0, 2.125)
        assert st["n_bad_label"] == 1 and st["n_changed"] == 1 and st["n_data"] == 2
    # no earlier labelling: n_changed is 0 whatever the labels are
    assert bcd_stats_ref(*field(flows, costs, [[0, 5, 0]]), tpsi=8, tphi=2.5)["n_changed"] == 0


def test_float64_costs_are_refused():
    with pytest.raises(TypeError):
        bcd_stats_ref(np.zeros((1, 1, 1, 2), np.int64), np.zeros((1, 1, 1)), np.ones((1, 1), np.int64), np.zeros((1, 1), np.int64), 8, 2.5)


def loop_energy(proposals, lcosts, labels, tpsi, lamda):
    """sum lamda lcost + sum over 4-adjacent pairs of min(tpsi, |f_p - f_q|_1), pixel by pixel."""
    H, W = labels.shape
    data, smooth = [], 0
    for y in range(H):
        for x in range(W):
            l = int(labels[y, x])
            data.append(float(lcosts[y, x, l]))
            for (qy, qx) in ((y, x + 1), (y + 1, x)):
                if qy < H and qx < W:
                    fq = proposals[qy, qx, int(labels[qy, qx])]
                    fp = proposals[y, x, l]
                    smooth += min(tpsi, abs(int(fp[0]) - int(fq[0])) + abs(int(fp[1]) - int(fq[1])))
    return lamda * math.fsum(data) + smooth, smooth


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_fixture_rows_equal_a_double_loop(golden, name):
    """The fixtures store the first two rows of proposals and lcosts of both directions and the labels after every sweep:
    the energy of that 2 x W strip, for every direction and sweep."""
    g = golden(name)
    for backward in (0, 1):
        k = "b%d_" % backward
        pr = g[k + "proposals_rows"].astype(np.int64)
        lc64 = g[k + "lcosts_rows"]
        lc = lc64.astype(np.float32)
        assert np.array_equal(lc.astype(np.float64), lc64)              # the reference's costs are float32-exact
        npr = g[k + "nprop"][:2].astype(np.int64)
        prev = None
        for w in range(int(g["bcd_times"]) + 1):
            lab = g[k + "labels%02d" % w][:2].astype(np.int64)
            st = bcd_stats_ref(pr, lc, npr, lab, tpsi=8, tphi=2.5, prev=prev)
            e, smooth = loop_energy(pr, lc, lab, 8, 0.05)
            assert st["n_bad_label"] == 0 and st["smooth_sum"] == smooth
            assert energy(st, 0.05) == e
            assert st["n_changed"] == (0 if prev is None else int((lab != prev).sum()))
            assert st["n_data_trunc"] == int(sum(lc[y, x, lab[y, x]] >= np.float32(2.5) for y in range(2) for x in range(lab.shape[1])))
            prev = lab
