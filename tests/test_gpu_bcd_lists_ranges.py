"""bcd_lists_kernel's range lookups byte for byte.  The kernel finds a label's compatible predecessors as a box in the rotated
coordinates u = dy + dx, v = dy - dx (two rank tables and two prefix-set tables per wave, csrc/bcd.hip), and falls back to the
all-pairs test when a pixel's labels span its rank table or more.  Both regions dflow_bcd_prepare writes in full, lab and blkA,
are compared with tests/bcd_lists_ref.py (numpy, |dy-dy'| + |dx-dx'| < tpsi as written) on 12 x 16 frames at label_pitch 160 with
the label counts of bcd_lists_ref.COUNTS, under the three poison bytes of ws_guard, and after one sweep the labels with the CPU
oracle's.  Frames:

  diamond   every label of a pixel lies at an offset of L1 norm tpsi - 1, tpsi or tpsi + 1 from the same label of its
            4-neighbours: all (a, b) with |a| + |b| = n, so the four axis directions, the four diagonals and the uneven splits:
            where a box that is not rotated, or a range end that is off by one, shows
  ties      groups of labels that share u and differ in v, groups that share v and differ in u, and exact duplicates of a whole
            flow: several equal values in one rank-table entry, placed in arbitrary order
  window    pixels whose labels span exactly R - 1 (tables), R and R + 1 (all-pairs) on u only, on v only and on both, next to
            each other and to narrow ones, so that waves of both kinds serve each other's successors
  extremes  pixels with all labels at one corner of the int16 square (tables at the ends of the coordinate range), pixels with
            labels at all four corners and ordinary ones (all-pairs: a span of 131070); (-32768, -32768) is the flow the kernel
            gives to lanes without a label
  tpsi      diamond and ties again at tpsi = 1 (only equal flows are compatible) and tpsi = 2

Each frame has a host-only test that reads off the reference that the frame holds its case."""
import ctypes as C
import functools

import numpy as np
import pytest

import bcd_lists_ref as R
import ws_guard as G
from conftest import pkg

RANGE_R = 767       # BCD_RANGE_R of csrc/bcd.hip: a wave whose labels span this or more (max - min) on u or v takes the all-pairs loop
H, W, LP = R.H, R.W, R.LP
CASES = (("diamond", 8), ("ties", 8), ("window", 8), ("extremes", 8), ("diamond", 1), ("ties", 1), ("diamond", 2), ("ties", 2))
IDS = ["%s-tpsi%d" % c for c in CASES]


def offsets(tpsi):
    """All (a, b) with |a| + |b| in {tpsi - 1, tpsi, tpsi + 1}."""
    out = []
    for n in (tpsi - 1, tpsi, tpsi + 1):
        for a in range(-n, n + 1):
            b = n - abs(a)
            out += [(a, b), (a, -b)] if b else [(a, 0)]
    return sorted(set(out))


def base_labels():
    """Label k of every pixel before its offset: at least 37 apart from every other label."""
    k = np.arange(LP)
    return np.stack([37 * (k % 13) - 200, 41 * (k // 13) - 250], axis=-1)


def diamond(tpsi):
    """Pixels with y + x even hold the base labels, the others base + offset; 4-neighbours are always of the other kind, and the
    offsets are symmetric, so every (pixel, predecessor) pair sees them."""
    offs = np.array(offsets(tpsi))
    yy, xx = np.mgrid[0:H, 0:W]
    idx = (np.arange(LP)[None, None, :] + 5 * yy[..., None] + 11 * xx[..., None]) % len(offs)
    full = base_labels()[None, None] + np.where(((yy + xx) & 1)[..., None, None] == 1, offs[idx], 0)
    return R._finish(full, 21)


def ties():
    """20 groups of 8 labels around centres 20 apart.  Even groups step by (+1, -1): one u, v two apart; odd groups by (+1, +1): one
    v, u two apart; the steps 5, 6 and 7 of a group are the same flow.  Blocks of 2 x 2 pixels share a shift of 0 or 1 per axis."""
    k = np.arange(LP)
    g, i = k // 8, np.minimum(k % 8, 5)
    one = np.stack([20 * (g % 5) + i, 20 * (g // 5) + np.where(g % 2 == 0, -i, i)], axis=-1)
    yy, xx = np.mgrid[0:H, 0:W]
    shift = np.stack([(yy // 2) % 2, (xx // 2) % 2], axis=-1)
    return R._finish(one[None, None] + shift[:, :, None, :], 22)


def window():
    """Rows y % 4 = 0 / 1 / 2: labels 0 and 1 of a pixel are the two ends of a span on u / v / both, the span R - 1, R, R + 1 by
    x % 3; rows y % 4 = 3 stay narrow.  The other labels lie in [-20, 20]^2.  Row neighbours share the axis and differ in the span
    by at most 2, so the far labels have members across the two kinds of wave."""
    rng = np.random.RandomState(23)
    full = rng.randint(-20, 21, size=(H, W, LP, 2))
    for y in range(H):
        for x in range(W):
            mode, far = y % 4, RANGE_R - 1 + x % 3 - 512
            if mode == 0:                                 # u from -512 to far, v in {0, -1}
                full[y, x, 0], full[y, x, 1] = (-256, -256), (far // 2, far - far // 2)
            elif mode == 1:                               # v from -512 to far, u in {0, 1}
                full[y, x, 0], full[y, x, 1] = (-256, 256), (-(-far // 2), -(-far // 2) - far)
            elif mode == 2:                               # u and v from -512 to far
                full[y, x, 0], full[y, x, 1] = (-512, 0), (far, 0)
    return R._finish(full, 24)


CORNERS = ((-32768, -32768, 1, 1), (32767, 32767, -1, -1), (-32768, 32767, 1, -1), (32767, -32768, -1, 1))


def extremes():
    """(y + 2 x) % 6 = c < 4: every label within 6 of corner c (label 0 on it); 4, 5: label k at corner k % 5, k % 5 = 4 ordinary."""
    rng = np.random.RandomState(25)
    inward = rng.randint(0, 7, size=(H, W, LP, 2))
    inward[:, :, 0:4] = 0
    ordinary = rng.randint(-12, 13, size=(H, W, LP, 2))
    full = np.empty((H, W, LP, 2), np.int64)
    for y in range(H):
        for x in range(W):
            kind = (y + 2 * x) % 6
            for k in range(LP):
                c = kind if kind < 4 else k % 5
                if c == 4:
                    full[y, x, k] = ordinary[y, x, k]
                else:
                    cy, cx, sy, sx = CORNERS[c]
                    full[y, x, k] = (cy + sy * inward[y, x, k, 0], cx + sx * inward[y, x, k, 1])
    return R._finish(full, 26)


@functools.lru_cache(maxsize=None)
def state(name, tpsi):
    return {"diamond": lambda: diamond(tpsi), "ties": ties, "window": window, "extremes": extremes}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, tpsi):
    st = state(name, tpsi)
    return R.prepared(st["proposals"], st["lcosts"], st["nprop"], tpsi)


def pairs():
    for y in range(H):
        for x in range(W):
            for d in (0, 1):
                q = R.predecessor(y, x, H, W, d)
                if q is not None:
                    yield y, x, d, q


def spans(st):
    """(H, W, 2): max - min of u and of v over a pixel's labels."""
    p, n = st["proposals"], st["nprop"]
    out = np.zeros((H, W, 2), np.int64)
    for y in range(H):
        for x in range(W):
            f = p[y, x, :n[y, x]]
            u, v = f[:, 0] + f[:, 1], f[:, 0] - f[:, 1]
            out[y, x] = u.max() - u.min(), v.max() - v.min()
    return out


@pytest.mark.parametrize("tpsi", (8, 1, 2))
def test_diamond_holds_every_offset_on_both_sides_of_the_bound(tpsi):
    """Host only.  Every offset occurs between a label and the same label of a predecessor; it is a member exactly below tpsi."""
    st, (_, _, cnt) = state("diamond", tpsi), reference("diamond", tpsi)
    offs = offsets(tpsi)
    assert {(s * n, 0) for n in (tpsi - 1, tpsi, tpsi + 1) for s in (1, -1)} <= set(offs)
    assert {(0, s * n) for n in (tpsi - 1, tpsi, tpsi + 1) for s in (1, -1)} <= set(offs)
    if tpsi == 8:
        assert {(4 * a, 4 * b) for a in (1, -1) for b in (1, -1)} <= set(offs) and {(3, 5), (-5, 3), (1, -7), (-6, -2)} <= set(offs)
    seen = set()
    for y, x, d, q in pairs():
        n = min(st["nprop"][y, x], st["nprop"][q])
        delta = st["proposals"][y, x, :n] - st["proposals"][q][:n]
        l1 = np.abs(delta).sum(axis=1)
        assert np.array_equal(cnt[y, x, d, :n], (l1 < tpsi).astype(np.int64))      # nothing else is near
        seen |= {(int(a), int(b)) for a, b in delta}
    assert seen == set(offs)


def test_ties_hold_shared_coordinates_and_duplicates():
    """Host only."""
    st = state("ties", 8)
    y, x = np.argwhere(st["nprop"] == 160)[0]
    f = st["proposals"][y, x]
    u, v = f[:, 0] + f[:, 1], f[:, 0] - f[:, 1]
    assert len(set(v[0:6])) == 6 and len(set(u[0:6])) == 1 and len(set(u[8:14])) == 6 and len(set(v[8:14])) == 1
    assert (f[5] == f[6]).all() and (f[5] == f[7]).all()
    for tpsi in (1, 2, 8):
        cnt = reference("ties", tpsi)[2]
        assert cnt.max() >= 3 and (cnt == 0).any()           # the duplicates are members of each other even at tpsi = 1
    assert reference("ties", 8)[2].max() > reference("ties", 2)[2].max() >= reference("ties", 1)[2].max()


def test_window_holds_both_kinds_of_wave_as_neighbours():
    """Host only.  Spans of exactly R - 1, R and R + 1 on u only, v only and both; pairs of a table pixel and an all-pairs pixel
    in both roles; the far labels have members across such pairs."""
    st, (_, _, cnt) = state("window", 8), reference("window", 8)
    sp = spans(st)
    seen = {(int(a), int(b)) for a, b in sp.reshape(-1, 2) if max(a, b) >= RANGE_R - 1}
    for s in (RANGE_R - 1, RANGE_R, RANGE_R + 1):
        assert any(a == s and b < 100 for a, b in seen) and any(b == s and a < 100 for a, b in seen) and (s, s) in seen, s
    wide = sp.max(axis=2) >= RANGE_R
    assert wide.any() and (~wide).any() and (sp.max(axis=2) < 100).any()
    roles = set()
    for y, x, d, q in pairs():
        roles.add((bool(wide[y, x]), bool(wide[q])))
        if d == 1 and y % 4 != 3 and min(st["nprop"][y, x], st["nprop"][q]) >= 2:
            assert (cnt[y, x, d, 0:2] >= 1).all(), (y, x)
    assert roles == {(False, False), (False, True), (True, False), (True, True)}


def test_extremes_hold_the_corners():
    """Host only.  All four corners themselves occur as labels; pixels at one corner are narrow, mixed pixels span the whole range."""
    st, (lab, blk, cnt) = state("extremes", 8), reference("extremes", 8)
    flows = {tuple(f) for y in range(H) for x in range(W) for f in st["proposals"][y, x, :st["nprop"][y, x]]}
    assert {c[:2] for c in CORNERS} <= flows
    sp = spans(st).max(axis=2)
    assert (sp[st["nprop"] > 1] < RANGE_R).any() and (sp == 131070).any()
    assert cnt.max() > 15 and (cnt == 0).any()
    # labels beyond a pixel's count: flow 0 and the empty block, also next to predecessors with labels on (-32768, -32768)
    unused = np.arange(LP)[None, None, :] >= st["nprop"][..., None]
    assert (lab[..., 0][unused] == 0).all()
    for d in (0, 1):
        assert (blk[:, :, d, :, 0][unused] == R.EMPTY_X).all() and (blk[:, :, d, :, 1][unused] == R.EMPTY_Y).all()
    assert any(st["nprop"][y, x] < LP and (st["proposals"][q][0] == (-32768, -32768)).all() for y, x, d, q in pairs())


@pytest.mark.gpu
@pytest.mark.parametrize("name,tpsi", CASES, ids=IDS)
def test_prepare_writes_the_reference_bytes(oracle, name, tpsi):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    st = state(name, tpsi)
    lab, blk, _ = reference(name, tpsi)
    want = (lab.tobytes(), blk.tobytes())
    (l0, l1), (a0, a1) = R.plane_offsets(H, W)
    labels = None
    for poison in G.POISONS:
        df = pkg("pipeline").DiscreteFlow(H, W, 6, 8, seed=3, maxnprop=LP, label_pitch=LP, tpsi=tpsi)
        need = G.stage_need("dflow_bcd_prepare", C.byref(df.p), G.PTR, G.PTR, G.PTR)
        assert a1 < need
        g = G.guard_pass(df, poison, need)
        df.set_host_state(st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"])
        df.pakovanje()
        ws = g.snapshot()
        what = "%s, tpsi %d, poison 0x%02X" % (name, tpsi, poison)
        g.assert_guards(what)
        for region, (b0, b1), ref in (("lab", (l0, l1), want[0]), ("blkA", (a0, a1), want[1])):
            got = np.frombuffer(ws[b0:b1], np.uint32)
            bad = np.flatnonzero(got != np.frombuffer(ref, np.uint32))
            assert bad.size == 0, "%s: %s differs in %d words, first at word %d (pixel %d): %08X, reference %08X" % (
                what, region, bad.size, bad[0], bad[0] // (2 * LP * (1 if region == "lab" else 2)), got[bad[0]],
                np.frombuffer(ref, np.uint32)[bad[0]])
        df.ceoBCD(1)
        g.assert_guards(what + ", after a sweep")
        got = df.bestlabels.cpu().numpy()
        assert labels is None or np.array_equal(got, labels), what
        labels = got
    p = df.p
    po = oracle.make_params(p.pich, p.picw, p.cellh, p.cellw, seed=p.seed, maxnprop=p.maxnprop, tpsi=p.tpsi, lamda=p.lamda,
                            tphi=p.tphi)
    bl = st["bestlabels"].copy()
    oracle.bcd_sweep(po, st["proposals"], st["lcosts"], st["nprop"], bl)
    assert np.array_equal(labels, bl), "%s: labels after one sweep differ from the oracle's in %d pixels" % (
        what, int((labels != bl).sum()))
