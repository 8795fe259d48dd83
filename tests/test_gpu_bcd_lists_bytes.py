"""bcd_lists_kernel byte for byte: the two regions dflow_bcd_prepare writes in full, lab and blkA, against tests/bcd_lists_ref.py
(numpy, from the header comment of csrc/bcd.hip), on uploaded proposals of 12 x 16 frames at label_pitch 160.

Label counts per pixel come from {1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 100, 125, 127, 128, 129, 150, 159, 160}: every chunk of
8 columns and every row word of the predecessor ends somewhere, and 4-neighbours always differ, so a wave's predecessor and its
two successors disagree.  Frames (bcd_lists_ref.frames): "all" (every label compatible with every other: more than 15 members,
pool rows, the cut-back to 15), "none" (no compatible pair), "random" (every list length; labels next to (-32768, -32768), the
flow the kernel gives to lanes without a label), "exact" (labels with exactly 5, 6, 10, 11, 15 and 16 members, scattered over the
row words), "sevens" / "twelves" (every label owns a second / third block: more than 40 / 24 per wave, the slot caps).

Every frame runs under the three poison bytes of ws_guard in a region of exactly the stage's need (an unwritten slot of lab or
blkA cannot equal the reference under all three), and after dflow_bcd_prepare + one dflow_bcd_sweep the labels equal the CPU
oracle's.  The reference itself is checked on the host (no GPU): decoded back and compared with a plain loop over label pairs,
and the frames are checked to contain the cases named above."""
import ctypes as C
import functools

import numpy as np
import pytest

import bcd_lists_ref as R
import ws_guard as G
from conftest import pkg

TPSI = 8
FRAMES, SIZES, SLOTS = R.frames()
NAMES = tuple(FRAMES)


@functools.lru_cache(maxsize=None)
def reference(name):
    st = FRAMES[name]
    return R.prepared(st["proposals"], st["lcosts"], st["nprop"], TPSI)


def members(P, Q, tl):
    """Plain loop: the compatible labels of the predecessor and their pair costs."""
    out = []
    for k in range(len(Q)):
        d = abs(int(P[tl][0]) - int(Q[k][0])) + abs(int(P[tl][1]) - int(Q[k][1]))
        if d < TPSI:
            out.append((k, d))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_reference_decodes_to_the_compat_lists(name):
    """Host only.  Sampled (pixel, direction, label): the block's member bytes, cost nibbles, count and flags against a plain loop."""
    st = FRAMES[name]
    lab, blk, counts = reference(name)
    rng = np.random.RandomState(11)
    nprop = st["nprop"]
    for _ in range(150):
        y, x, d = rng.randint(R.H), rng.randint(R.W), rng.randint(2)
        tl = rng.randint(R.LP)
        bx, by = int(blk[y, x, d, tl, 0]), int(blk[y, x, d, tl, 1])
        q = R.predecessor(y, x, R.H, R.W, d)
        if q is None or tl >= nprop[y, x]:
            assert (bx, by) == (R.EMPTY_X, R.EMPTY_Y), (name, y, x, d, tl)
            continue
        m = members(st["proposals"][y, x, :nprop[y, x]], st["proposals"][q][:nprop[q]], tl)
        assert counts[y, x, d, tl] == len(m)
        got = [(bx >> (8 * j)) & 0xFF for j in range(4)] + [by & 0xFF]
        want = [k for k, _ in m[:5]] + [0xFF] * (5 - min(5, len(m)))
        assert got == want, (name, y, x, d, tl)
        assert [(by >> (8 + 4 * j)) & 7 for j in range(5)] == [c for _, c in m[:5]] + [0] * (5 - min(5, len(m)))
        more, has_b, has_c = bool(by & R.BLK_MORE), bool(by & R.BLK_HAS_B), bool(by & R.BLK_HAS_C)
        assert by >> 28 == (15 if more else min(len(m), 15))
        assert (not has_b or len(m) > 5) and (not has_c or (len(m) > 10 and has_b))
        assert more == (len(m) > 15 or (len(m) > 5 and not has_b) or (len(m) > 10 and not has_c))
    assert lab.shape == (R.H, R.W, R.LP, 2) and (lab[..., 0][np.arange(R.LP)[None, None, :] >= nprop[..., None]] == 0).all()


def test_frames_hold_the_cases():
    """Host only.  What the frames are there for, read off the reference."""
    nprop = FRAMES["all"]["nprop"]
    assert set(nprop.ravel()) == set(R.COUNTS)
    assert (nprop[:, 1:] != nprop[:, :-1]).all() and (nprop[1:] != nprop[:-1]).all()
    cnt = {n: reference(n)[2] for n in NAMES}
    blk = {n: reference(n)[1] for n in NAMES}
    assert cnt["all"].max() == 160 and (cnt["all"] > 15).any()
    pred = cnt["all"] >= 0
    interior = np.zeros_like(pred)
    for y in range(R.H):
        for x in range(R.W):
            for d in (0, 1):
                q = R.predecessor(y, x, R.H, R.W, d)
                if q is not None:
                    interior[y, x, d, :nprop[y, x]] = True
                    assert (cnt["all"][y, x, d, :nprop[y, x]] == nprop[q]).all()          # every label against every label
    assert (pred == interior).all()
    assert cnt["none"].max() == 0 and ((blk["none"][..., 0] == R.EMPTY_X) & (blk["none"][..., 1] == R.EMPTY_Y)).all()
    assert set(range(0, 17)) <= set(cnt["random"].ravel())
    # "exact": against a predecessor with all 160 labels, the labels of group i have exactly SIZES[i] members
    st, at, seen = FRAMES["exact"], 0, set()
    for i, s in enumerate(SIZES):
        for y in range(R.H):
            for x in range(R.W):
                for d in (0, 1):
                    q = R.predecessor(y, x, R.H, R.W, d)
                    tl = int(SLOTS[at])
                    if q is not None and st["nprop"][q] == 160 and tl < st["nprop"][y, x]:
                        assert cnt["exact"][y, x, d, tl] == s
                        seen.add(s)
        at += s
    assert seen == set(SIZES)
    # the slot caps: labels with 6..10 members marked "more" (no second block), with 11..15 and a second but no third block
    for n, lo in (("sevens", 7), ("twelves", 12)):
        y_ = blk[n][..., 1]
        full = cnt[n] == lo
        assert (full & ((y_ & R.BLK_HAS_B) != 0)).any() and (full & ((y_ & R.BLK_HAS_B) == 0) & ((y_ & R.BLK_MORE) != 0)).any()
    y_ = blk["twelves"][..., 1]
    assert ((cnt["twelves"] == 12) & ((y_ & R.BLK_HAS_B) != 0) & ((y_ & R.BLK_HAS_C) == 0) & ((y_ & R.BLK_MORE) != 0)).any()
    assert ((cnt["twelves"] == 12) & ((y_ & R.BLK_HAS_C) != 0) & ((y_ & R.BLK_MORE) == 0)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_prepare_writes_the_reference_bytes(oracle, name):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    st = FRAMES[name]
    lab, blk, _ = reference(name)
    want = (lab.tobytes(), blk.tobytes())
    (l0, l1), (a0, a1) = R.plane_offsets(R.H, R.W)
    labels = None
    for poison in G.POISONS:
        df = pkg("pipeline").DiscreteFlow(R.H, R.W, 6, 8, seed=3, maxnprop=R.LP, label_pitch=R.LP, tpsi=TPSI)
        need = G.stage_need("dflow_bcd_prepare", C.byref(df.p), G.PTR, G.PTR, G.PTR)
        assert a1 < need
        g = G.guard_pass(df, poison, need)
        df.set_host_state(st["proposals"], st["lcosts"], st["nprop"], st["bestlabels"])
        df.pakovanje()
        ws = g.snapshot()
        what = "%s, poison 0x%02X" % (name, poison)
        g.assert_guards(what)
        for region, (b0, b1), ref in (("lab", (l0, l1), want[0]), ("blkA", (a0, a1), want[1])):
            got = np.frombuffer(ws[b0:b1], np.uint32)
            bad = np.flatnonzero(got != np.frombuffer(ref, np.uint32))
            assert bad.size == 0, "%s: %s differs in %d words, first at word %d (pixel %d): %08X, reference %08X" % (
                what, region, bad.size, bad[0], bad[0] // (2 * R.LP * (1 if region == "lab" else 2)), got[bad[0]],
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
        name, int((labels != bl).sum()))
