"""What dflow_bcd_prepare leaves in the two workspace regions it writes in full (csrc/bcd.hip, header comment and BcdPlanes), built
in numpy from proposals, lcosts, nprop and tpsi:

  lab  [pix][LP]     {biased flow, data cost}: label k < nprop: packed label ^ 0x80008000 and the float32 cost, else 0 and 1000.0f
  blkA [pix][2][LP]  the first 8-byte block of label tl of pixel p against p's PREDECESSOR q on its column chain (0) / row chain
                     (1): x = the first four members k (bytes, increasing; 0xFF = none), y = the fifth | the pair costs of the
                     five as nibbles << 8 | BLK_MORE | BLK_HAS_B | BLK_HAS_C | count << 28.  Members = { k < nprop[q] :
                     |dy - dy'| + |dx - dx'| < tpsi }.  Second / third blocks (more than 5 / 10 members) get a slot by their rank
                     among the labels of the same 64-label wave that own one, 40 / 24 slots in waves 0 and 1, 16 / 8 in wave 2; a
                     label with more than 15 members, or whose second or third block found no slot, is marked "more" and reports
                     count 15.  Chain starts and labels >= nprop[p] hold the empty block.

Host only; frames() are the inputs of tests/test_gpu_bcd_lists_bytes.py."""
import numpy as np

LP = 160
CAP_B, CAP_C = (40, 40, 16), (24, 24, 8)
BLK_MORE, BLK_HAS_B, BLK_HAS_C = 0x800, 0x8000, 0x80000
EMPTY_X, EMPTY_Y = 0xFFFFFFFF, 0xFF
COUNTS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 100, 125, 127, 128, 129, 150, 159, 160)


def predecessor(y, x, H, W, d):
    """python bcd.py:265-277: even columns run down, odd columns up, even rows leftwards, odd rows rightwards."""
    if d == 0:
        py = y + 1 if x & 1 else y - 1
        return (py, x) if 0 <= py < H else None
    px = x - 1 if y & 1 else x + 1
    return (y, px) if 0 <= px < W else None


def pack(proposals):
    """(…,2) int [dy,dx] -> uint32 int16 dy | int16 dx << 16."""
    p = np.asarray(proposals).astype(np.int64)
    return ((p[..., 0] & 0xFFFF) | ((p[..., 1] & 0xFFFF) << 16)).astype(np.uint32)


def first_blocks(P, Q, tpsi, lp=LP):
    """P (tn,2), Q (pn,2) int64: the labels of a pixel and of its predecessor.  -> (x, y) uint32[lp], cnt int[tn]."""
    bx, by = np.full(lp, EMPTY_X, np.uint32), np.full(lp, EMPTY_Y, np.uint32)
    tn, pn = len(P), len(Q)
    if tn == 0 or pn == 0:
        return bx, by, np.zeros(tn, np.int64)
    D = np.abs(P[:, None, 0] - Q[None, :, 0]) + np.abs(P[:, None, 1] - Q[None, :, 1])
    C = D < tpsi
    cnt = C.sum(axis=1)
    key = np.sort(np.where(C, np.arange(pn)[None, :], 255), axis=1)
    mem = np.full((tn, 15), 255, np.int64)
    mem[:, :min(15, pn)] = key[:, :15]
    cost = np.where(mem < 255, np.take_along_axis(D, np.minimum(mem, pn - 1), axis=1), 0)
    assert cost.max(initial=0) < 8
    grp = np.arange(tn) // 64
    has_b, has_c = cnt > 5, cnt > 10
    rank_b, rank_c = np.zeros(tn, np.int64), np.zeros(tn, np.int64)
    for g in range(3):
        s = grp == g
        rank_b[s] = np.cumsum(has_b[s]) - has_b[s]
        rank_c[s] = np.cumsum(has_c[s]) - has_c[s]
    store_b = has_b & (rank_b < np.array(CAP_B)[grp])
    store_c = has_c & store_b & (rank_c < np.array(CAP_C)[grp])
    more = (cnt > 15) | (has_b & ~store_b) | (has_c & ~store_c)
    x = mem[:, 0] | (mem[:, 1] << 8) | (mem[:, 2] << 16) | (mem[:, 3] << 24)
    y = mem[:, 4].copy()
    for e in range(5):
        y |= cost[:, e] << (8 + 4 * e)
    y |= more * BLK_MORE | store_b * BLK_HAS_B | store_c * BLK_HAS_C | (np.where(more, 15, np.minimum(cnt, 15)) << 28)
    bx[:tn], by[:tn] = x.astype(np.uint32), y.astype(np.uint32)
    return bx, by, cnt


def prepared(proposals, lcosts, nprop, tpsi, lp=LP):
    """proposals (H,W,lp,2) int64, lcosts (H,W,lp) float, nprop (H,W) -> lab (H,W,lp,2) uint32, blkA (H,W,2,lp,2) uint32 and the
    member counts (H,W,2,lp) (-1: no such label / chain start)."""
    H, W = nprop.shape
    used = np.arange(lp)[None, None, :] < nprop[..., None]
    lab = np.zeros((H, W, lp, 2), np.uint32)
    lab[..., 0] = np.where(used, pack(proposals) ^ np.uint32(0x80008000), 0)
    lab[..., 1] = np.where(used, lcosts.astype(np.float32), np.float32(1000.0)).astype(np.float32).view(np.uint32)
    blk = np.empty((H, W, 2, lp, 2), np.uint32)
    blk[..., 0], blk[..., 1] = EMPTY_X, EMPTY_Y
    counts = np.full((H, W, 2, lp), -1, np.int64)
    for y in range(H):
        for x in range(W):
            for d in (0, 1):
                q = predecessor(y, x, H, W, d)
                if q is None:
                    continue
                tn, pn = int(nprop[y, x]), int(nprop[q])
                bx, by, cnt = first_blocks(proposals[y, x, :tn], proposals[q][:pn], tpsi, lp)
                blk[y, x, d, :, 0], blk[y, x, d, :, 1], counts[y, x, d, :tn] = bx, by, cnt
    return lab, blk, counts


def plane_offsets(H, W, lp=LP):
    """Byte ranges of lab and blkA in the BCD workspace, by planes_of (csrc/bcd.hip): back, the longest phase's chains x 192 bytes per
    step, comes first; every region starts on a multiple of 256."""
    a256 = lambda v: (v + 255) & ~255                    # noqa: E731
    back = a256(max(((W + 1) // 2) * H, ((H + 1) // 2) * W) * 192)
    lab, blk_a = H * W * lp * 8, H * W * 2 * lp * 8
    return (back, back + lab), (back + a256(lab), back + a256(lab) + blk_a)


# ------------------------------------------------------------------------------------------------ inputs
H, W = 12, 16
FAR = 3000


def _counts():
    """Every pixel's label count from COUNTS; 4-neighbours always differ (steps of 3 and 7 modulo 19)."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.array(COUNTS, np.int64)[(3 * yy + 7 * xx) % len(COUNTS)]


def _finish(full, seed):
    nprop = _counts()
    rng = np.random.RandomState(seed)
    used = np.arange(LP)[None, None, :] < nprop[..., None]
    proposals = np.where(used[..., None], full, -1).astype(np.int64)
    lc = (rng.randint(0, 641, size=(H, W, LP)) / 256.0).astype(np.float32)            # float32-exact costs in [0, 2.5]
    lcosts = np.where(used, lc, np.float32(1000.0)).astype(np.float64)
    return dict(proposals=np.ascontiguousarray(proposals), lcosts=np.ascontiguousarray(lcosts), nprop=nprop,
                bestlabels=np.zeros((H, W), np.int64))


def _clusters(size):
    """The same labels in every pixel: clusters of `size` labels within L1 distance 4 of each other, the clusters 30 apart."""
    k = np.arange(LP)
    r = k % size
    one = np.stack([(r % 3) + (r // 9), 30 * (k // size) + (r // 3) % 3], axis=-1)
    return np.broadcast_to(one, (H, W, LP, 2))


def frames():
    """name -> host state (reference dtypes) of a 12 x 16 frame at label_pitch 160."""
    rng = np.random.RandomState(5)
    out = {}
    # every label compatible with every other: more than 15 members everywhere, pool rows, the cut-back to 15
    out["all"] = _finish(rng.randint(0, 4, size=(H, W, LP, 2)), 1)
    # no compatible pair at all: the labels of a pixel lie 40 away from those of its neighbours
    yy, xx = np.mgrid[0:H, 0:W]
    out["none"] = _finish(np.stack([40 * yy, 40 * xx], axis=-1)[:, :, None, :] + rng.randint(0, 4, size=(H, W, LP, 2)), 2)
    # lists of every length around the block sizes, members in all five row words, and labels next to (-32768, -32768): the
    # flow value 0 after the bias, which the kernel loads into lanes that have no label
    rnd = rng.randint(-12, 13, size=(H, W, LP, 2))
    low = rng.rand(H, W, LP) < 0.08
    rnd[low] = -32768 + rng.randint(0, 4, size=(int(low.sum()), 2))
    out["random"] = _finish(rnd, 3)
    # exactly 5, 6, 10, 11, 15 and 16 members: group i is that many labels around (0, 40 i), in slots scattered over the row;
    # the other slots are far away from everything and from each other
    sizes = (5, 6, 10, 11, 15, 16)
    slots = rng.permutation(LP)
    one = np.stack([FAR + 20 * np.arange(LP), -FAR - 20 * np.arange(LP)], axis=-1)
    at = 0
    for i, s in enumerate(sizes):
        j = np.arange(s)
        one[slots[at:at + s]] = np.stack([j % 4, 40 * i + j // 4], axis=-1)
        at += s
    out["exact"] = _finish(np.broadcast_to(one, (H, W, LP, 2)), 4)
    # 7 / 12 members for every label: more than 40 labels of a wave own a second block, more than 24 a third one
    out["sevens"] = _finish(_clusters(7), 6)
    out["twelves"] = _finish(_clusters(12), 7)
    return out, sizes, slots
