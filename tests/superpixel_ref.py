"""numpy restatements of dflow_superpixels and dflow_segment_fit, written from the definitions in include/dflow.h and not from the
HIP code: uint64 keys and int64 sums for the SLIC, a plain breadth-first search for the components, int64 sums and float64 /
float32 scalars in the written order for the fit.  tests/test_superpixel_ref.py pins them by hand; tests/test_gpu_superpixels.py
holds the device to them byte for byte.

`mutate` names one deliberate mistake ("tie_larger", "floor_div", "target_right_down", "t_power"): the hand tests must notice each."""
from collections import deque

import numpy as np

KEY_BITS = 22
SP_COUNTS = ("K", "empty_centres", "components", "small", "pixels_merged", "n_seg", "largest", "reserved")
SF_COUNTS = ("part", "agree", "with_model", "affine", "translation", "bad_label", "out_of_range", "reserved")
F32 = np.float32


def grid(h, w, S):
    gw, gh = -(-w // S), -(-h // S)
    return gh, gw, gh * gw


def scan_len(h, w):
    """The int32 elements of dflow_superpixels' d_scan."""
    return -(-(h * w) // 256) + 1


def slic(img, S, m, iters, mutate=None):
    """The raw labels (h,w) int32 of the last assignment and the centres (K,8) int32 after its update."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w, _ = img.shape
    gh, gw, K = grid(h, w, S)
    assert K <= 1 << KEY_BITS
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    px = img.astype(np.int64)
    gy, gx = np.divmod(np.arange(K, dtype=np.int64), gw)
    cx0, cy0 = np.minimum(gx * S + S // 2, w - 1), np.minimum(gy * S + S // 2, h - 1)
    c = np.zeros((K, 8), np.int64)
    c[:, 0], c[:, 1] = 16 * cx0, 16 * cy0
    c[:, 2:5] = 16 * px[cy0, cx0]
    cell_y, cell_x = ys // S, xs // S
    lab = None
    for _ in range(iters):
        best = np.full((h, w), np.iinfo(np.uint64).max, np.uint64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cy, cx = cell_y + dy, cell_x + dx
                ok = (cy >= 0) & (cy < gh) & (cx >= 0) & (cx < gw)
                k = np.where(ok, cy * gw + cx, 0)
                ck = c[k]
                dc2 = sum((16 * px[..., j] - ck[..., 2 + j]) ** 2 for j in range(3))
                ds2 = (16 * xs - ck[..., 0]) ** 2 + (16 * ys - ck[..., 1]) ** 2
                assert dc2.max() < 1 << 26 and ds2.max() < 1 << 25, "the header's bounds"
                D = S * S * dc2 + m * m * ds2
                assert D.max() < 1 << 42
                low = (K - 1 - k) if mutate == "tie_larger" else k
                key = (D.astype(np.uint64) << np.uint64(KEY_BITS)) | low.astype(np.uint64)
                best = np.where(ok, np.minimum(best, key), best)
        lab = (best & np.uint64((1 << KEY_BITS) - 1)).astype(np.int64)
        if mutate == "tie_larger":
            lab = K - 1 - lab
        n = np.bincount(lab.ravel(), minlength=K).astype(np.int64)
        sums = np.zeros((K, 5), np.int64)
        for j, v in enumerate((xs, ys, px[..., 0], px[..., 1], px[..., 2])):
            np.add.at(sums[:, j], lab.ravel(), v.ravel())
        assert sums.max() < 1 << 32
        has = n > 0
        half = 0 if mutate == "floor_div" else (n[has] >> 1)[:, None]
        c[has, :5] = (16 * sums[has] + half) // n[has][:, None]
        c[:, 5] = n
    return lab.astype(np.int32), c.astype(np.int32)


def components(lab):
    """The 4-connected components of equal value, breadth first: (root per pixel, {root: size}); a root is the smallest raster
    index of its component."""
    lab = np.asarray(lab)
    h, w = lab.shape
    root = np.full((h, w), -1, np.int64)
    sizes = {}
    for y0 in range(h):
        for x0 in range(w):
            if root[y0, x0] >= 0:
                continue
            r, v, cnt = y0 * w + x0, lab[y0, x0], 0
            root[y0, x0] = r
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                cnt += 1
                for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= yy < h and 0 <= xx < w and root[yy, xx] < 0 and lab[yy, xx] == v:
                        root[yy, xx] = r
                        todo.append((yy, xx))
            sizes[r] = cnt
    return root, sizes


def merge_and_number(raw, min_size, mutate=None):
    """The component step and the numbering on any label plane: (final numbers (h,w) int32, counts[2:7])."""
    h, w = raw.shape
    root, sizes = components(raw)
    flat = root.ravel()

    def target(r):
        y0, x0 = divmod(r, w)
        if mutate == "target_right_down":
            return int(flat[r + 1]) if x0 + 1 < w else int(flat[r + w]) if y0 + 1 < h else None
        return int(flat[r - 1]) if x0 > 0 else int(flat[r - w]) if y0 > 0 else None

    final = {}
    for r in sizes:
        f, steps = r, 0
        while sizes[f] < min_size and f != 0:
            t = target(f)
            if t is None:
                break
            f, steps = t, steps + 1
            assert steps <= h * w
        final[r] = f
    finals = sorted(set(final.values()))
    number = {f: i for i, f in enumerate(finals)}
    fsize = dict.fromkeys(finals, 0)
    for r, f in final.items():
        fsize[f] += sizes[r]
    out = np.array([number[final[int(r)]] for r in flat], np.int32).reshape(h, w)
    merged = sum(sizes[r] for r, f in final.items() if f != r)
    small = sum(1 for r in sizes if sizes[r] < min_size)
    return out, [len(sizes), small, merged, len(finals), max(fsize.values())]


def superpixels(img, S, m, iters, min_size, mutate=None):
    """dflow_superpixels: dict(label, centers, slic, counts)."""
    raw, centers = slic(img, S, m, iters, mutate)
    label, tail = merge_and_number(raw, min_size, mutate)
    K = centers.shape[0]
    counts = np.array([K, int((centers[:, 5] == 0).sum())] + tail + [0], np.int32)
    return dict(label=label, centers=centers, slic=raw, counts=counts)


# ---------------------------------------------------------------------------------------------------- the per-segment fit
def flow_uv(flow):
    """(U, V, good) of a field in either layout; GOOD as in dflow_flow_consistency."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] in (2, 3)
    if flow.shape[2] == 3:
        U, V = flow[..., 0], flow[..., 1]
        valid = flow[..., 2] > F32(0.5)
    else:
        U, V = flow[..., 1], flow[..., 0]
        valid = np.ones(U.shape, bool)
    return U, V, valid & np.isfinite(U) & np.isfinite(V)


def solve(S, w, h):
    """The solve of one segment from its twelve integer sums: (kind, float32[6]); kind 0: N == 0, nothing is known."""
    N = int(S[0])
    if N == 0:
        return 0, None
    d = [float(int(v)) for v in S]                    # each sum converted to float64 once
    if N >= 3:
        n, sa, sb, saa, sab, sbb = d[:6]
        c00, c01, c02 = sbb * n - sb * sb, sb * sa - sab * n, sab * sb - sbb * sa
        c11, c12, c22 = saa * n - sa * sa, sa * sab - saa * sb, saa * sbb - sab * sab
        det = (saa * c00 + sab * c01) + sa * c02
        if det != 0.0 and np.isfinite(det):
            m = []
            with np.errstate(over="ignore"):
                for r2, r0, r1 in ((d[6], d[7], d[8]), (d[9], d[10], d[11])):
                    x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
                    x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
                    x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
                    m += [F32(x0 * 0.03125), F32(x1 * 0.03125), F32(((x2 - x0 * float(w - 1)) - x1 * float(h - 1)) * 0.015625)]
            if all(np.isfinite(v) for v in m):
                return 2, np.array(m, F32)
    z = F32(0.0)
    return 1, np.array([z, z, F32((d[6] / d[0]) * 0.015625), z, z, F32((d[9] / d[0]) * 0.015625)], F32)


def model_flow(models, lab, xf, yf):
    m = models[lab]
    Um = (m[..., 0] * xf + m[..., 1] * yf) + m[..., 2]
    Vm = (m[..., 3] * xf + m[..., 4] * yf) + m[..., 5]
    return Um, Vm


def agrees(U, V, Um, Vm, T):
    with np.errstate(invalid="ignore", over="ignore"):
        eu, ev = U - Um, V - Vm
        return eu * eu + ev * ev <= T * T


def segment_fit(flow, label, n_seg, thresh, rounds, mutate=None):
    """dflow_segment_fit: dict(models, seg_counts, out, cls, counts)."""
    U, V, good = flow_uv(flow)
    label = np.asarray(label)
    assert label.dtype == np.int32 and label.shape == U.shape
    h, w = U.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xf, yf = xs.astype(F32), ys.astype(F32)
    in_label = (label >= 0) & (label < n_seg)
    lab = np.where(in_label, label, 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        ranged = good & (np.abs(U) <= F32(32768)) & (np.abs(V) <= F32(32768))
    part = in_label & ranged
    a, b = 2 * xs - (w - 1), 2 * ys - (h - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.where(part, np.rint(np.where(part, U, 0) * F32(64)), 0).astype(np.int64)
        q = np.where(part, np.rint(np.where(part, V, 0) * F32(64)), 0).astype(np.int64)
    terms = (np.ones_like(a), a, b, a * a, a * b, b * b, p, a * p, b * p, q, a * q, b * q)
    models = np.zeros((n_seg, 6), F32)
    kind = np.zeros(n_seg, np.int32)
    seg_counts = np.zeros((n_seg, 4), np.int32)
    seg_counts[:, 0] = np.bincount(lab[in_label], minlength=n_seg)
    thresh = F32(thresh)
    for r in range(rounds):
        use = part
        if r > 0:
            T = thresh * F32(2.0 ** (rounds - 1 - r + (1 if mutate == "t_power" else 0)))
            Um, Vm = model_flow(models, lab, xf, yf)
            use = part & (kind[lab] != 0) & agrees(U, V, Um, Vm, T)
        sums = np.zeros((n_seg, 12), np.int64)
        for j, t in enumerate(terms):
            np.add.at(sums[:, j], lab[use], t[use])
        if r == 0:
            seg_counts[:, 1] = sums[:, 0]
        for s in range(n_seg):
            k, m = solve(sums[s], w, h)
            if k:
                kind[s], models[s] = k, m
    Um, Vm = model_flow(models, lab, xf, yf)
    has = in_label & (kind[lab] != 0)
    agree = part & has & agrees(U, V, Um, Vm, thresh)
    out = np.zeros((h, w, 3), F32)
    out[..., 0], out[..., 1], out[..., 2] = np.where(has, Um, F32(0)), np.where(has, Vm, F32(0)), np.where(has, F32(1), F32(0))
    cls = np.where(~part, 0, np.where(~has, 3, np.where(agree, 1, 2))).astype(np.uint8)
    seg_counts[:, 2] = np.bincount(lab[agree], minlength=n_seg)
    seg_counts[:, 3] = kind
    counts = np.array([part.sum(), agree.sum(), (kind != 0).sum(), (kind == 2).sum(), (kind == 1).sum(), (~in_label).sum(),
                       (good & ~ranged).sum(), 0], np.int32)
    return dict(models=models, seg_counts=seg_counts, out=out, cls=cls, counts=counts)
