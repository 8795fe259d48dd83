"""dflow_two_view restated from include/dflow.h ("Two-view reconstruction"): the essential matrix, the cyclic Jacobi sweeps and the
four candidates in plain Python floats (IEEE doubles), the vote and the apply step in numpy float64 arrays, one operation per
written operation in the written order, with no np.linalg anywhere in the chain.  The scenes, `rotation`, `field` and `dirty` are
epipolar_ref's; the planes of a field and the normalisation are motion_ref's."""
import math

import numpy as np

import epipolar_ref as E
from motion_ref import Field, normalisation

F = np.float32
SWEEPS = 8                          # TV_SWEEPS of csrc/two_view.hip
SIGMA2_MIN = 2.0 ** -20             # TV_SIGMA2_MIN
PAIRS = ((0, 1), (0, 2), (1, 2))
THREADS, PER_LANE = 256, 8            # TV_THREADS, TV_PER_LANE: a block votes on THREADS * PER_LANE contiguous grid pixels
COUNTS = ("voters", "votes", "runner_up", "candidate", "front", "behind", "flat", "reserved")
MUTATIONS = ("w_twice", "vote_z1_only", "tie_larger", "den32", "u3_from_E")


def essential(model, h, w, fx, fy, cx, cy):
    """A. E = A^T F^ A as three rows of Python floats."""
    cxF, cyF, s, _ = normalisation(h, w)
    f = [float(v) for v in np.asarray(model, F).reshape(9)]
    a00, a02, a11, a12 = s * fx, s * (cx - cxF), s * fy, s * (cy - cyF)
    G = [[f[3 * i] * a00, f[3 * i + 1] * a11, (f[3 * i] * a02 + f[3 * i + 1] * a12) + f[3 * i + 2]] for i in range(3)]
    return [[a00 * G[0][j] for j in range(3)], [a11 * G[1][j] for j in range(3)],
            [(a02 * G[0][j] + a12 * G[1][j]) + G[2][j] for j in range(3)]]


def jacobi(M):
    """The eigenvalues (the diagonal) and eigenvectors (the columns of V) of the symmetric 3 x 3 M after SWEEPS cyclic sweeps."""
    M = [[float(x) for x in row] for row in M]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            apq = M[p][q]
            if apq == 0.0:
                continue
            theta = (M[q][q] - M[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))          # an overflowed theta gives t = 0
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * c
            r = 3 - p - q
            M[p][p], M[q][q] = M[p][p] - t * apq, M[q][q] + t * apq
            M[p][q] = M[q][p] = 0.0
            arp, arq = M[r][p], M[r][q]
            M[r][p] = M[p][r] = c * arp - sn * arq
            M[r][q] = M[q][r] = sn * arp + c * arq
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - sn * vkq, sn * vkp + c * vkq
    return [M[0][0], M[1][1], M[2][2]], V


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def mat_vec(Em, v):
    return [(Em[i][0] * v[0] + Em[i][1] * v[1]) + Em[i][2] * v[2] for i in range(3)]


def decompose(model, h, w, fx, fy, cx, cy, w_twice=False, u3_from_E=False):
    """A and B -> None (NO POSE) or dict(Ra, Rb: nine floats row-major, t: three, sigma: the three ratios).  w_twice and u3_from_E
    are mutations."""
    if not np.asarray(model, F).any():
        return None
    Em = essential(model, h, w, fx, fy, cx, cy)
    M = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            M[i][j] = M[j][i] = (Em[0][i] * Em[0][j] + Em[1][i] * Em[1][j]) + Em[2][i] * Em[2][j]
    lam, V = jacobi(M)
    idx = [0, 1, 2]
    for i in (1, 2):
        j = i
        while j > 0 and lam[idx[j]] > lam[idx[j - 1]]:
            idx[j], idx[j - 1] = idx[j - 1], idx[j]
            j -= 1
    v = [[V[k][idx[i]] for k in range(3)] for i in range(3)]
    det = (v[0][0] * (v[1][1] * v[2][2] - v[2][1] * v[1][2]) - v[1][0] * (v[0][1] * v[2][2] - v[2][1] * v[0][2])) \
        + v[2][0] * (v[0][1] * v[1][2] - v[1][1] * v[0][2])
    if det < 0.0:
        v[2] = [-x for x in v[2]]
    w1 = mat_vec(Em, v[0])
    s1 = math.sqrt(dot3(w1, w1))
    if not (math.isfinite(s1) and s1 > 0.0):
        return None
    u1 = [x / s1 for x in w1]
    w2 = mat_vec(Em, v[1])
    g = dot3(w2, u1)
    w2 = [w2[i] - g * u1[i] for i in range(3)]
    s2 = math.sqrt(dot3(w2, w2))
    if not s2 > SIGMA2_MIN * s1:
        return None
    u2 = [x / s2 for x in w2]
    u3 = cross3(u1, u2)
    w3 = mat_vec(Em, v[2])
    s3 = math.sqrt(dot3(w3, w3))
    if u3_from_E:
        u3 = [x / s3 for x in w3] if s3 > 0.0 else [0.0, 0.0, 0.0]
    Ra = [(u2[i] * v[0][j] - u1[i] * v[1][j]) + u3[i] * v[2][j] for i in range(3) for j in range(3)]
    Rb = [(u1[i] * v[1][j] - u2[i] * v[0][j]) + u3[i] * v[2][j] for i in range(3) for j in range(3)]
    return dict(Ra=Ra, Rb=Ra if w_twice else Rb, t=u3, sigma=[1.0, s2 / s1, s3 / s1])


def geometry(R, t, x1, y1, x2, y2, den32=False):
    """C. (r, d, n1, n2) of one candidate at float64 arrays."""
    with np.errstate(all="ignore"):
        r = [(R[3 * i] * x1 + R[3 * i + 1] * y1) + R[3 * i + 2] for i in range(3)]
        c0, c1, c2 = r[1] - r[2] * y2, r[2] * x2 - r[0], r[0] * y2 - r[1] * x2
        d = (c0 * c0 + c1 * c1) + c2 * c2
        if den32:                                      # the mutation: |r|^2 |x2|^2 - (r.x2)^2 in float32
            rr, xx = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]).astype(F), ((x2 * x2 + y2 * y2) + 1.0).astype(F)
            rx = ((r[0] * x2 + r[1] * y2) + r[2]).astype(F)
            d = (rr * xx - rx * rx).astype(np.float64)
        a0, a1, a2 = y2 * t[2] - t[1], t[0] - x2 * t[2], x2 * t[1] - y2 * t[0]
        n1 = (a0 * c0 + a1 * c1) + a2 * c2
        b0, b1, b2 = r[1] * t[2] - r[2] * t[1], r[2] * t[0] - r[0] * t[2], r[0] * t[1] - r[1] * t[0]
        n2 = (b0 * c0 + b1 * c1) + b2 * c2
    return r, d, n1, n2


def candidates(dec):
    neg = [-x for x in dec["t"]]
    return [(dec["Ra"], dec["t"]), (dec["Ra"], neg), (dec["Rb"], dec["t"]), (dec["Rb"], neg)]


def two_view(flow, model, fx=None, fy=None, cx=None, cy=None, part=None, step=1, w_twice=False, u3_from_E=False, vote_z1_only=False,
             tie_larger=False, den32=False):
    """dflow_two_view -> dict: pose float64[16], votes [4], depth (h,w) float32, cls (h,w) uint8, err (h,w) float32, counts [8].
    fx = fy = max(h, w) and the frame's centre by default.  The last five arguments are the mutations the tests must catch."""
    fd = Field(flow, None, step)
    h, w = fd.h, fd.w
    fx = float(max(h, w)) if fx is None else float(fx)
    fy = fx if fy is None else float(fy)
    cx = (w - 1) * 0.5 if cx is None else float(cx)
    cy = (h - 1) * 0.5 if cy is None else float(cy)
    dec = decompose(model, h, w, fx, fy, cx, cy, w_twice=w_twice, u3_from_E=u3_from_E)
    cover = fd.good & fd.on_grid
    if part is not None:
        cover &= np.asarray(part).reshape(-1) == 1
    with np.errstate(all="ignore"):
        x1, y1 = (fd.xf.astype(np.float64) - cx) / fx, (fd.yf.astype(np.float64) - cy) / fy
        x2, y2 = (fd.tx.astype(np.float64) - cx) / fx, (fd.ty.astype(np.float64) - cy) / fy
    votes, best = [0, 0, 0, 0], -1
    if dec is not None:
        for k, (R, t) in enumerate(candidates(dec)):
            _, d, n1, n2 = geometry(R, t, x1, y1, x2, y2, den32)
            with np.errstate(all="ignore"):
                ok = (d > 0) & (d < np.inf) & (n1 > 0) & ((n2 > 0) | vote_z1_only)
            votes[k] = int((ok & cover).sum())
        for k in range(4):
            if votes[k] > (votes[best] if best >= 0 else 0) or (tie_larger and votes[k] > 0 and best >= 0 and votes[k] == votes[best]):
                best = k
    pose = np.zeros(16)
    pose[15] = -1.0
    good = fd.good
    depth = np.zeros(fd.n, F)
    cls = np.where(good, 3, 0).astype(np.uint8)
    err = np.where(good, F(np.inf), F(-1.0)).astype(F)
    if best >= 0:
        R, t = candidates(dec)[best]
        pose[:9], pose[9:12], pose[12:15], pose[15] = R, t, dec["sigma"], float(best)
        r, d, n1, n2 = geometry(R, t, x1, y1, x2, y2, den32)
        with np.errstate(all="ignore"):
            dok = (d > 0) & (d < np.inf)
            Z = np.where(dok, n1 / d, 0.0)
            depth = np.where(good, Z, 0.0).astype(F)
            cls = np.where(~good, 0, np.where(~dok, 3, np.where((n1 > 0) & (n2 > 0), 1, 2))).astype(np.uint8)
            Y = [Z * r[i] + t[i] for i in range(3)]
            ex = ((fx * Y[0]) / Y[2] + cx) - fd.tx.astype(np.float64)
            ey = ((fy * Y[1]) / Y[2] + cy) - fd.ty.astype(np.float64)
            e = np.sqrt(ex * ex + ey * ey).astype(F)
            err = np.where(~good, F(-1.0), np.where(dok & (Y[2] > 0), e, F(np.inf))).astype(F)
    others = sorted((votes[k] for k in range(4) if k != best), reverse=True)
    counts = [int(cover.sum()), votes[best] if best >= 0 else 0, others[0] if best >= 0 else 0, best,
              int((cls == 1).sum()), int((cls == 2).sum()), int((cls == 3).sum()), 0]
    return dict(pose=pose, votes=votes, depth=depth.reshape(h, w), cls=cls.reshape(h, w), err=err.reshape(h, w), counts=counts)


# ---- what the nine numbers mean, and the exact F^ of a known motion (np.linalg is fine here: it is not part of the chain)
def exact_model(h, w, t, rot, fx=None, fy=None, cx=None, cy=None, sign=1.0):
    """The float32 F^ of the camera motion (rot, t) in the header's coordinates, in canonical scale times `sign`."""
    fx = float(max(h, w)) if fx is None else fx
    fy = fx if fy is None else fy
    cx = (w - 1) * 0.5 if cx is None else cx
    cy = (h - 1) * 0.5 if cy is None else cy
    cxF, cyF, s, _ = normalisation(h, w)
    A = np.array([[s * fx, 0.0, s * (cx - cxF)], [0.0, s * fy, s * (cy - cyF)], [0.0, 0.0, 1.0]])
    tx, ty, tz = t
    Em = np.array([[0.0, -tz, ty], [tz, 0.0, -tx], [-ty, tx, 0.0]]) @ E.rotation(rot)
    Ai = np.linalg.inv(A)
    Fh = Ai.T @ Em @ Ai
    big = Fh.reshape(-1)[np.argmax(np.abs(Fh))]
    return (sign * Fh / big).astype(F).reshape(-1)


def camera_flow(h, w, seed, t, rot, fx=None, fy=None, cx=None, cy=None, objects=()):
    """epipolar_ref.rigid_flow's scene seen by a camera with any intrinsics: (flow (h,w,3) float64, the depth map Z, mask)."""
    fx = float(max(h, w)) if fx is None else fx
    fy = fx if fy is None else fy
    cx = (w - 1) * 0.5 if cx is None else cx
    cy = (h - 1) * 0.5 if cy is None else cy
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 4)
    Z = 8.0 + 2.0 * np.sin(2 * np.pi * 1.3 * xs / w + ph[0]) * np.cos(2 * np.pi * 0.9 * ys / h + ph[1]) \
        + 1.5 * np.sin(2 * np.pi * (0.7 * xs / w + 1.1 * ys / h) + ph[2]) + 1.0 * np.cos(2 * np.pi * 2.1 * xs / w + ph[3])
    X = np.stack([(xs - cx) / fx * Z, (ys - cy) / fy * Z, Z], axis=-1)
    Y = X @ E.rotation(rot).T + np.asarray(t, np.float64)
    U, V = fx * Y[..., 0] / Y[..., 2] + cx - xs, fy * Y[..., 1] / Y[..., 2] + cy - ys
    mask = np.zeros((h, w), bool)
    for y0, x0, y1, x1, du, dv in objects:
        U[y0:y1, x0:x1] += du
        V[y0:y1, x0:x1] += dv
        mask[y0:y1, x0:x1] = True
    return np.stack([U, V, np.ones((h, w))], axis=-1), Z, mask


def rotation_error_deg(R, rot):
    """The angle of R R_true^T in degrees."""
    D = np.asarray(R, np.float64).reshape(3, 3) @ E.rotation(rot).T
    skew = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.degrees(math.atan2(skew, 0.5 * (np.trace(D) - 1.0)))
