"""Numpy restatement of the pose refinement (csrc/refine.hip, sam6d_hip.refine), code of its own on top of tests/raster_ref.py's Setup
and tests/verify_ref.py's window_zbuffer.  Per-pixel arithmetic is float32 with one rounding per operation, the sums are Python / int64
integers, the solve is float64 (Python floats: IEEE double, one rounding per operation, math.sqrt correctly rounded).

    view    [fl32(R * scale) | fl32(t)] from the float64 state
    pair    o > 0, |o - r| <= gate, masks[n, y, x] != 0; ray ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1); q = ray o, p = ray r;
            nrm = unit normal of the face's stored vertices through the view, towards the camera; e = nrm . (q - p) * inv_unit;
            c = (q - t) * inv_unit, dropped unless |c|^2 <= 256 and |e| <= 16; J = (c x nrm, nrm)
    sums    u = (J, e): acc[k] = sum rint(u_i u_j 2^30) over the upper triangle of the 7 x 7 matrix, row-major; acc[28] = pairs
    solve   A_ii += damping A_ii, Cholesky, xi = (omega, v); R <- Cayley(omega) R, t <- t + v / inv_unit
    status  0 stepped, 1 too few pairs, 2 singular, 3 step refused, 4 no window
"""
import math

import numpy as np

from tests import raster_ref as RR
from tests import verify_ref as VR

F32 = np.float32
F64 = np.float64
S = 30
BOUND = F32(16.0)
WORDS = [(i, j) for i in range(7) for j in range(i, 7)]  # word k of acc


def view_of(state, scale):
    """(3,4) float32 from one pose's twelve float64"""
    s = np.asarray(state, F64)
    return np.concatenate([(s[:9].reshape(3, 3) * F64(F32(scale))).astype(F32), s[9:].astype(F32).reshape(3, 1)], axis=1)


def pairs(vert, faces, M, intr, size, near, win, depth, mask, gate, inv_unit):
    """u (P,7) float32 = (J0 .. J5, e) of the pairs of one pose with view M in the window win = (x0, y0, bw, bh)"""
    fx, fy, cx, cy = (F32(v) for v in intr)
    H, W = size
    s = RR.Setup(vert, faces, M, fx, fy, cx, cy, near, H, W)
    zb = VR.window_zbuffer(s, win)
    ys, xs = np.nonzero(zb != RR.EMPTY)
    if ys.size == 0:
        return np.zeros((0, 7), F32)
    keys = zb[ys, xs]
    r = VR.key_depth(keys)
    f = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ys, xs = ys + win[1], xs + win[0]
    o = np.asarray(depth, F32)[ys, xs]
    iu, gate = F32(inv_unit), F32(gate)
    with np.errstate(all="ignore"):
        ok = (o > 0) & (np.abs(o - r) <= gate)
        if mask is not None:
            ok &= np.asarray(mask)[ys, xs] != 0
        rx = ((xs.astype(F32) + F32(0.5)) - cx) / fx
        ry = ((ys.astype(F32) + F32(0.5)) - cy) / fy
        q = [rx * o, ry * o, o]
        p = [rx * r, ry * r, r]
        P = s.P[f]  # (P, vertex, coordinate), stored order
        a = [P[:, 1, k] - P[:, 0, k] for k in range(3)]
        b = [P[:, 2, k] - P[:, 0, k] for k in range(3)]
        m = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        l = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        ok &= l > 0
        n = [m[k] / l for k in range(3)]
        away = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2] > 0
        n = [np.where(away, -c, c) for c in n]
        d = [q[k] - p[k] for k in range(3)]
        e = ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) * iu
        M = np.asarray(M, F32).reshape(3, 4)
        c = [(q[k] - M[k, 3]) * iu for k in range(3)]
        ok &= ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2] <= BOUND * BOUND) & (np.abs(e) <= BOUND)
        J = [c[1] * n[2] - c[2] * n[1], c[2] * n[0] - c[0] * n[2], c[0] * n[1] - c[1] * n[0]]
    u = np.stack(J + n + [e], axis=1)
    assert u.dtype == F32
    return u[ok]


def sums(u):
    """acc (32) int64 of the pairs u (P,7)"""
    acc = np.zeros(32, np.int64)
    d = u.astype(F64)
    for k, (i, j) in enumerate(WORDS):
        acc[k] = np.rint(d[:, i] * d[:, j] * F64(2.0 ** S)).astype(np.int64).sum()
    acc[28] = len(u)
    return acc


def solve(acc, state, damping, min_pairs, max_step, inv_unit):
    """-> (status, new state (12) float64) from one pose's sums; the window is not empty"""
    if int(acc[28]) < min_pairs:
        return 1, state
    inv = 1.0 / 2.0 ** S
    word = {ij: k for k, ij in enumerate(WORDS)}
    L = [[float(int(acc[word[(j, i)]])) * inv if j <= i else 0.0 for j in range(6)] for i in range(6)]
    g = [float(int(acc[word[(i, 6)]])) * inv for i in range(6)]
    damping = float(damping)
    for i in range(6):
        L[i][i] = L[i][i] + damping * L[i][i]
    for j in range(6):
        s = L[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return 2, state
        d = math.sqrt(s)
        L[j][j] = d
        for i in range(j + 1, 6):
            t = L[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / d
    x = [0.0] * 6
    for i in range(6):
        t = g[i]
        for k in range(i):
            t = t - L[i][k] * x[k]
        x[i] = t / L[i][i]
    for i in range(5, -1, -1):
        t = x[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * x[k]
        x[i] = t / L[i][i]
    step2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]
    max_step = float(max_step)
    if not step2 <= max_step * max_step:
        return 3, state
    w = [x[0] * 0.5, x[1] * 0.5, x[2] * 0.5]
    s = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    k = 2.0 / (1.0 + s)
    X = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    C = [[(1.0 if i == j else 0.0) + k * (X[i][j] + ((w[i] * w[j] - s) if i == j else w[i] * w[j])) for j in range(3)] for i in range(3)]
    R = [float(v) for v in state[:9]]
    unit = 1.0 / float(F32(inv_unit))
    new = np.array(state, F64)
    for i in range(3):
        for j in range(3):
            new[i * 3 + j] = (C[i][0] * R[j] + C[i][1] * R[3 + j]) + C[i][2] * R[6 + j]
        new[9 + i] = float(state[9 + i]) + x[3 + i] * unit
    return 0, new


def step(vert, faces, state, scale, intr, size, near, box, depth, masks, gate, inv_unit, damping, min_pairs, max_step):
    """sam6d_pose_refine_step -> state (N,12) float64, acc (N,32) int64, stats (N,4) int32"""
    state = np.array(state, F64).reshape(-1, 12)
    N = len(state)
    acc = np.zeros((N, 32), np.int64)
    stats = np.zeros((N, 4), np.int32)
    total = VR.areas(box, size).sum()
    for n in range(N):
        win = VR.clamp_box(box[n], size)
        if total > 0 and win[2] > 0:
            u = pairs(vert, faces, view_of(state[n], scale), intr, size, near, win, depth, None if masks is None else masks[n], gate, inv_unit)
            acc[n] = sums(u)
        status = 4
        if win[2] > 0:
            status, state[n] = solve(acc[n], state[n].copy(), damping, min_pairs, max_step, inv_unit)
        see = int(acc[n, 27]) & 0xFFFFFFFFFFFFFFFF
        stats[n] = np.array([acc[n, 28], status, see & 0xFFFFFFFF, see >> 32], np.uint32).view(np.int32)
    return state, acc, stats


def radius2(vert):
    v = np.asarray(vert, F32)
    return ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).max()


def inv_unit_of(vert, scale=1.0):
    """what sam6d_hip.refine passes: float32(1 / (sqrt(max |v|^2) * |scale|))"""
    return F32(1.0 / (math.sqrt(float(radius2(vert))) * abs(float(F32(scale)))))


def grow(box, margin, size):
    H, W = size
    out = np.array(box, np.int32)
    for b in out:
        if b[2] >= b[0] and b[3] >= b[1]:
            b[:] = [max(b[0] - margin, 0), max(b[1] - margin, 0), min(b[2] + margin, W - 1), min(b[3] + margin, H - 1)]
        else:
            b[:] = [0, 0, -1, -1]
    return out


def rms_of(stats, inv_unit):
    st = np.asarray(stats).view(np.uint32).astype(np.int64)
    see = ((st[:, 3] << 32) | st[:, 2]).astype(F64) * F64(2.0 ** -S)
    unit = 1.0 / float(F32(inv_unit))
    rms = np.sqrt(see / np.maximum(st[:, 0].astype(F64), 1.0)) * unit
    return np.where(st[:, 0] > 0, rms, 0.0).astype(F32)


def refine(vert, faces, R, t, intr, size, depth, masks=None, iters=5, gate=0.02, margin=8, damping=1e-6, min_pairs=32, max_step=math.inf,
           scale=1.0, near=1e-3):
    """sam6d_hip.refine.refine_poses -> dict(R, t, n_pairs, rms, status, history, boxes)"""
    R, t = np.asarray(R, F32), np.asarray(t, F32)
    N = len(R)
    view0 = np.concatenate([R * F32(scale), t[:, :, None]], axis=2)
    box = grow(VR.windows(vert, faces, view0, intr, size, near)[0], margin, size)
    iu = inv_unit_of(vert, scale)
    state = np.concatenate([R.reshape(N, 9), t], axis=1).astype(F64)
    history = np.zeros((N, iters, 2), F32)
    for it in range(iters):
        state, acc, stats = step(vert, faces, state, scale, intr, size, near, box, depth, masks, gate, iu, damping, min_pairs, max_step)
        history[:, it, 0] = stats[:, 0].astype(F32)
        history[:, it, 1] = rms_of(stats, iu)
    return dict(R=state[:, :9].astype(F32).reshape(N, 3, 3), t=state[:, 9:].astype(F32), n_pairs=stats[:, 0].copy(), rms=history[:, -1, 1].copy(),
                status=stats[:, 1].copy(), history=history, boxes=box, state=state, acc=acc)


# ---------------------------------------------------------------------------------------------- scenes for the tests
BIG = (96, 128)
BIG_INTR = (120.0, 120.0, 64.0, 48.0)
TRUE = VR.pose((0.1, -0.05, 4.0))
STARTS = {"near": (0.05, (0.03, -0.02, 0.05)), "far": (0.15, (0.08, -0.05, 0.1))}
GATE = 0.3


def mesh_a():
    """the octahedron with its six vertices at different distances: no symmetry, so depth alone fixes the pose"""
    v, f = RR.octahedron()
    return (v * np.array([1.0, 0.6, 0.8, 0.5, 0.7, 0.9], F32)[:, None]).astype(F32), f


def mesh_b():
    """icosphere(2), 320 faces, every vertex moved along its radius by a smooth bump"""
    v, f = RR.icosphere(2)
    d = v.astype(F64)
    bump = 1.0 + 0.12 * np.sin(5.0 * d[:, 0] + 1.0) * np.cos(4.0 * d[:, 1] - 0.5) + 0.08 * d[:, 2]
    return (d * bump[:, None]).astype(F32), f


def start(name, true=TRUE):
    """(R (3,3), t (3)) float32: the true pose turned about (3, -1, 2) and shifted"""
    angle, shift = STARTS[name]
    true = np.asarray(true, F64)
    return (VR.rotation((3.0, -1.0, 2.0), angle) @ true[:, :3]).astype(F32), (true[:, 3] + np.asarray(shift)).astype(F32)


def five_starts():
    """VR.five_poses (inside; straddling the right and bottom borders; through the camera plane; off-screen; behind the camera), each
    turned about (3, -1, 2) by 0.05 rad and shifted by (0.03, -0.02, 0.05) -> R (5,3,3), t (5,3) float32"""
    Rs, ts = zip(*[start("near", M) for M in VR.five_poses()])
    return np.stack(Rs), np.stack(ts)
