"""Numpy restatement of the template rasteriser (csrc/raster.hip, sam6d_hip.onboard.render_views), code of its own: the recipe at the
top of raster.hip, float32 operation by operation in the order written there, int64 edge functions, and a z-buffer of uint64 keys
reduced with np.minimum.  Every float array here is float32 and every constant is wrapped in np.float32, so numpy rounds each
operation once, as the device does without fused multiply-adds.

    P_r   = ((M[r,0]*x + M[r,1]*y) + M[r,2]*z) + M[r,3]
    drop  : an index outside [0, V) or not (P_z >= near)
    X     = int(floor(clamp((f * (P_x / P_z) + c) * 256, -2^24, 2^24) + 0.5))       (1/256 pixel; centre of pixel j at 256 j + 128)
    area2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0); 0 covers nothing, < 0 swaps vertices 1 and 2
    E_ab(p) = (bx-ax)(py-ay) - (by-ay)(px-ax); covered: E > 0, or E == 0 and (by < ay or (by == ay and bx > ax))
    q_i = float(w_i) / z_i, qs = (q0 + q1) + q2, depth = float(area2) / qs, l_i = q_i / qs
    key = bits(depth) << 32 | face, the minimum wins
"""
import numpy as np

F32 = np.float32
GAIN = F32(25.330296)
LIMIT = F32(16777216.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _row(M, r, x, y, z):
    return ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]


def _snap(f, a, z, c):
    u = (f * (a / z) + c) * F32(256.0)
    u = np.where(u >= -LIMIT, u, -LIMIT)
    u = np.where(u <= LIMIT, u, LIMIT)
    return np.floor(u + F32(0.5)).astype(np.int64)


def _owner(ax, ay, bx, by):
    return np.where((by < ay) | ((by == ay) & (bx > ax)), 0, -1).astype(np.int64)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


class Setup:
    """Per-face values of one view, arrays over the F faces (vertex order after the winding swap)."""

    def __init__(self, vert, faces, M, fx, fy, cx, cy, near, H, W):
        vert = np.asarray(vert, F32)
        faces = np.asarray(faces, np.int64)
        M = np.asarray(M, F32).reshape(3, 4)
        V = vert.shape[0]
        inside = ((faces >= 0) & (faces < V)).all(axis=1)
        safe = np.where(inside[:, None], faces, 0)
        p = vert[safe]  # (F,3 vertices,3 coordinates)
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        with np.errstate(all="ignore"):
            self.P = np.stack([_row(M, r, x, y, z) for r in range(3)], axis=-1)  # camera space, stored order
            pz = self.P[..., 2]
            ok = inside & (pz >= F32(near)).all(axis=1)
            X = _snap(F32(fx), self.P[..., 0], pz, F32(cx))
            Y = _snap(F32(fy), self.P[..., 1], pz, F32(cy))
        a2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        self.dropped = ~ok
        self.swapped = ok & (a2 < 0)
        order = np.where(self.swapped[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
        rows = np.arange(faces.shape[0])[:, None]
        self.X, self.Y, self.z = X[rows, order], Y[rows, order], pz[rows, order]
        self.area2 = np.abs(a2)
        self.live = ok & (a2 != 0)
        X, Y = self.X, self.Y
        self.bias = np.stack([_owner(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2]), _owner(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0]),
                              _owner(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1])], axis=1)
        self.x0 = np.maximum((X.min(axis=1) + 127) >> 8, 0)
        self.x1 = np.minimum((X.max(axis=1) - 128) >> 8, W - 1)
        self.y0 = np.maximum((Y.min(axis=1) + 127) >> 8, 0)
        self.y1 = np.minimum((Y.max(axis=1) - 128) >> 8, H - 1)

    def edges(self, f, px, py):
        """w0, w1, w2 of faces f (scalar or array) at the sub-pixel points px, py (int64, broadcast against f)"""
        X, Y = self.X[f], self.Y[f]
        return (_edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], px, py), _edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], px, py),
                _edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], px, py))

    def weights(self, f, w):
        """depth and the perspective-correct weights (swapped order) from the edge values"""
        z = self.z[f]
        with np.errstate(all="ignore"):
            q = [w[k].astype(F32) / z[..., k] for k in range(3)]
            qs = (q[0] + q[1]) + q[2]
            return np.asarray(self.area2[f]).astype(F32) / qs, [q[k] / qs for k in range(3)]


def _mix(l, a0, a1, a2):
    return (l[0] * a0 + l[1] * a1) + l[2] * a2


def render_view(vert, faces, normals, colors, M, light, fx, fy, cx, cy, H, W, near, base_color, colorize, lut):
    vert = np.asarray(vert, F32)
    faces = np.asarray(faces, np.int64)
    M = np.asarray(M, F32).reshape(3, 4)
    s = Setup(vert, faces, M, fx, fy, cx, cy, near, H, W)
    zb = np.full((H, W), EMPTY, np.uint64)
    for f in np.nonzero(s.live & (s.x0 <= s.x1) & (s.y0 <= s.y1))[0]:
        ys, xs = np.mgrid[s.y0[f]:s.y1[f] + 1, s.x0[f]:s.x1[f] + 1]
        w = s.edges(f, 256 * xs + 128, 256 * ys + 128)
        cover = (w[0] + s.bias[f, 0] >= 0) & (w[1] + s.bias[f, 1] >= 0) & (w[2] + s.bias[f, 2] >= 0)
        if not cover.any():
            continue
        d, _ = s.weights(f, w)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sl = (slice(s.y0[f], s.y1[f] + 1), slice(s.x0[f], s.x1[f] + 1))
        zb[sl] = np.minimum(zb[sl], np.where(cover, key, EMPTY))
    out = dict(mask=np.zeros((H, W), np.uint8), face=np.full((H, W), -1, np.int32), depth=np.zeros((H, W), F32),
               xyz=np.zeros((H, W, 3), F32), rgb=np.zeros((H, W, 3), np.uint8), n_dropped=np.int32(s.dropped.sum()))
    ys, xs = np.nonzero(zb != EMPTY)
    if ys.size == 0:
        return out
    f = (zb[ys, xs] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    w = s.edges(f, 256 * xs + 128, 256 * ys + 128)
    d, l = s.weights(f, w)
    sw = s.swapped[f]
    m = [l[0], np.where(sw, l[2], l[1]), np.where(sw, l[1], l[2])]  # the stored vertex order
    fv = faces[f]
    out["mask"][ys, xs] = 255
    out["face"][ys, xs] = f
    out["depth"][ys, xs] = d
    out["xyz"][ys, xs] = np.stack([_mix(m, vert[fv[:, 0], k], vert[fv[:, 1], k], vert[fv[:, 2], k]) for k in range(3)], axis=1)
    # ---- shading
    P = s.P[f]  # (n, vertex, coordinate)
    Pc = [_mix(m, P[:, 0, k], P[:, 1, k], P[:, 2, k]) for k in range(3)]
    if normals is not None:
        normals = np.asarray(normals, F32)
        no = [_mix(m, normals[fv[:, 0], k], normals[fv[:, 1], k], normals[fv[:, 2], k]) for k in range(3)]
        n = [(M[k, 0] * no[0] + M[k, 1] * no[1]) + M[k, 2] * no[2] for k in range(3)]
    else:
        e1 = [P[:, 1, k] - P[:, 0, k] for k in range(3)]
        e2 = [P[:, 2, k] - P[:, 0, k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    facing = (n[0] * Pc[0] + n[1] * Pc[1]) + n[2] * Pc[2]
    n = [np.where(facing > 0, -c, c) for c in n]
    light = np.asarray(light, F32)
    L = [light[k] - Pc[k] for k in range(3)]
    d2 = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    ndl = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]
    with np.errstate(all="ignore"):
        cs = ndl / (np.sqrt(nn) * np.sqrt(d2))
        cs = np.where(cs > 0, cs, F32(0))
        v = GAIN * cs / d2
    grey = bool(colorize) or colors is None
    for k in range(3):
        if grey:
            alb = F32(base_color)
        else:
            c = np.asarray(colors, np.uint8)
            alb = _mix(m, c[fv[:, 0], k].astype(F32) / F32(255), c[fv[:, 1], k].astype(F32) / F32(255), c[fv[:, 2], k].astype(F32) / F32(255))
        with np.errstate(all="ignore"):
            lin = alb * v
        lin = np.where(lin > 0, lin, F32(0))
        lin = np.where(lin < 1, lin, F32(1))
        out["rgb"][ys, xs, k] = np.asarray(lut)[(lin * F32(4095) + F32(0.5)).astype(np.int64)]
    assert all(a.dtype == F32 for a in (d, v, Pc[0], n[0]))
    return out


def render(vert, faces, normals, colors, view, light, intrinsics, size, near, base_color, colorize, lut):
    """T views: the dict of sam6d_hip.onboard.render_views in numpy"""
    fx, fy, cx, cy = intrinsics
    H, W = size
    per = [render_view(vert, faces, normals, colors, view[t], light[t], fx, fy, cx, cy, H, W, near, base_color, colorize, lut)
           for t in range(len(view))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


# ---------------------------------------------------------------------------------------------- meshes for the tests
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def icosphere(level, radius=1.0):
    """an icosahedron subdivided `level` times (20 * 4^level faces), vertices on the sphere of `radius`"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(F32), np.array(f, np.int32)
