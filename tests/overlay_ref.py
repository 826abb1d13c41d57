"""Numpy restatements of the recipes at the top of csrc/overlay.hip, written to share neither the device's data flow nor its visiting
order: the pose overlay is a SEQUENTIAL painter (instances, stages and primitives in the reference's order, each primitive's predicate
evaluated over all pixels of the image and assigned; no keys, no maximum, no walk), the mask overlay takes its dilation from
scipy.ndimage.binary_dilation itself."""
import numpy as np
from scipy import ndimage

GROUND = ((4, 5), (5, 7), (6, 4), (7, 6))
PILLARS = ((0, 4), (1, 5), (2, 6), (3, 7))
TOP = ((0, 1), (1, 3), (2, 0), (3, 2))
COORD_LO, COORD_HI = np.float32(-8192.0), np.float32(8191.0)


def grey(rgb):
    """OpenCV's published 8-bit RGB2GRAY fixed point (restated; cv2 is not pinned)"""
    c = rgb.astype(np.int64)
    return (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14


def edge0(mask):
    """mask pixels with at least one 4-neighbour inside the image that is not mask"""
    m = np.asarray(mask) != 0
    out = np.zeros_like(m)
    out[1:, :] |= m[1:, :] & ~m[:-1, :]
    out[:-1, :] |= m[:-1, :] & ~m[1:, :]
    out[:, 1:] |= m[:, 1:] & ~m[:, :-1]
    out[:, :-1] |= m[:, :-1] & ~m[:, 1:]
    return out


def mask_edge(mask):
    return ndimage.binary_dilation(edge0(mask), np.ones((2, 2)))


def overlay_masks(rgb, masks, lut, draw_edge=True):
    """rgb (H,W,3) u8, masks (M,H,W), lut (M,3,256) u8 -> canvas (H,2W,3) u8"""
    g = grey(rgb)
    out = np.stack([g, g, g], axis=-1).astype(np.uint8)
    edge = np.zeros(g.shape, bool)
    for m in range(len(masks)):
        inside = np.asarray(masks[m]) != 0
        for c in range(3):
            out[inside, c] = lut[m][c][g[inside]]
        if draw_edge:
            edge |= mask_edge(inside)
    out[edge, :] = 255
    return np.concatenate([rgb, out], axis=1)


def project(R, t, K, p):
    """The fp32 projection of the recipe for points p (n,3): (u, v) int32 and kept (bool); u, v are 0 where skipped."""
    f = np.float32
    R, t, K, p = (np.asarray(a, dtype=f) for a in (R, t, K, p))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        P = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
        q = [(K[r, 0] * P[0] + K[r, 1] * P[1]) + K[r, 2] * P[2] for r in range(3)]
        front = q[2] > 0
        uf, vf = q[0] / q[2], q[1] / q[2]
        keep = front & (uf >= COORD_LO) & (uf <= COORD_HI) & (vf >= COORD_LO) & (vf <= COORD_HI)
    u = np.where(keep, uf, 0).astype(np.int32)  # astype truncates toward zero
    v = np.where(keep, vf, 0).astype(np.int32)
    return u, v, keep


def in_line(ax, ay, bx, by, T, xx, yy):
    """the thick-line predicate at the int64 pixel grids xx, yy"""
    ax, ay, bx, by, T = (np.int64(v) for v in (ax, ay, bx, by, T))
    dx, dy = bx - ax, by - ay
    wx, wy = xx - ax, yy - ay
    L2 = dx * dx + dy * dy
    s = wx * dx + wy * dy
    cap_a = 4 * (wx * wx + wy * wy) <= T * T
    ex, ey = xx - bx, yy - by
    cap_b = 4 * (ex * ex + ey * ey) <= T * T
    cr = dx * wy - dy * wx
    band = 4 * (cr * cr) <= T * T * L2
    return np.where(s <= 0, cap_a, np.where(s >= L2, cap_b, band))


def in_disc(cx, cy, r, xx, yy):
    dx, dy = xx - np.int64(cx), yy - np.int64(cy)
    return dx * dx + dy * dy <= np.int64(r) * np.int64(r)


def shades(color):
    c = [int(v) for v in color]
    return [tuple(int(v * 0.3) for v in c), tuple(int(v * 0.6) for v in c), tuple(c), tuple(c)]


def _window(H, W, x0, x1, y0, y1, pad, window):
    if not window:
        return 0, H, 0, W
    return max(min(y0, y1) - pad, 0), min(max(y0, y1) + pad + 1, H), max(min(x0, x1) - pad, 0), min(max(x0, x1) + pad + 1, W)


def draw_detections(rgb, R, t, K, box, pts, colors, thickness=3, radius=1, window=False):
    """The sequential painter.  -> (canvas (H,2W,3) u8, n_skipped (N) int32).  window=True evaluates a primitive's predicate on its
    own neighbourhood only (the same pixels are accepted; for timing, not for the tests)."""
    H, W = rgb.shape[:2]
    img = rgb.copy()
    N = len(R)
    colors = np.broadcast_to(np.asarray(colors), (N, 3))
    skipped = np.zeros(N, np.int32)
    YY, XX = np.mgrid[0:H, 0:W].astype(np.int64)
    for i in range(N):
        sh = shades(colors[i])
        cu, cv, ck = project(R[i], t[i], K[i], box)
        for stage, edges in enumerate((GROUND, PILLARS, TOP)):
            for a, b in edges:
                if not (ck[a] and ck[b]):
                    skipped[i] += 1
                    continue
                y0, y1, x0, x1 = _window(H, W, cu[a], cu[b], cv[a], cv[b], thickness + 2, window)
                if y0 >= y1 or x0 >= x1:
                    continue
                hit = in_line(cu[a], cv[a], cu[b], cv[b], thickness, XX[y0:y1, x0:x1], YY[y0:y1, x0:x1])
                img[y0:y1, x0:x1][hit] = sh[stage]
        if len(pts):
            pu, pv, pk = project(R[i], t[i], K[i], pts)
            skipped[i] += int((~pk).sum())
            for j in np.nonzero(pk)[0]:
                y0, y1, x0, x1 = _window(H, W, pu[j], pu[j], pv[j], pv[j], radius + 1, window)
                if y0 >= y1 or x0 >= x1:
                    continue
                hit = in_disc(pu[j], pv[j], radius, XX[y0:y1, x0:x1], YY[y0:y1, x0:x1])
                img[y0:y1, x0:x1][hit] = sh[3]
    return np.concatenate([rgb, img], axis=1), skipped
