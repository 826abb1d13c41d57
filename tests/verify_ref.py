"""Numpy restatement of the pose check (csrc/verify.hip, sam6d_hip.verify), code of its own on top of tests/raster_ref.py's Setup:
windows, per-pose z-buffers, classification, composite and the picture.  Everything is integer or float32 with one rounding per
operation.

    window   box[n] = min x0, y0 and max x1, y1 over the live faces whose image-clamped pixel box is not empty, else [0, 0, -1, -1]
    z-buffer per pose, bh x bw words: every face's box clamped to the window, key = bits(depth) << 32 | face, the minimum wins
    classify r = the float of the key's upper half, o = depth_obs[y, x]: unknown when not (o > 0); e = o - r; behind e > tau,
             occluded e < -tau, else inlier; inter when masks[n, y, x] != 0
    composite key = bits(r) << 32 | n, the minimum wins; ids = lower half (-1 empty), depth_out = float of the upper half (0 empty)
    picture  id outside [0, N) -> -1; id >= 0: (rgb * (256 - alpha) + color * alpha + 128) >> 8, or color where a 4-neighbour inside
             the image has another id; id = -1: rgb
"""
import numpy as np

from tests import raster_ref as RR

F32 = np.float32
EMPTY = RR.EMPTY
INLIER, OCCLUDED, BEHIND, UNKNOWN = 1, 2, 3, 4
COLUMNS = ("n_render", "n_inlier", "n_occluded", "n_behind", "n_unknown", "n_mask", "n_inter", "n_dropped")


def _setups(vert, faces, view, intr, size, near):
    fx, fy, cx, cy = intr
    H, W = size
    return [RR.Setup(vert, faces, M, fx, fy, cx, cy, near, H, W) for M in np.asarray(view, F32).reshape(-1, 3, 4)]


def windows(vert, faces, view, intr, size, near=1e-3):
    """-> box (N,4) int32 [x0, y0, x1, y1] inclusive, n_dropped (N) int32"""
    setups = _setups(vert, faces, view, intr, size, near)
    box = np.zeros((len(setups), 4), np.int32)
    dropped = np.zeros(len(setups), np.int32)
    for n, s in enumerate(setups):
        boxed = s.live & (s.x0 <= s.x1) & (s.y0 <= s.y1)
        dropped[n] = s.dropped.sum()
        box[n] = [s.x0[boxed].min(), s.y0[boxed].min(), s.x1[boxed].max(), s.y1[boxed].max()] if boxed.any() else [0, 0, -1, -1]
    return box, dropped


def clamp_box(b, size):
    """(x0, y0, bw, bh) of a box clamped to the image; 0 x 0 when empty"""
    H, W = size
    x0, y0, x1, y1 = max(int(b[0]), 0), max(int(b[1]), 0), min(int(b[2]), W - 1), min(int(b[3]), H - 1)
    bw, bh = max(x1 - x0 + 1, 0), max(y1 - y0 + 1, 0)
    return (x0, y0, 0, 0) if bw == 0 or bh == 0 else (x0, y0, bw, bh)


def areas(box, size):
    return np.array([clamp_box(b, size)[2] * clamp_box(b, size)[3] for b in box], np.int64)


def window_zbuffer(s, win):
    """the (bh, bw) uint64 keys of one pose (s: its Setup) in the window win = (x0, y0, bw, bh)"""
    wx0, wy0, bw, bh = win
    zb = np.full((bh, bw), EMPTY, np.uint64)
    if bw == 0:
        return zb
    x0, y0 = np.maximum(s.x0, wx0), np.maximum(s.y0, wy0)
    x1, y1 = np.minimum(s.x1, wx0 + bw - 1), np.minimum(s.y1, wy0 + bh - 1)
    for f in np.nonzero(s.live & (x0 <= x1) & (y0 <= y1))[0]:
        ys, xs = np.mgrid[y0[f]:y1[f] + 1, x0[f]:x1[f] + 1]
        w = s.edges(f, 256 * xs + 128, 256 * ys + 128)
        cover = (w[0] + s.bias[f, 0] >= 0) & (w[1] + s.bias[f, 1] >= 0) & (w[2] + s.bias[f, 2] >= 0)
        if not cover.any():
            continue
        d, _ = s.weights(f, w)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sl = (slice(y0[f] - wy0, y1[f] + 1 - wy0), slice(x0[f] - wx0, x1[f] + 1 - wx0))
        zb[sl] = np.minimum(zb[sl], np.where(cover, key, EMPTY))
    return zb


def key_depth(keys):
    """the float32 whose bits are the upper half of each key"""
    return (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32).view(F32)


def window_depth(zb):
    """the window's depth image: 0 where the word is empty"""
    return np.where(zb != EMPTY, key_depth(zb), F32(0))


def classify(r, o, tau):
    """class codes of rendered depths r against observed depths o (float32 arrays of one shape)"""
    r, o, tau = np.asarray(r, F32), np.asarray(o, F32), F32(tau)
    with np.errstate(all="ignore"):
        e = o - r
        cls = np.where(e > tau, BEHIND, np.where(e < -tau, OCCLUDED, INLIER))
        return np.where(o > 0, cls, UNKNOWN).astype(np.int32)


def pose_verify(vert, faces, view, intr, size, near, box, depth_obs, masks, tau):
    """sam6d_pose_verify -> counts (N,8) int32, ids (H,W) int32, depth_out (H,W) float32"""
    H, W = size
    setups = _setups(vert, faces, view, intr, size, near)
    N = len(setups)
    counts = np.zeros((N, 8), np.int32)
    comp = np.full((H, W), EMPTY, np.uint64)
    depth_obs = np.asarray(depth_obs, F32)
    if areas(box, size).sum() > 0:  # total == 0: zeros and background, no pass runs
        for n, s in enumerate(setups):
            x0, y0, bw, bh = clamp_box(box[n], size)
            zb = window_zbuffer(s, (x0, y0, bw, bh))
            hit = zb != EMPTY
            r = key_depth(zb)
            sl = (slice(y0, y0 + bh), slice(x0, x0 + bw))
            cls = classify(r, depth_obs[sl], tau)
            counts[n, 0] = hit.sum()
            for c in (INLIER, OCCLUDED, BEHIND, UNKNOWN):
                counts[n, c] = (hit & (cls == c)).sum()
            if masks is not None:
                counts[n, 5] = np.count_nonzero(masks[n])
                counts[n, 6] = (hit & (np.asarray(masks[n])[sl] != 0)).sum()
            counts[n, 7] = s.dropped.sum()
            key = (zb & np.uint64(0xFFFFFFFF00000000)) | np.uint64(n)
            comp[sl] = np.minimum(comp[sl], np.where(hit, key, EMPTY))
    empty = comp == EMPTY
    ids = np.where(empty, -1, (comp & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth_out = np.where(empty, F32(0), key_depth(comp)).astype(F32)
    return counts, ids, depth_out


def ratios(counts):
    """inlier, behind, occluded, unknown ratios: float32 true division by n_render, 0 where that is 0"""
    c = np.asarray(counts)
    n = c[:, 0].astype(F32)
    with np.errstate(all="ignore"):
        return {k: np.where(c[:, 0] > 0, c[:, col].astype(F32) / n, F32(0)).astype(F32)
                for k, col in (("inlier_ratio", 1), ("behind_ratio", 3), ("occluded_ratio", 2), ("unknown_ratio", 4))}


def mask_iou(counts):
    c = np.asarray(counts)
    union = c[:, 0] + c[:, 5] - c[:, 6]
    with np.errstate(all="ignore"):
        return np.where(union > 0, c[:, 6].astype(F32) / union.astype(F32), F32(0)).astype(F32)


# ---------------------------------------------------------------------------------------------- scenes for the tests
INTR = (60.0, 60.0, 32.0, 24.0)  # a unit sphere four units away is a disc of radius 15 pixels
SIZE = (48, 64)


def rotation(axis, angle):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(t, axis=(1.0, 2.0, 3.0), angle=0.7):
    """(3,4) float32: a rotation about `axis` and the translation t"""
    return np.concatenate([rotation(axis, angle), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F32)


def five_poses():
    """inside the image; straddling the right and bottom borders; straddling the camera plane (faces dropped, the rest boxed); wholly
    off-screen; wholly behind the camera"""
    return np.stack([pose((0.1, -0.05, 4.0)), pose((1.9, 1.4, 4.0)), pose((0.0, 0.0, 0.5)), pose((10.0, 0.0, 4.0)), pose((0.0, 0.0, -4.0))])


def render_depth(vert, faces, M, intr, size, near=1e-3):
    """(mask == 255, depth) of raster_ref.render_view for one view"""
    H, W = size
    out = RR.render_view(vert, faces, None, None, M, np.zeros(3, F32), *intr, H, W, near, 0.05, False, np.zeros(4096, np.uint8))
    return out["mask"] == 255, out["depth"]


def overlay_instances(rgb, ids, colors, alpha):
    """sam6d_overlay_instances -> canvas (H, 2W, 3) uint8"""
    rgb, colors = np.asarray(rgb, np.uint8), np.asarray(colors, np.uint8)
    H, W = rgb.shape[:2]
    N = len(colors)
    ids = np.asarray(ids, np.int64)
    idn = np.where((ids >= 0) & (ids < N), ids, -1)
    edge = np.zeros((H, W), bool)
    edge[1:] |= idn[1:] != idn[:-1]
    edge[:-1] |= idn[:-1] != idn[1:]
    edge[:, 1:] |= idn[:, 1:] != idn[:, :-1]
    edge[:, :-1] |= idn[:, :-1] != idn[:, 1:]
    col = colors[np.maximum(idn, 0)].astype(np.int64)
    blend = (rgb.astype(np.int64) * (256 - int(alpha)) + col * int(alpha) + 128) >> 8
    right = np.where((idn >= 0)[..., None], np.where(edge[..., None], col, blend), rgb.astype(np.int64)).astype(np.uint8)
    return np.concatenate([rgb, right], axis=1)
