"""Numpy restatement of the surface sampler (csrc/meshsample.hip, sam6d_hip.onboard.sample_surface), code of its own: float32 areas
in source order, integer weights, a uint64 cumulative sum, keys from tests/choice_ref.py's hash and np.searchsorted.

    area[f]   = sqrt((cx*cx + cy*cy) + cz*cz) * 0.5,  c = (v1 - v0) x (v2 - v0); 0 for an index outside [0, V) or a NaN
    weight[f] = 0 where area is 0, else max(1, min(2^24, floor(area / area_max * 2^24)))
    start     = exclusive prefix sum, total = sum
    a = fmix(seed ^ 0x9E3779B9), b = fmix(a + 0x4D455348), h(r) = fmix(fmix(r ^ b) + a)
    sample g = row + j:  u = (h(3g) * total) >> 32, face = last f with start[f] <= u,
                         r1 = (h(3g+1) >> 8) / 2^24, r2 = (h(3g+2) >> 8) / 2^24, both reflected (1 - r) where r1 + r2 > 1,
                         point = (v0 + r1 * (v1 - v0)) + r2 * (v2 - v0)
"""
import numpy as np

from tests.choice_ref import M32, fmix

F32 = np.float32
SALT = 0x4D455348


def keys(seed, r):
    a = fmix(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9))
    b = fmix((a + np.uint64(SALT)) & M32)
    r = np.asarray(r, dtype=np.uint64) & M32
    return fmix((fmix(r ^ b) + a) & M32)


def areas(vert, faces):
    vert = np.asarray(vert, F32)
    faces = np.asarray(faces, np.int64)
    inside = ((faces >= 0) & (faces < vert.shape[0])).all(axis=1)
    p = vert[np.where(inside[:, None], faces, 0)]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        ar = np.sqrt((cx * cx + cy * cy) + cz * cz) * F32(0.5)
    ar = np.where(inside & (ar > 0), ar, F32(0))
    assert ar.dtype == F32
    return ar


def weights(area):
    amax = area.max()
    if not (amax > 0 and np.isfinite(amax)):
        raise ValueError("every face has zero area")
    with np.errstate(all="ignore"):
        r = area / amax * F32(16777216.0)
    r = np.where(r >= 1, r, F32(1))
    r = np.where(r <= F32(16777216.0), r, F32(16777216.0))
    return np.where(area > 0, np.floor(r).astype(np.uint64), np.uint64(0))


def sample(vert, faces, n, seed=0, row=0):
    """points (n,3) float32, face (n,) int32"""
    vert = np.asarray(vert, F32)
    faces = np.asarray(faces, np.int64)
    w = weights(areas(vert, faces))
    incl = np.cumsum(w, dtype=np.uint64)
    total = int(incl[-1])
    start = incl - w
    g = ((np.arange(n, dtype=np.uint64) + np.uint64(int(row) & 0xFFFFFFFF)) & M32) * np.uint64(3)
    h = [keys(seed, g + np.uint64(k)) for k in range(3)]
    u = np.array([(int(x) * total) >> 32 for x in h[0]], dtype=np.uint64)
    f = np.searchsorted(start, u, side="right") - 1
    r1 = (h[1] >> np.uint64(8)).astype(F32) / F32(16777216.0)
    r2 = (h[2] >> np.uint64(8)).astype(F32) / F32(16777216.0)
    flip = r1 + r2 > F32(1)
    r1 = np.where(flip, F32(1) - r1, r1)
    r2 = np.where(flip, F32(1) - r2, r2)
    p, q, r = vert[faces[f, 0]], vert[faces[f, 1]], vert[faces[f, 2]]
    pts = (p + r1[:, None] * (q - p)) + r2[:, None] * (r - p)
    assert pts.dtype == F32
    return pts, f.astype(np.int32)
