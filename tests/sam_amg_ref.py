"""Float64 restatement of SAM's mask-generator tail (what sam6d_hip.amg computes), the exact construction of the fixture's logits, and the
rule by which thresholded results are compared.  numpy only; no GPU, no reference code.

Bilinear interpolation with align_corners=False is linear and separable, so both interpolations of postprocess_masks collapse into one
row matrix and one column matrix per geometry: logits = Rh @ low @ Rw^T, every weight formed in float64.
"""
import numpy as np

CAP = 1e-4  # at most this fraction of a mask's pixels may lie within eps of a threshold (a condition on the inputs)


# ------------------------------------------------------------------------------------------------- fixture logits, exactly
def hash_noise(seed, lh, lw):
    """(lh, lw) int64 in [-6, 6], mean 0, sigma 2.2: four 2-bit fields of a 32-bit integer hash of (x, y, seed), summed.  uint64
    arithmetic on values below 2^32, masked after every product: exact and the same everywhere."""
    y, x = np.mgrid[0:lh, 0:lw].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    h = (x * np.uint64(0x9E3779B1) + y * np.uint64(0x85EBCA77) + np.uint64(seed) * np.uint64(0xC2B2AE3D)) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m32
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m32
    h ^= h >> np.uint64(15)
    seven = np.uint64(3)
    tot = (h & seven) + ((h >> np.uint64(8)) & seven) + ((h >> np.uint64(16)) & seven) + ((h >> np.uint64(24)) & seven)
    return tot.astype(np.int64) - 6


def build_logits(params, seeds, lh=256, lw=256):
    """params (M, 5) int: cx, cy, kx, ky, a; seeds (M) int.  Integer arithmetic throughout:
        d = (x - cx)^2 kx + (y - cy)^2 ky   (an ellipse; kx = ky = 0: a constant)
        q = clip(16 a - d // 16 + 16 hash_noise(seed)[y, x], -4095, 4095);   logit = (2 q + 1) / 256
    so every logit is an odd multiple of 1/256 within +-32: exact in fp32, and never equal to a threshold (0, +-1).  A smooth blob
    plus noise of 0.28 logits sigma."""
    params = np.asarray(params, dtype=np.int64)
    y, x = np.mgrid[0:lh, 0:lw].astype(np.int64)
    out = np.empty((len(params), lh, lw), dtype=np.float32)
    for i, (cx, cy, kx, ky, a) in enumerate(params):
        d = (x - cx) ** 2 * kx + (y - cy) ** 2 * ky
        q = np.clip(16 * a - d // 16 + 16 * hash_noise(int(seeds[i]), lh, lw), -4095, 4095)
        out[i] = ((2 * q + 1) / 256.0).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------- the tail in float64
def preprocess_shape(h, w, side):
    scale = side * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def interp_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of a bilinear resize, align_corners=False."""
    scale = n_in / n_out
    src = np.maximum(0.0, scale * (np.arange(n_out) + 0.5) - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    A = np.zeros((n_out, n_in))
    np.add.at(A, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(A, (np.arange(n_out), i1), l1)
    return A


def postprocess_masks(low, input_size, crop_size, img_size):
    """low (M, lh, lw) -> float64 (M, out_h, out_w): interpolate to img_size^2, keep [:in_h, :in_w], interpolate to crop_size."""
    low = np.asarray(low, dtype=np.float64)
    Rh = interp_matrix(input_size[0], crop_size[0]) @ interp_matrix(low.shape[1], img_size)[: input_size[0]]
    Rw = interp_matrix(input_size[1], crop_size[1]) @ interp_matrix(low.shape[2], img_size)[: input_size[1]]
    return np.einsum("yr,mrc,xc->myx", Rh, low, Rw, optimize=True)


def mask_box(mask):
    """xyxy (inclusive) of a bool mask, [0, 0, 0, 0] when empty."""
    ys, xs = np.where(mask.any(axis=1))[0], np.where(mask.any(axis=0))[0]
    if len(ys) == 0:
        return [0, 0, 0, 0]
    return [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])]


def near_crop_edge(boxes, crop_box, orig_size, atol=20.0):
    boxes = np.asarray(boxes, dtype=np.float64) + np.array([crop_box[0], crop_box[1], crop_box[0], crop_box[1]])
    near_crop = np.abs(boxes - np.array(crop_box, dtype=np.float64)) <= atol
    near_img = np.abs(boxes - np.array([0, 0, orig_size[1], orig_size[0]], dtype=np.float64)) <= atol
    return (near_crop & ~near_img).any(axis=1)


def stats(logits, thr, offset):
    """n_hi, n_lo, area (M) and boxes (M, 4) of float64 logits."""
    n_hi = (logits > thr + offset).sum(axis=(1, 2))
    n_lo = (logits > thr - offset).sum(axis=(1, 2))
    masks = logits > thr
    return n_hi, n_lo, masks.sum(axis=(1, 2)), np.array([mask_box(m) for m in masks], dtype=np.int64).reshape(-1, 4), masks


def uncrop(masks, crop_box, orig_size):
    out = np.zeros((masks.shape[0],) + tuple(orig_size), dtype=masks.dtype)
    out[:, crop_box[1]:crop_box[3], crop_box[0]:crop_box[2]] = masks
    return out


def rle_encode(mask):
    """Uncompressed COCO RLE counts of one (H, W) bool mask: column-major runs, the zero run first."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(edges).tolist()
    return ([0] if flat[0] else []) + counts


def rle_decode(counts, h, w):
    flat = np.zeros(h * w, dtype=bool)
    pos, val = 0, False
    for c in counts:
        flat[pos:pos + c] = val
        pos += c
        val = not val
    return flat.reshape(w, h).T


# ------------------------------------------------------------------------------------------------- how decisions are compared
def band(logits, t, eps):
    """(M, h, w) bool: pixels whose float64 value is within eps of threshold t -- the only ones whose decision may differ."""
    return np.abs(logits - t) <= eps


def check_cap(logits, thresholds, eps):
    """The condition on the inputs: per mask and threshold at most CAP of the pixels inside the band.  -> the worst fraction."""
    worst = 0.0
    for t in thresholds:
        frac = band(logits, t, eps).sum(axis=(1, 2)) / float(logits.shape[1] * logits.shape[2])
        worst = max(worst, float(frac.max()))
    assert worst <= CAP, "inputs put %.2e of a mask's pixels within %.1e of a threshold (cap %.0e)" % (worst, eps, CAP)
    return worst


def stability_decided(logits, thr, offset, thresh, eps):
    """(M) bool: the float64 stability decision cannot change when n_hi and n_lo move by their band counts."""
    n_hi, n_lo = (logits > thr + offset).sum(axis=(1, 2)), (logits > thr - offset).sum(axis=(1, 2))
    b_hi, b_lo = band(logits, thr + offset, eps).sum(axis=(1, 2)), band(logits, thr - offset, eps).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = (n_hi - b_hi) / (n_lo + b_lo).astype(np.float64)
        hi = (n_hi + b_hi) / np.maximum(n_lo - b_lo, 0).astype(np.float64)
        mid = n_hi / n_lo.astype(np.float64)
    empty = (n_lo + b_lo) == 0  # 0 / 0 whatever the band does: dropped by every path
    return empty | ((lo >= thresh) & (mid >= thresh)) | ((hi < thresh) & (mid < thresh))


def compare_stats(got, logits, thr, offset, eps, name=""):
    """got: dict n_hi, n_lo, area (M), box (M, 4), masks (M, h, w) bool of some fp32 path; logits: float64 values of the same masks.
    Bits equal outside the band; counts within the band's size; box corners equal unless a band pixel lies on the extreme row / column."""
    n_hi, n_lo, area, boxes, masks = stats(logits, thr, offset)
    for key, want, t in (("n_hi", n_hi, thr + offset), ("n_lo", n_lo, thr - offset), ("area", area, thr)):
        slack = band(logits, t, eps).sum(axis=(1, 2))
        diff = np.abs(np.asarray(got[key], dtype=np.int64) - want)
        assert (diff <= slack).all(), "%s %s: off by %s with %s band pixels" % (name, key, diff.tolist(), slack.tolist())
    bnd = band(logits, thr, eps)
    bad = (np.asarray(got["masks"], dtype=bool) != masks) & ~bnd
    assert not bad.any(), "%s: %d mask bits differ outside the band" % (name, int(bad.sum()))
    gb = np.asarray(got["box"], dtype=np.int64)
    for m in range(len(boxes)):
        if (gb[m] == boxes[m]).all():
            continue
        on = masks[m] | bnd[m]
        ext = mask_box(on)  # the box when every band pixel counts ...
        off = mask_box(masks[m] & ~bnd[m])  # ... and when none does
        lo = [min(ext[0], off[0]), min(ext[1], off[1]), min(ext[2], off[2]), min(ext[3], off[3])]
        hi = [max(ext[0], off[0]), max(ext[1], off[1]), max(ext[2], off[2]), max(ext[3], off[3])]
        assert bnd[m].any() and all(lo[k] <= gb[m][k] <= hi[k] for k in range(4)), "%s box %d: %s, float64 %s" % (name, m, gb[m], boxes[m])
