"""Test-only numpy restatements of the two resizes `segmentor_width_size` puts round the mask generator (ISM/model/sam.py:77-100), for
whole rectangular images.  Nothing in the package imports this module, and it shares no code with tests/cv2_linear.py (the square
restatement that pins the rgb crops): the taps here are formed index by index with numpy scalars, so the two can be held against each
other (tests/test_seg_resize_host.py).

Image: cv2.resize(src, (w, h)), default INTER_LINEAR, of a CV_8UC3 image as OpenCV 4.x computes it (imgproc/src/resize.cpp): 11-bit
coefficients saturate_cast<short>(rint(f * 2048)), the source coordinate (float)((d + 0.5) * scale - 0.5) with scale = 1.0 /
((double)dst / src), the x axis clamped to (0, 0) below the row and to (n - 1, 0) from its last pixel on, the y axis with clamped row
indices only, the horizontal pass in int32 and the vertical pass in its vectorised form for every column; exactly 2x on both axes is
the INTER_AREA mean, equal sizes copy.  Parity with OpenCV itself is checked only where cv2 imports.

Masks: F.interpolate(masks[:, None].float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0] with the taps formed in fp32
exactly as upsample_bilinear2d forms them (operation by operation on numpy float32) and the four taps combined in float64: the
yardstick the fp32 routes are measured against."""
import numpy as np

F32 = np.float32


def _short(v):
    return max(-32768, min(32767, int(v)))


# ------------------------------------------------------------------------------------------------------------------ the image
def axis_taps(n_src, n_dst, x_axis):
    """Per output index of one axis: (first source index, second source index, coefficient of the first, of the second)."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    i0, i1, k0, k1 = (np.zeros(n_dst, dtype=np.int64) for _ in range(4))
    for d in range(n_dst):
        f = F32((d + 0.5) * scale - 0.5)          # double arithmetic, one rounding to float
        s = int(np.floor(f))
        f = F32(f - F32(s))
        if x_axis:
            if s < 0:
                s, f = 0, F32(0)
            if s >= n_src - 1:
                s, f = n_src - 1, F32(0)
        k0[d] = _short(np.rint(F32(F32(1) - f) * F32(2048)))
        k1[d] = _short(np.rint(f * F32(2048)))
        i0[d] = min(max(s, 0), n_src - 1)
        i1[d] = min(max(s + 1, 0), n_src - 1)
    return i0, i1, k0, k1


def resize(src, h, w):
    """cv2.resize(src, (w, h)) of an (H, W, 3) uint8 image, INTER_LINEAR."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    H, W = src.shape[:2]
    if h < 1 or w < 1:
        raise ValueError("cv2.resize raises for an empty output size (%d x %d)" % (h, w))
    p = src.astype(np.int64)
    if (H, W) == (h, w):
        return src.copy()
    if (H, W) == (2 * h, 2 * w):
        quad = p.reshape(h, 2, w, 2, 3)
        return ((quad.sum(axis=(1, 3)) + 2) // 4).astype(np.uint8)
    xa, xb, a0, a1 = axis_taps(W, w, True)
    ya, yb, b0, b1 = axis_taps(H, h, False)
    rows = np.take(p, xa, axis=1) * a0.reshape(1, w, 1) + np.take(p, xb, axis=1) * a1.reshape(1, w, 1)  # the horizontal pass, (H, w, 3)
    rows = np.clip(rows >> 4, -32768, 32767)
    upper = (np.take(rows, ya, axis=0) * b0.reshape(h, 1, 1)) >> 16
    lower = (np.take(rows, yb, axis=0) * b1.reshape(h, 1, 1)) >> 16
    return np.clip((np.clip(upper + lower, -32768, 32767) + 2) >> 2, 0, 255).astype(np.uint8)


def resized_shape(orig_size, width):
    """ISM/model/sam.py:78-80."""
    return int(width * orig_size[0] / orig_size[1]), int(width)


def resize_width(src, width):
    """preprocess_resize (ISM/model/sam.py:77-83)."""
    h, w = resized_shape(src.shape[:2], width)
    return resize(src, h, w)


def bilinear_f64(src, h, w):
    """The same coordinate map with exact float64 weights and no rounding."""
    src = np.asarray(src, dtype=np.float64)
    H, W = src.shape[:2]
    fx = (np.arange(w) + 0.5) * (W / w) - 0.5
    sx = np.floor(fx)
    fx = fx - sx
    fx = np.where((sx < 0) | (sx >= W - 1), 0.0, fx)
    sx = np.clip(sx, 0, W - 1).astype(np.int64)
    fy = (np.arange(h) + 0.5) * (H / h) - 0.5
    sy = np.floor(fy)
    fy = fy - sy
    sy = sy.astype(np.int64)
    hx = src[:, sx] * (1 - fx)[None, :, None] + src[:, np.minimum(sx + 1, W - 1)] * fx[None, :, None]
    return hx[np.clip(sy, 0, H - 1)] * (1 - fy)[:, None, None] + hx[np.clip(sy + 1, 0, H - 1)] * fy[:, None, None]


def scale_boxes(boxes, orig_size, width):
    """postprocess_resize's boxes (ISM/model/sam.py:94-99): float32 boxes times W / width, clamped to the image."""
    import torch
    b = boxes.float() * (orig_size[1] / width)
    b[:, [0, 2]] = torch.clamp(b[:, [0, 2]], 0, orig_size[1] - 1)
    b[:, [1, 3]] = torch.clamp(b[:, [1, 3]], 0, orig_size[0] - 1)
    return b


# ------------------------------------------------------------------------------------------------------------------ the masks
def mask_taps(n_src, n_dst):
    """area_pixel_compute_source_index with align_corners=False in fp32: (i0, i1, l0, l1), the weights float32."""
    scale = F32(n_src) / F32(n_dst)
    src = scale * (np.arange(n_dst, dtype=np.float32) + F32(0.5)) - F32(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int64), n_src - 1)
    i1 = i0 + (i0 < n_src - 1)
    l1 = src - i0.astype(np.float32)
    l0 = F32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def masks_bilinear(masks, H, W):
    """(K, h, w) masks (non-zero = 1) -> (K, H, W) float64: the fp32 taps, the four products and three sums in float64."""
    m = (np.asarray(masks) != 0).astype(np.float64)
    y0, y1, h0, h1 = mask_taps(m.shape[1], H)
    x0, x1, w0, w1 = mask_taps(m.shape[2], W)
    w0, w1 = w0.astype(np.float64)[None, None, :], w1.astype(np.float64)[None, None, :]
    h0, h1 = h0.astype(np.float64)[None, :, None], h1.astype(np.float64)[None, :, None]
    top, bot = m[:, y0], m[:, y1]
    return h0 * (w0 * top[:, :, x0] + w1 * top[:, :, x1]) + h1 * (w0 * bot[:, :, x0] + w1 * bot[:, :, x1])


# ------------------------------------------------------------------------------------------------------------------ inputs
# (H, W, width) of the image cases: 2x area; 2x in one axis only; 3x shrink; enlarging; portrait and odd; the copy
GEOMETRIES = [(96, 128, 64), (97, 128, 64), (135, 240, 80), (30, 40, 64), (53, 37, 64), (48, 64, 64)]
FULL = (1080, 1920, 640)


def noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def stripes(H, W):
    """0 / 255 stripes one pixel wide, vertical in the upper half and horizontal below: every coefficient pair meets a full step."""
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[: H // 2, 1::2] = 255
    img[H // 2:, :, :][1::2] = 255
    return img


def mask_patterns(K, h, w, seed=0):
    """K masks (bool) cycling through: blobs, all zeros, all ones, a checkerboard, single pixels in the four corners."""
    g = np.random.default_rng(seed + 31 * h + w)
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((K, h, w), dtype=bool)
    for k in range(K):
        kind = k % 5
        if kind == 0:
            for _ in range(3):
                cy, cx, r = g.uniform(0, h), g.uniform(0, w), g.uniform(1, max(2, min(h, w) / 3))
                out[k] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        elif kind == 2:
            out[k] = True
        elif kind == 3:
            out[k] = (yy + xx) % 2 == 0
        elif kind == 4:
            out[k, [0, 0, -1, -1], [0, -1, 0, -1]] = True
    return out
