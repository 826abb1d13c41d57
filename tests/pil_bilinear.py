"""A numpy restatement of what SAM does to an image before its encoder, with coefficient code of its own (it imports nothing from
sam6d_hip): ResizeLongestSide.apply_image (ISM/segment_anything/utils/transforms.py:26-31: torchvision's resize of a PIL image, i.e.
PIL.Image.resize(..., BILINEAR)), then Sam.preprocess (modeling/sam.py:164-173).

Pillow's ImagingResample for 8-bit pixels (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
Vertical_8bpc) is integer arithmetic once its per-axis coefficients are known:
    scale = in / out, filterscale = max(scale, 1), support = filterscale (the bilinear filter's support is 1)
    output i: center = (i + 0.5) scale, lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), in)
    tap j = 0 .. hi - lo - 1: w = triangle((j + lo - center + 0.5) * (1 / filterscale)), divided by the sum of the taps' w
    k = int(0.5 + w * 2^22)
    a pass: clip8((2^21 + sum_j pixel_j k_j) >> 22), stored as a byte
horizontal pass first, then the vertical pass on its bytes; a pass whose axis keeps its size is skipped.  One exception lies in
Image.resize itself (Pillow 12.2.0, the version the fixture was made with): an image more than 100 times as tall as it is wide that
shrinks vertically gets its vertical pass first (`vertical_first`).  tests/test_sam_front_host.py holds this against Pillow itself
(the fixture tests/golden/sam_front.npz, and PIL directly wherever it imports)."""
import numpy as np

PRECISION_BITS = 22


def preprocess_shape(h, w, side):
    """ResizeLongestSide.get_preprocess_shape (transforms.py:91-102)."""
    scale = side * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def coefficients(in_size, out_size):
    """[(lo, [k_0 .. k_{n-1}]) for every output index]: python floats are C doubles, the statements follow precompute_coeffs."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = []
        for j in range(hi - lo):
            t = abs((j + lo - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(w[1:], w[0]) if w else 0.0  # (summed left to right, as the C loop does)
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((lo, [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out


def _pass(img, coeffs, axis):
    """One resampling pass of a (H, W, C) uint8 image along `axis` (0 vertical, 1 horizontal)."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    res = np.empty((len(coeffs),) + src.shape[1:], dtype=np.uint8)
    for i, (lo, k) in enumerate(coeffs):
        ss = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j, kj in enumerate(k):
            ss += src[lo + j] * kj
        res[i] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis)


def vertical_first(h, w, oh):
    """Image.resize's rule for running the vertical pass first (PIL/Image.py, `self.size[1] > self.size[0] * 100 and size[1] <
    self.size[1]`)."""
    return h > w * 100 and oh < h


def resize(img, oh, ow):
    """PIL.Image.fromarray(img).resize((ow, oh), BILINEAR) for a (H, W, C) uint8 array."""
    img = np.ascontiguousarray(img)
    if vertical_first(img.shape[0], img.shape[1], oh):
        img = _pass(img, coefficients(img.shape[0], oh), 0)
    if img.shape[1] != ow:
        img = _pass(img, coefficients(img.shape[1], ow), 1)
    if img.shape[0] != oh:
        img = _pass(img, coefficients(img.shape[0], oh), 0)
    return np.ascontiguousarray(img)


def preprocessed(img, mean, std, side, reverse=False):
    """(H, W, 3) uint8 -> (3, side, side) float32: resize to preprocess_shape, (x - mean) / std per channel in float32 (one
    subtraction, one division), zeros below and to the right.  reverse: the channels are read in the opposite order first (the
    predictor's image[..., ::-1] for a BGR image_format, predictor.py:56-58)."""
    if reverse:
        img = img[..., ::-1]
    oh, ow = preprocess_shape(img.shape[0], img.shape[1], side)
    r = resize(img, oh, ow).astype(np.float32).transpose(2, 0, 1)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    out = np.zeros((3, side, side), dtype=np.float32)
    out[:, :oh, :ow] = (r - m) / s
    return out


def patch_rows(x, patch=16):
    """(3, side, side) -> ((side / patch)^2, 3 patch^2): row (side / patch) py + px, columns in (c, kh, kw) order."""
    c, s, _ = x.shape
    g = s // patch
    return np.ascontiguousarray(x.reshape(c, g, patch, g, patch).transpose(1, 3, 0, 2, 4).reshape(g * g, c * patch * patch))
