"""The project's own restatement, in numpy, of what sam6d_hip.refdata computes before the encoder: PIL's getbbox rule and the template
crops of ISM/run_inference_custom.py:136-155 ("custom") and ISM/provider/bop.py:66-83 ("bop") through CropResizePad(224)
(ISM/utils/bbox_utils.py:89-126).  tests/test_refdata_host.py pins the box rule against the installed Pillow and the crops against the
composition of parts already pinned to the reference (host getbbox, tests/dinov2_ref.crop_resize_pad, the literal torch operations);
the GPU tests compare the kernels with this file bit for bit."""
import math

import numpy as np

MEAN = np.array((0.485, 0.456, 0.406), np.float32)
STD = np.array((0.229, 0.224, 0.225), np.float32)
TARGET = 224


def getbbox(band):
    """Image.getbbox() of one single-band image (H,W): (left, upper, right + 1, lower + 1) over the pixels != 0; (0,0,0,0) where PIL
    returns None."""
    a = np.asarray(band) != 0
    ys, xs = np.nonzero(a.any(axis=1))[0], np.nonzero(a.any(axis=0))[0]
    if len(ys) == 0:
        return (0, 0, 0, 0)
    return (int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1)


def boxes(bands):
    """getbbox of every image of (T,H,W) -> (T,4) int64."""
    return np.array([getbbox(b) for b in bands], np.int64).reshape(-1, 4)


BOX_SIZES = ((1, 1), (5, 7), (64, 61), (37, 130))  # (H, W): one pixel, small, a width that is no multiple of 4, wider than tall


def box_cases():
    """The box test images, as (name, (H,W) uint8): per size one pixel in each corner in turn, only the last row, only the last
    column, the full image, value 1 instead of 255, two far-apart pixels, and the empty image."""
    out = []
    for H, W in BOX_SIZES:
        def img(fill=None):
            a = np.zeros((H, W), np.uint8)
            if fill is not None:
                fill(a)
            return a
        tag = "%dx%d " % (H, W)
        for name, (y, x) in (("top-left", (0, 0)), ("top-right", (0, W - 1)), ("bottom-left", (H - 1, 0)), ("bottom-right", (H - 1, W - 1))):
            out.append((tag + name, img(lambda a, y=y, x=x: a.__setitem__((y, x), 255))))
        out.append((tag + "last row", img(lambda a: a.__setitem__((H - 1, slice(None)), 255))))
        out.append((tag + "last column", img(lambda a: a.__setitem__((slice(None), W - 1), 255))))
        out.append((tag + "full", img(lambda a: a.fill(255))))
        out.append((tag + "value 1", img(lambda a: a.__setitem__((H // 2, W // 3), 1))))
        out.append((tag + "two pixels", img(lambda a: (a.__setitem__((H // 5, W - 1 - W // 7), 200), a.__setitem__((H - 1 - H // 9, W // 6), 3)))))
        out.append((tag + "empty", img()))
    return out


# (x1, y1, x2, y2) on a 480 x 640 image, beside the boxes of tests/golden/crop_resize_pad.npz: the whole image, one pixel wide, one pixel
# tall, a square of side 224, of side 3, larger than 224, one touching the far corner, one whose padding is odd (57 rows -> 127)
CROP_BOXES_480x640 = ((0, 0, 640, 480), (300, 100, 301, 300), (100, 200, 300, 201), (50, 60, 274, 284), (10, 10, 13, 13),
                      (100, 50, 400, 350), (520, 405, 640, 480), (200, 200, 300, 257))
# on a 48 x 64 image (H x W): every box upscales
CROP_BOXES_48x64 = ((0, 0, 64, 48), (3, 5, 40, 20), (10, 2, 11, 47), (1, 30, 63, 31), (20, 10, 43, 33), (61, 45, 64, 48), (7, 9, 30, 48))


def template_scene(H, W, bxs, seed):
    """One template per box: rgba (T,H,W,4) u8 with random colours everywhere and an alpha band that is 0 outside the box, a ring of
    intermediate values (1 .. 254) on the box's border and 0 / 255 inside it -- so getbbox of the alpha band is the box."""
    g = np.random.default_rng(seed)
    T = len(bxs)
    rgba = g.integers(0, 256, (T, H, W, 4), dtype=np.uint8)
    rgba[..., 3] = 0
    for t, (x1, y1, x2, y2) in enumerate(bxs):
        a = np.where(g.random((y2 - y1, x2 - x1)) < 0.8, 255, 0).astype(np.uint8)
        ring = np.ones(a.shape, bool)
        ring[1:-1, 1:-1] = False
        a[ring] = g.integers(1, 255, int(ring.sum()), dtype=np.uint8)
        rgba[t, y1:y2, x1:x2, 3] = a
    return rgba


def _nearest(n_out, inv, size):
    """source index of every output index of a nearest resize: min(floor(dst * inv), size - 1), the product in float32"""
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * np.float32(inv)).astype(np.int64), size - 1)


def crop_maps(box, H, W):
    """CropResizePad(224) of one box as index maps: rows (224), cols (224) of the source pixel of every output row / column and
    row_ok, col_ok (224) bool, False where the output is padding.  A box without area, or whose resized crop is empty, is all padding."""
    none = (np.zeros(TARGET, np.int64), np.zeros(TARGET, np.int64), np.zeros(TARGET, bool), np.zeros(TARGET, bool))
    bx1, by1, bx2, by2 = (int(v) for v in box)
    side = max(bx2 - bx1, by2 - by1)
    if side <= 0:
        return none
    s = float(np.float32(1.0) / np.float32(side) * np.float32(TARGET))  # reciprocal, then times 224, both in float32
    x1, x2 = min(max(bx1, 0), W), min(max(bx2, 0), W)
    y1, y2 = min(max(by1, 0), H), min(max(by2, 0), H)
    cw, ch = x2 - x1, y2 - y1
    if cw <= 0 or ch <= 0:
        return none
    rw, rh = math.floor(cw * s), math.floor(ch * s)
    if rw <= 0 or rh <= 0:
        return none
    final = np.arange(TARGET)  # output pixel -> pixel of the padded square
    top = left = 0
    if rw == rh:
        if rw != TARGET:
            assert math.floor(rw * (TARGET / rw)) == TARGET
            final = _nearest(TARGET, np.float32(1.0 / (TARGET / rw)), rw)
    else:
        top, left = max((TARGET - rh) // 2, 0), max((TARGET - rw) // 2, 0)
    ry, rx = final - top, final - left
    inv1 = np.float32(1.0 / s)
    rows = y1 + _nearest(rh, inv1, ch)[np.clip(ry, 0, rh - 1)]
    cols = x1 + _nearest(rw, inv1, cw)[np.clip(rx, 0, rw - 1)]
    return rows, cols, (ry >= 0) & (ry < rh), (rx >= 0) & (rx < rw)


def template_crops(rgb, mask, bxs, flavour):
    """rgb (T,H,W,3|4) u8, mask (T,H,W) u8, bxs (T,4) -> (templates (T,3,224,224), masks224 (T,224,224)) float32.
    custom: fl32(u8 / 255) * fl32(mask / 255), padding 0.  bop: (fl32(u8 / 255) - mean) / std with Normalize applied after the
    padding, so a padded pixel holds (0 - mean) / std.  The mask: fl32(mask / 255), padding 0.  (u8 / 255 in float64 rounded to
    float32 equals the float32 division for all 256 values: test_refdata_host.py.)"""
    assert flavour in ("custom", "bop")
    rgb, mask = np.asarray(rgb), np.asarray(mask)
    T, H, W = mask.shape
    out = np.zeros((T, 3, TARGET, TARGET), np.float32)
    om = np.zeros((T, TARGET, TARGET), np.float32)
    for t in range(T):
        rows, cols, row_ok, col_ok = crop_maps(bxs[t], H, W)
        inside = row_ok[:, None] & col_ok[None, :]
        px = rgb[t][rows[:, None], cols[None, :], :3].astype(np.float32) / np.float32(255)
        m = mask[t][rows[:, None], cols[None, :]].astype(np.float32) / np.float32(255)
        m[~inside] = 0
        if flavour == "custom":
            v = px * m[:, :, None]
        else:
            v = px.copy()
        v[~inside] = 0
        if flavour == "bop":
            v = (v - MEAN) / STD
        out[t] = v.transpose(2, 0, 1)
        om[t] = m
    return out, om
