"""SAM's automatic mask generator after the mask decoder, on the library (ISM/model/sam.py:52-148 CustomSamAutomaticMaskGenerator,
ISM/segment_anything/automatic_mask_generator.py:225-321, ISM/segment_anything/modeling/sam.py:133-162, ISM/segment_anything/utils/amg.py).

Per point batch the decoder leaves `low` (B, 3, 256, 256) logits and `iou_preds` (B, 3).  The reference upsamples all of them to
1024 x 1024 and on to the image size, thresholds that tensor three times, walks it for boxes, run-length encodes every kept mask through
the host and decodes it again at the end.  Here one launch (sam6d_amg_mask_stats) leaves two counts, an area, a box and the bit-packed
mask per live proposal; the keep decisions are small vector ops on the device; a crop ends with one compaction, sam6d_nms and one
launch (sam6d_amg_unpack_masks) that writes the surviving masks in the image frame.  A crop costs two 4-byte read-backs (how many
proposals the filters kept, how many NMS kept), whatever the number of batches and masks.

The min_mask_region_area clean-up behind the generator (automatic_mask_generator.py:324-372, utils/amg.py:267-291) is here as well:
`mask_components` (8-connected labelling in a canonical form), `remove_small_regions` (both passes for all masks, in place on the device)
and `postprocess_small_regions` (clean-up, boxes, NMS; one 4-byte read-back) on sam6d_mask_components / sam6d_amg_small_regions.

`eager_tail` is the same tail in plain torch ops on any device: the CPU path, the SAM6D_HIP_AMG=0 path and the timing baseline.
The geometry helpers (point grids, crop boxes, apply_coords) are the reference's arithmetic restated on the host.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .ism import mask_to_indices, nms
from .runtime import _p, _s

MASKS_PER_POINT = 3   # multimask_output=True
EDGE_ATOL = 20.0      # is_box_near_crop_edge's default


def hip_enabled(device):
    """The library path is taken for HIP device tensors unless SAM6D_HIP_AMG=0."""
    return torch.device(device).type == "cuda" and os.environ.get("SAM6D_HIP_AMG", "1") != "0"


# ------------------------------------------------------------------------------------------------- geometry on the host
def preprocess_shape(h, w, side):
    """ResizeLongestSide.get_preprocess_shape (ISM/segment_anything/utils/transforms.py:91-102), in double."""
    scale = side * 1.0 / max(h, w)
    newh, neww = h * scale, w * scale
    return int(newh + 0.5), int(neww + 0.5)


def apply_coords(coords, original_size, side):
    """ResizeLongestSide.apply_coords (transforms.py:33-45): (..., 2) xy points of an original_size = (H, W) image -> float64 points
    of the resized input."""
    old_h, old_w = original_size
    new_h, new_w = preprocess_shape(old_h, old_w, side)
    out = np.array(coords, dtype=np.float64, copy=True)
    out[..., 0] = out[..., 0] * (new_w / old_w)
    out[..., 1] = out[..., 1] * (new_h / old_h)
    return out


def point_grid(n_per_side):
    """build_point_grid (amg.py:179-186): (n*n, 2) xy in [0, 1], x fastest."""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    xs = np.tile(side[None, :], (n_per_side, 1))
    ys = np.tile(side[:, None], (1, n_per_side))
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def layer_point_grids(n_per_side, n_layers, scale_per_layer):
    """build_all_layer_point_grids (amg.py:189-197)."""
    return [point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def crop_boxes(im_size, n_layers, overlap_ratio):
    """generate_crop_boxes (amg.py:200-234): xyxy boxes (exclusive ends) and their layer, the whole image first."""
    im_h, im_w = im_size
    boxes, layers = [[0, 0, im_w, im_h]], [0]
    short = min(im_h, im_w)
    for i_layer in range(n_layers):
        n = 2 ** (i_layer + 1)
        overlap = int(overlap_ratio * short * (2 / n))
        cw = int(math.ceil((overlap * (n - 1) + im_w) / n))
        ch = int(math.ceil((overlap * (n - 1) + im_h) / n))
        for x0 in [int((cw - overlap) * i) for i in range(n)]:
            for y0 in [int((ch - overlap) * i) for i in range(n)]:
                boxes.append([x0, y0, min(x0 + cw, im_w), min(y0 + ch, im_h)])
                layers.append(i_layer + 1)
    return boxes, layers


# ------------------------------------------------------------------------------------------------- the two bindings
def _need_hip(t, who):
    if not t.is_cuda:
        raise RuntimeError("%s: needs HIP device tensors (eager_tail is the CPU path)" % who)


def words(width):
    return (width + 31) // 32


def mask_stats(low, live, input_size, crop_size, img_size, thr, offset, out=None, logits=False):
    """sam6d_amg_mask_stats.  low (M, lh, lw) float32, live (M) uint8 / bool, input_size = (in_h, in_w) of the encoder's unpadded
    input, crop_size = (out_h, out_w), img_size = the encoder side S -> dict n_hi, n_lo, area (M) int32, box (M, 4) int32, bits
    (M, out_h, ceil(out_w / 32)) int32 (the words of the packed mask), and `logits` (M, out_h, out_w) when asked for (a test's
    measurement; the product path never is).  `out`: a dict of caller-owned tensors of those shapes to write into (rows with live == 0
    stay as they are); without it fresh zero tensors are returned.  Asynchronous."""
    _need_hip(low, "mask_stats")
    if low.dim() != 3 or low.dtype != torch.float32:
        raise ValueError("mask_stats: low must be (M, lh, lw) float32, got %s %s" % (tuple(low.shape), low.dtype))
    low = low.contiguous()
    M, lh, lw = low.shape
    (in_h, in_w), (oh, ow) = input_size, crop_size
    live8 = live.to(torch.uint8).contiguous()
    if tuple(live8.shape) != (M,):
        raise ValueError("mask_stats: live must be (%d,), got %s" % (M, tuple(live8.shape)))
    dev = low.device
    with torch.cuda.device(dev):
        if out is None:
            z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
            out = dict(n_hi=z(M), n_lo=z(M), area=z(M), box=z(M, 4), bits=z(M, oh, words(ow)))
        for k, shape in (("n_hi", (M,)), ("n_lo", (M,)), ("area", (M,)), ("box", (M, 4)), ("bits", (M, oh, words(ow)))):
            t = out[k]
            if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
                raise ValueError("mask_stats: out[%r] must be a contiguous int32 %s on %s" % (k, shape, dev))
        lg = torch.empty((M, oh, ow), dtype=torch.float32, device=dev) if logits else None
        nbytes = int(_lib.load().sam6d_amg_mask_stats_workspace_bytes(M, lh, lw, int(img_size), in_h, oh))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        _lib.call("sam6d_amg_mask_stats", _p(low), _p(live8), M, lh, lw, int(img_size), in_h, in_w, oh, ow, float(thr), float(offset),
                  _p(out["n_hi"]), _p(out["n_lo"]), _p(out["area"]), _p(out["box"]), _p(out["bits"]), _p(lg), _p(ws), nbytes,
                  _s())
    if logits:
        out = dict(out, logits=lg)
    return out


def unpack_masks(bits, idx, crop_size, crop_box, orig_size, dtype=torch.bool):
    """sam6d_amg_unpack_masks.  bits (C, out_h, ceil(out_w / 32)) int32, idx (K) int64 rows of it -> (K, H, W) masks of the orig_size =
    (H, W) image, the crop placed at crop_box's corner and zero around it (uncrop_masks); dtype bool / uint8 / float32."""
    _need_hip(bits, "unpack_masks")
    (oh, ow), (H, W) = crop_size, orig_size
    x0, y0 = int(crop_box[0]), int(crop_box[1])
    if tuple(bits.shape[1:]) != (oh, words(ow)) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError("unpack_masks: bits must be a contiguous int32 (C, %d, %d), got %s %s" % (oh, words(ow), tuple(bits.shape), bits.dtype))
    if dtype not in (torch.bool, torch.uint8, torch.float32):
        raise ValueError("unpack_masks: dtype must be bool, uint8 or float32, got %s" % dtype)
    idx = idx.to(device=bits.device, dtype=torch.int64).contiguous()
    K = idx.shape[0]
    f32 = dtype == torch.float32
    with torch.cuda.device(bits.device):
        out = torch.empty((K, H, W), dtype=torch.float32 if f32 else torch.uint8, device=bits.device)
        for k0 in range(0, K, 65535):
            k = min(65535, K - k0)
            _lib.call("sam6d_amg_unpack_masks", _p(bits), idx.data_ptr() + 8 * k0, bits.shape[0], k, oh, ow, x0, y0, H, W, int(f32),
                      out.data_ptr() + k0 * H * W * out.element_size(), _s())
    return out.view(torch.bool) if dtype == torch.bool else out


# ------------------------------------------------------------------------------------------------- segmentor_width_size
IMAGE_MAX_SIZE = 4096   # sam6d_image_resize_linear: H, W, h, w
MASKS_MAX_SIZE = 8192   # sam6d_masks_resize_bilinear: h, w, H, W


def resized_shape(orig_size, width):
    """The size preprocess_resize asks cv2.resize for (ISM/model/sam.py:78-80): orig_size = (H, W) -> (int(width * H / W), int(width))."""
    return int(width * orig_size[0] / orig_size[1]), int(width)


def _image_sizes(image, size, who):
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() != 3:
        raise ValueError("%s: the image must be a uint8 tensor (H, W, 3), got %s %s"
                         % (who, getattr(image, "dtype", type(image).__name__), tuple(getattr(image, "shape", ()))))
    if image.shape[2] != 3:
        raise ValueError("%s: the image must have 3 channels, got %d" % (who, image.shape[2]))
    (H, W), (h, w) = (int(v) for v in image.shape[:2]), (int(v) for v in size)
    if not (1 <= H <= IMAGE_MAX_SIZE and 1 <= W <= IMAGE_MAX_SIZE):
        raise ValueError("%s: H and W must be 1 .. %d, got %d x %d" % (who, IMAGE_MAX_SIZE, H, W))
    if h < 1:
        raise ValueError("%s: the output has %d rows: h must be at least 1 (cv2.resize raises for an empty size)" % (who, h))
    if not (1 <= w <= IMAGE_MAX_SIZE and h <= IMAGE_MAX_SIZE):
        raise ValueError("%s: h and w must be 1 .. %d, got %d x %d" % (who, IMAGE_MAX_SIZE, h, w))
    return H, W, h, w


def resize_image(image_u8, size, out=None):
    """sam6d_image_resize_linear.  image_u8 (H, W, 3) uint8 on a HIP device (a crop view with a row stride above 3 W is read in place),
    size = (h, w) -> (h, w, 3) uint8 = cv2.resize(image, (w, h)), default INTER_LINEAR, as OpenCV 4.x computes it for CV_8UC3 (exactly
    2x on both axes: the INTER_AREA mean; equal sizes: a copy).  `out`: a contiguous uint8 (h, w, 3) tensor to write into, which must
    not overlap the image.  Asynchronous."""
    H, W, h, w = _image_sizes(image_u8, size, "resize_image")
    if not image_u8.is_cuda:
        raise RuntimeError("resize_image: needs a HIP device tensor (resize_image_eager is the CPU path)")
    img = image_u8
    if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * W:
        img = img.contiguous()
    with torch.cuda.device(img.device):
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
        elif tuple(out.shape) != (h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != img.device:
            raise ValueError("resize_image: out must be a contiguous uint8 (%d, %d, 3) on %s" % (h, w, img.device))
        _lib.call("sam6d_image_resize_linear", _p(img), img.stride(0), H, W, 3, _p(out), h, w, _s())
    return out


@functools.lru_cache(maxsize=64)
def _cv_axis(n_src, n_dst, clamp):
    """OpenCV's INTER_LINEAR taps of one axis (imgproc/src/resize.cpp), n_src -> n_dst pixels: the source coordinate
    (float)((d + 0.5) * scale - 0.5) with scale = 1.0 / ((double)n_dst / n_src), its floor and fraction in fp32, the 11-bit coefficients
    saturate_cast<short>(rint(f * 2048)).  clamp (the x axis): s < 0 -> (0, 0) and s >= n_src - 1 -> (n_src - 1, 0); without (the y
    axis) only the indices are clipped.  -> (i0, i1, k0, k1) int64 numpy arrays, read-only."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    f = f - fl
    s = fl.astype(np.int64)
    if clamp:
        f[s < 0], s[s < 0] = 0, 0
        f[s >= n_src - 1], s[s >= n_src - 1] = 0, n_src - 1
    k0 = np.clip(np.rint((np.float32(1.0) - f) * np.float32(2048.0)), -32768, 32767).astype(np.int64)
    k1 = np.clip(np.rint(f * np.float32(2048.0)), -32768, 32767).astype(np.int64)
    out = (np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), k0, k1)
    for a in out:
        a.setflags(write=False)
    return out


def resize_image_eager(image_u8, size):
    """`resize_image` in plain torch on the image's device (CPU included): the same taps, the horizontal pass, the vertical pass in its
    vectorised form and the 2 x 2 mean as int32 gathers and sums."""
    H, W, h, w = _image_sizes(image_u8, size, "resize_image_eager")
    if (H, W) == (h, w):
        return image_u8.contiguous().clone()
    dev = image_u8.device
    v = image_u8.to(torch.int32)
    if (H, W) == (2 * h, 2 * w):
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).to(torch.uint8)
    x0, x1, a0, a1 = (torch.from_numpy(a.copy()).to(dev) for a in _cv_axis(W, w, True))
    y0, y1, b0, b1 = (torch.from_numpy(a.copy()).to(dev) for a in _cv_axis(H, h, False))
    hx = v[:, x0] * a0.int()[None, :, None] + v[:, x1] * a1.int()[None, :, None]  # (H, w, 3), int32
    hx = (hx >> 4).clamp(-32768, 32767)
    t0 = (hx[y0] * b0.int()[:, None, None]) >> 16
    t1 = (hx[y1] * b1.int()[:, None, None]) >> 16
    return (((t0 + t1).clamp(-32768, 32767) + 2) >> 2).clamp(0, 255).to(torch.uint8)


def _masks_sizes(masks, size, who):
    if not torch.is_tensor(masks) or masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: masks must be a (K, h, w) bool or uint8 tensor, got %s %s"
                         % (who, getattr(masks, "dtype", type(masks).__name__), tuple(getattr(masks, "shape", ()))))
    (K, h, w), (H, W) = (int(v) for v in masks.shape), (int(v) for v in size)
    if not all(1 <= v <= MASKS_MAX_SIZE for v in (h, w, H, W)):
        raise ValueError("%s: sizes must be 1 .. %d, got %d x %d -> %d x %d" % (who, MASKS_MAX_SIZE, h, w, H, W))
    return K, h, w, H, W


def resize_masks(masks, size, out=None):
    """sam6d_masks_resize_bilinear.  masks (K, h, w) bool or uint8 on a HIP device (any non-zero byte is 1), size = (H, W) -> (K, H, W)
    float32 = F.interpolate(masks.unsqueeze(1).float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0], enlarging or
    shrinking; neither a float copy of the input nor anything but the result is allocated.  `out`: a contiguous float32 (K, H, W)
    tensor to write into.  Asynchronous."""
    K, h, w, H, W = _masks_sizes(masks, size, "resize_masks")
    if not masks.is_cuda:
        raise RuntimeError("resize_masks: needs a HIP device tensor (resize_masks_eager is the CPU path)")
    m8 = masks.contiguous()
    if m8.dtype == torch.bool:
        m8 = m8.view(torch.uint8)
    with torch.cuda.device(m8.device):
        if out is None:
            out = torch.empty((K, H, W), dtype=torch.float32, device=m8.device)
        elif tuple(out.shape) != (K, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != m8.device:
            raise ValueError("resize_masks: out must be a contiguous float32 (%d, %d, %d) on %s" % (K, H, W, m8.device))
        for k0 in range(0, K, 65535):
            _lib.call("sam6d_masks_resize_bilinear", m8.data_ptr() + k0 * h * w, min(65535, K - k0), h, w, H, W,
                      out.data_ptr() + 4 * k0 * H * W, _s())
    return out


def resize_masks_eager(masks, size):
    """`resize_masks` as the reference computes it (ISM/model/sam.py:86-93), on the masks' device (CPU included)."""
    K, h, w, H, W = _masks_sizes(masks, size, "resize_masks_eager")
    if K == 0:
        return torch.zeros((0, H, W), dtype=torch.float32, device=masks.device)
    return F.interpolate((masks != 0).unsqueeze(1).float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0]


# ------------------------------------------------------------------------------------------------- min_mask_region_area
REGIONS_WS_BYTES = 256 << 20   # the most workspace one launch group gets; K is processed in slices that fit (one mask always does)
REGIONS_MAX_K = 65535


def _masks_u8(masks, who):
    """(K, H, W) bool / uint8 / float32 on a HIP device -> a fresh contiguous uint8 tensor of 0 / 1 that the entries may overwrite."""
    _need_hip(masks, who)
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8, torch.float32):
        raise ValueError("%s: masks must be (K, H, W) bool, uint8 or float32, got %s %s" % (who, tuple(masks.shape), masks.dtype))
    if masks.shape[1] == 0 or masks.shape[2] == 0:
        raise ValueError("%s: empty image %s" % (who, tuple(masks.shape)))
    if masks.dtype == torch.bool:
        return masks.contiguous().view(torch.uint8).clone()
    return (masks != 0).to(torch.uint8)


def _region_slices(K, H, W, bytes_of):
    """K in slices whose workspace stays under REGIONS_WS_BYTES (and under the entries' K <= 65535): (k0, k, workspace bytes)."""
    per = int(bytes_of(1, H, W))
    if per == 0:
        raise ValueError("masks of %d x %d: H * W must be at most 2^31 - 2" % (H, W))
    step = max(1, min(REGIONS_MAX_K, REGIONS_WS_BYTES // per))
    return [(k0, min(step, K - k0), int(bytes_of(min(step, K - k0), H, W))) for k0 in range(0, K, step)]


def mask_components(masks, invert=False):
    """sam6d_mask_components.  masks (K, H, W) bool / uint8 / float32 on a HIP device; the foreground is masks != 0, or masks == 0 with
    `invert` -> (labels, areas), both (K, H, W) int32: labels = 0 off the foreground, else 1 + the smallest row-major pixel index of the
    pixel's 8-connected component; areas = that component's pixel count, 0 off the foreground.  Asynchronous."""
    m8 = _masks_u8(masks, "mask_components")
    K, H, W = m8.shape
    dev = m8.device
    labels = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    areas = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    if K == 0:
        return labels, areas
    with torch.cuda.device(dev):
        slices = _region_slices(K, H, W, _lib.load().sam6d_mask_components_workspace_bytes)
        ws = torch.empty((slices[0][2],), dtype=torch.uint8, device=dev)  # the first slice is the largest
        for k0, k, nbytes in slices:
            _lib.call("sam6d_mask_components", _p(m8[k0:]), k, H, W, int(bool(invert)), _p(labels[k0:]), _p(areas[k0:]), _p(ws),
                      nbytes, _s())
    return labels, areas


def region_threshold(min_area):
    """The integer threshold of `size < min_area` for integer sizes: ceil(min_area), at least 1 (nothing is below a threshold <= 0, and
    nothing is below 1 either: a component has at least one pixel)."""
    return max(1, int(math.ceil(min_area)))


def remove_small_regions(masks, min_area):
    """remove_small_regions (ISM/segment_anything/utils/amg.py:267-291) in its two modes, as postprocess_small_regions chains them
    (automatic_mask_generator.py:344-349), for all masks at once: holes smaller than min_area are filled, then islands smaller than
    min_area are dropped (the largest island stays where all are smaller; among equals, the first in row-major order).  masks
    (K, H, W) bool / uint8 / float32 (0 / 1) on a HIP device -> (cleaned masks of the same dtype, changed (K) bool, boxes (K, 4) int64
    xyxy of the cleaned masks, [0, 0, 0, 0] for an empty one).  The input is left as it is.  Asynchronous."""
    m8 = _masks_u8(masks, "remove_small_regions")
    K, H, W = m8.shape
    dev = m8.device
    thr = region_threshold(min_area)
    if thr > 2147483647:
        thr = 2147483647  # above every possible size
    changed = torch.zeros((K,), dtype=torch.uint8, device=dev)
    box = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    if K == 0:
        return masks.clone(), changed.view(torch.bool), box.long()
    with torch.cuda.device(dev):
        slices = _region_slices(K, H, W, _lib.load().sam6d_amg_small_regions_workspace_bytes)
        ws = torch.empty((slices[0][2],), dtype=torch.uint8, device=dev)  # the first slice is the largest
        for k0, k, nbytes in slices:
            _lib.call("sam6d_amg_small_regions", _p(m8[k0:]), k, H, W, thr, _p(changed[k0:]), _p(box[k0:]), _p(ws), nbytes, _s())
    cleaned = m8.view(torch.bool) if masks.dtype == torch.bool else m8.to(masks.dtype)
    return cleaned, changed.view(torch.bool), box.long()


def postprocess_small_regions(mask_data, min_area, nms_thresh):
    """postprocess_small_regions (ISM/segment_anything/automatic_mask_generator.py:324-372) on the device: mask_data = {"masks" (K, H, W),
    "boxes" (K, 4)} -> {"masks", "boxes"} of the survivors of an NMS over the cleaned masks' boxes that prefers unchanged masks (score
    1) to changed ones (score 0), in NMS order (score descending, stable by index); a changed survivor carries its new box, an
    unchanged one the box it came with.  One 4-byte read-back (how many the NMS kept)."""
    masks = mask_data["masks"]
    if len(masks) == 0:
        return mask_data
    cleaned, changed, boxes = remove_small_regions(masks, min_area)
    keep = nms(boxes.float(), (~changed).float(), nms_thresh)
    old = mask_data["boxes"]
    out_boxes = torch.where(changed[:, None], boxes.to(old.dtype), old)
    return {"masks": cleaned[keep], "boxes": out_boxes[keep]}


# ------------------------------------------------------------------------------------------------- one crop
class CropState:
    """What one crop of the generator needs: its settings and, on a HIP device, the fixed-capacity device buffers that the point batches
    fill (n_points * 3 proposals: packed masks, counts, boxes, scores, points, keep flags).  On any other device, or with
    SAM6D_HIP_AMG=0, the batches are kept as eager results instead."""

    def __init__(self, crop_box, orig_size, img_size, n_points, device, mask_threshold=0.0, stability_score_offset=1.0,
                 pred_iou_thresh=0.88, stability_score_thresh=0.95, hip=None):
        self.crop_box = [int(v) for v in crop_box]
        self.orig_size = (int(orig_size[0]), int(orig_size[1]))
        x0, y0, x1, y1 = self.crop_box
        self.crop_size = (y1 - y0, x1 - x0)
        self.img_size = int(img_size)
        self.input_size = preprocess_shape(self.crop_size[0], self.crop_size[1], self.img_size)
        self.mask_threshold = float(mask_threshold)
        self.stability_score_offset = float(stability_score_offset)
        self.pred_iou_thresh = float(pred_iou_thresh)
        self.stability_score_thresh = float(stability_score_thresh)
        self.device = torch.device(device)
        self.hip = hip_enabled(self.device) if hip is None else bool(hip)
        self.capacity = int(n_points) * MASKS_PER_POINT
        self.filled = 0
        self.parts = []  # the eager path's per-batch results
        if self.hip:
            dev, C = self.device, self.capacity
            oh, ow = self.crop_size
            z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
            self.out = dict(n_hi=z(C), n_lo=z(C), area=z(C), box=z(C, 4), bits=torch.empty((C, oh, words(ow)), dtype=torch.int32, device=dev))
            self.iou = torch.zeros(C, dtype=torch.float32, device=dev)
            self.stability = torch.zeros(C, dtype=torch.float32, device=dev)
            self.points = torch.zeros((C, 2), dtype=torch.float64, device=dev)
            self.keep = torch.zeros(C, dtype=torch.uint8, device=dev)
            self._crop = torch.tensor(self.crop_box, dtype=torch.float32, device=dev)
            self._orig = torch.tensor([0, 0, self.orig_size[1], self.orig_size[0]], dtype=torch.float32, device=dev)
            self._off = torch.tensor([x0, y0, x0, y0], dtype=torch.int32, device=dev)

    def settings(self):
        return dict(crop_box=self.crop_box, orig_size=self.orig_size, img_size=self.img_size, mask_threshold=self.mask_threshold,
                    stability_score_offset=self.stability_score_offset, pred_iou_thresh=self.pred_iou_thresh,
                    stability_score_thresh=self.stability_score_thresh)


def _flat(low, iou_preds, points, device):
    if low.dim() == 4:
        low = low.flatten(0, 1)
    iou = iou_preds.reshape(-1)
    per = low.shape[0] // max(1, len(points))
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.asarray(points, dtype=np.float64))
    pts = points.to(device=device, dtype=torch.float64).repeat_interleave(per, dim=0)
    return low, iou, pts


def process_batch(low, iou_preds, state, points):
    """_process_batch from the decoder's output onwards (automatic_mask_generator.py:286-321): low (B, 3, lh, lw) logits, iou_preds
    (B, 3), points (B, 2) xy in the crop (a host array, or a tensor: one already on the device costs no upload).  On the library path everything lands in the crop's device buffers and
    nothing is read back; otherwise the eager result of the batch is kept."""
    low, iou, pts = _flat(low, iou_preds, points, low.device)
    if not state.hip:
        state.parts.append(eager_batch(low, iou, pts, **state.settings()))
        return
    M, a = low.shape[0], state.filled
    if a + M > state.capacity:
        raise ValueError("process_batch: %d proposals exceed the crop's capacity of %d" % (a + M, state.capacity))
    b = a + M
    live = iou > state.pred_iou_thresh if state.pred_iou_thresh > 0.0 else torch.ones_like(iou, dtype=torch.bool)
    out = {k: v[a:b] for k, v in state.out.items()}
    mask_stats(low.float(), live, state.input_size, state.crop_size, state.img_size, state.mask_threshold, state.stability_score_offset, out=out)
    stab = out["n_hi"] / out["n_lo"]  # int32 / int32 true division, as calculate_stability_score returns it
    keep = live
    if state.stability_score_thresh > 0.0:
        keep = keep & (stab >= state.stability_score_thresh)
    boxes = (out["box"] + state._off).float()
    near_crop = (boxes - state._crop).abs() <= EDGE_ATOL
    near_image = (boxes - state._orig).abs() <= EDGE_ATOL
    keep = keep & ~(near_crop & ~near_image).any(dim=1)
    state.iou[a:b] = iou
    state.stability[a:b] = stab
    state.points[a:b] = pts
    state.keep[a:b] = keep.to(torch.uint8)
    state.filled = b


def _empty_result(state, dev, mask_dtype):
    H, W = state.orig_size
    return dict(masks=torch.zeros((0, H, W), dtype=mask_dtype, device=dev), boxes=torch.zeros((0, 4), dtype=torch.int64, device=dev),
                iou_preds=torch.zeros(0, dtype=torch.float32, device=dev), stability_score=torch.zeros(0, dtype=torch.float32, device=dev),
                points=torch.zeros((0, 2), dtype=torch.float64, device=dev))


def finish_crop(state, crop_box=None, orig_size=None, box_nms_thresh=0.7, mask_dtype=torch.bool):
    """The end of _process_crop (automatic_mask_generator.py:250-264) and the masks of ISM/model/sam.py:146-148: NMS inside the crop,
    boxes and points back in the image frame, masks (K, H, W) of the whole image.  -> {"masks", "boxes" (K, 4) int64 xyxy, "iou_preds",
    "stability_score", "points"} on the device, in NMS order (score descending).  crop_box / orig_size, when given, must be the state's."""
    if crop_box is not None and [int(v) for v in crop_box] != state.crop_box:
        raise ValueError("finish_crop: crop_box %s is not the state's %s" % (list(crop_box), state.crop_box))
    if orig_size is not None and (int(orig_size[0]), int(orig_size[1])) != state.orig_size:
        raise ValueError("finish_crop: orig_size %s is not the state's %s" % (tuple(orig_size), state.orig_size))
    if not state.hip:
        return _eager_finish(state.parts, state, box_nms_thresh, mask_dtype)
    n = state.filled
    if n == 0:
        return _empty_result(state, state.device, mask_dtype)
    idx = mask_to_indices(state.keep[:n])                                        # read-back 1: proposals the filters kept
    order = nms(state.out["box"][:n][idx].float(), state.iou[:n][idx], box_nms_thresh)  # read-back 2: proposals NMS kept
    sel = idx[order]
    x0, y0 = state.crop_box[:2]
    masks = unpack_masks(state.out["bits"], sel, state.crop_size, state.crop_box, state.orig_size, mask_dtype)
    boxes = state.out["box"][sel].long() + torch.tensor([x0, y0, x0, y0], device=state.device)
    pts = state.points[sel] + torch.tensor([x0, y0], device=state.device)
    return dict(masks=masks, boxes=boxes, iou_preds=state.iou[sel], stability_score=state.stability[sel], points=pts)


def merge_crops(results, crop_box_list, crop_nms_thresh=0.7):
    """ISM/model/sam.py:133-144 for crop_n_layers > 0: the crops' results concatenated, then NMS across crops that prefers the proposals
    of smaller crops (score 1 / box_area(crop_box))."""
    keys = ("masks", "boxes", "iou_preds", "stability_score", "points")
    data = {k: torch.cat([r[k] for r in results], dim=0) for k in keys}
    dev = data["boxes"].device
    cb = torch.cat([torch.tensor([list(b)] * len(r["boxes"]), dtype=torch.int64).reshape(-1, 4) for r, b in zip(results, crop_box_list)])
    data["crop_boxes"] = cb.to(dev)
    if len(results) > 1:
        scores = (1 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]))).to(dev)
        if hip_enabled(dev):
            keep = nms(data["boxes"].float(), scores, crop_nms_thresh)
        else:
            keep = nms_torch(data["boxes"].float(), scores, crop_nms_thresh)
        data = {k: v[keep] for k, v in data.items()}
    return data


# ------------------------------------------------------------------------------------------------- the same tail in plain torch
def postprocess_masks(low, input_size, crop_size, img_size):
    """Sam.postprocess_masks (modeling/sam.py:133-162) for low (M, lh, lw): both interpolations as torch does them, in low's dtype."""
    m = F.interpolate(low[:, None], (img_size, img_size), mode="bilinear", align_corners=False)
    m = m[..., : input_size[0], : input_size[1]]
    return F.interpolate(m, tuple(crop_size), mode="bilinear", align_corners=False)[:, 0]


def mask_boxes(masks):
    """batched_mask_to_box (amg.py:303-346) for (M, h, w) bool masks: (M, 4) int64 xyxy, [0, 0, 0, 0] for an empty mask."""
    M, h, w = masks.shape
    if masks.numel() == 0:
        return torch.zeros((M, 4), dtype=torch.int64, device=masks.device)
    in_h = masks.any(dim=2)
    ys = torch.arange(h, device=masks.device)[None, :]
    bottom = (in_h * ys).max(dim=1).values
    top = (in_h * ys + h * (~in_h)).min(dim=1).values
    in_w = masks.any(dim=1)
    xs = torch.arange(w, device=masks.device)[None, :]
    right = (in_w * xs).max(dim=1).values
    left = (in_w * xs + w * (~in_w)).min(dim=1).values
    empty = (right < left) | (bottom < top)
    return torch.stack([left, top, right, bottom], dim=1) * (~empty)[:, None]


def box_near_crop_edge(boxes, crop_box, orig_box, atol=EDGE_ATOL):
    """is_box_near_crop_edge (amg.py:78-88); boxes in the crop's frame."""
    dev = boxes.device
    x0, y0 = crop_box[0], crop_box[1]
    b = (boxes + torch.tensor([x0, y0, x0, y0], device=dev)).float()
    near_crop = (b - torch.tensor(crop_box, dtype=torch.float32, device=dev)).abs() <= atol
    near_image = (b - torch.tensor(orig_box, dtype=torch.float32, device=dev)).abs() <= atol
    return (near_crop & ~near_image).any(dim=1)


def stability_counts(logits, thr, offset):
    """The two sums of calculate_stability_score (amg.py:156-176) as int32."""
    hi = (logits > (thr + offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    lo = (logits > (thr - offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    return hi, lo


def eager_batch(low, iou_preds, points, crop_box, orig_size, img_size, mask_threshold=0.0, stability_score_offset=1.0,
                pred_iou_thresh=0.88, stability_score_thresh=0.95):
    """One point batch as the reference works through it, filter by filter: low (M, lh, lw), iou_preds (M), points (M, 2) ->
    {"masks" (k, H, W) bool in the image frame, "boxes" (k, 4) int64 in the crop's frame, "iou_preds", "stability_score", "points"}."""
    x0, y0, x1, y1 = crop_box
    H, W = orig_size
    crop_size = (y1 - y0, x1 - x0)
    input_size = preprocess_shape(crop_size[0], crop_size[1], img_size)
    if pred_iou_thresh > 0.0:
        k = iou_preds > pred_iou_thresh
        low, iou_preds, points = low[k], iou_preds[k], points[k]
    logits = postprocess_masks(low, input_size, crop_size, img_size)
    hi, lo = stability_counts(logits, mask_threshold, stability_score_offset)
    stab = hi / lo
    if stability_score_thresh > 0.0:
        k = stab >= stability_score_thresh
        logits, iou_preds, points, stab = logits[k], iou_preds[k], points[k], stab[k]
    masks = logits > mask_threshold
    boxes = mask_boxes(masks)
    k = ~box_near_crop_edge(boxes, crop_box, [0, 0, W, H])
    masks, boxes, iou_preds, points, stab = masks[k], boxes[k], iou_preds[k], points[k], stab[k]
    if not (x0 == 0 and y0 == 0 and x1 == W and y1 == H):
        masks = F.pad(masks, (x0, W - x1, y0, H - y1), value=0)
    return dict(masks=masks, boxes=boxes, iou_preds=iou_preds, stability_score=stab, points=points)


def nms_torch(boxes, scores, thresh):
    """torchvision.ops.nms restated: boxes (N, 4) float xyxy, scores (N) -> kept indices, score descending (stable).  The IoU matrix in
    torch ops on the boxes' device, the greedy pass on the host."""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    over = ((inter / (area[:, None] + area[None, :] - inter)) > thresh).cpu().numpy()
    removed = np.zeros(n, dtype=bool)
    kept = []
    for i in range(n):
        if not removed[i]:
            kept.append(i)
            removed[i + 1:] |= over[i, i + 1:]
    return order[torch.as_tensor(kept, dtype=torch.int64, device=boxes.device)]


def _eager_finish(parts, state, box_nms_thresh, mask_dtype):
    dev = state.device
    if not parts:
        return _empty_result(state, dev, mask_dtype)
    data = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
    keep = nms_torch(data["boxes"].float(), data["iou_preds"], box_nms_thresh)
    data = {k: v[keep] for k, v in data.items()}
    x0, y0 = state.crop_box[:2]
    data["boxes"] = data["boxes"] + torch.tensor([x0, y0, x0, y0], device=data["boxes"].device)
    data["points"] = data["points"] + torch.tensor([x0, y0], device=data["points"].device)
    data["masks"] = data["masks"].to(mask_dtype)
    return data


def eager_tail(batches, crop_box, orig_size, img_size, box_nms_thresh=0.7, mask_dtype=torch.bool, **settings):
    """The whole tail of one crop in plain torch ops, on whatever device the inputs are on.  batches: an iterable of (low, iou_preds,
    points) as process_batch takes them; settings: mask_threshold, stability_score_offset, pred_iou_thresh, stability_score_thresh.
    -> the dict finish_crop returns."""
    state = None
    for low, iou_preds, points in batches:
        if state is None:
            state = CropState(crop_box, orig_size, img_size, 0, low.device, hip=False, **settings)
        low, iou, pts = _flat(low, iou_preds, points, low.device)
        state.parts.append(eager_batch(low, iou, pts, **state.settings()))
    if state is None:
        raise ValueError("eager_tail: no batches")
    return _eager_finish(state.parts, state, box_nms_thresh, mask_dtype)
