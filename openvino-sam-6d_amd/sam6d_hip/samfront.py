"""SAM's image front on the library: the (H, W, 3) uint8 image -> the preprocessed tensor `sam.image_encoder` is called on, or the
patch rows the encoder's first GEMM reads, in one launch (csrc/samfront.hip).

Reference: ResizeLongestSide.apply_image (ISM/segment_anything/utils/transforms.py:26-31, get_preprocess_shape :91-102: torchvision's
resize of a PIL image, i.e. Pillow's 8-bit bilinear ImagingResample), SamPredictor.set_image (predictor.py:56-58, 88) and
Sam.preprocess (modeling/sam.py:164-173).  Pillow's resample is integer arithmetic once the per-axis coefficients are known: `tables`
computes them in float64 as Resample.c's precompute_coeffs and normalize_coeffs_8bpc do, the kernel and `eager` (the same steps as
integer gathers and sums in plain torch, on any device) do the two passes, the fp32 subtraction and division, and the zero padding.
The results are the reference's bit for bit (tests/test_sam_front_host.py, tests/test_sam_front_gpu.py).

Limits, refused by name: H, W 1 .. 4096; side a multiple of 16 up to 1024; at most 9 taps per axis (shrinking by up to 4, which is
what 4096 pixels at side 1024 need); and images more than 100 times as tall as wide that shrink vertically, for which Pillow's
Image.resize (12.2.0) runs the vertical pass first -- both routes here always run the horizontal pass first.
"""
import functools

import numpy as np
import torch

from . import _lib, amg
from .runtime import _empty, _p, _s, on_tensor_device

PRECISION_BITS = 22
MAX_TAPS = 9
MAX_SIZE = 4096
LAYOUTS = {"x": 0, "rows": 1}  # SAM6D_SAM_FRONT_X, SAM6D_SAM_FRONT_ROWS (include/sam6d_hip.h)


@functools.lru_cache(maxsize=256)
def tables(in_size, out_size):
    """Pillow's coefficients for resampling an axis of in_size pixels to out_size with the bilinear filter (Resample.c,
    precompute_coeffs and normalize_coeffs_8bpc), in float64: (lo (out,), count (out,), k (out, taps)) int32 numpy arrays, read-only;
    taps = the largest count, k is zero behind a row's count."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sam6d_hip.samfront: cannot resample %d pixels to %d" % (in_size, out_size))
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale  # (the bilinear filter's own support is 1)
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (int() of the C code: truncation; negative values are cut to 0 anyway)
    hi = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = hi - lo
    taps = int(count.max())
    j = np.arange(taps, dtype=np.int64)[None, :]
    t = np.abs((j + lo[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (j < count[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for c in range(taps):  # (left to right, as the C loop sums)
        ww = ww + w[:, c]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    k[j >= count[:, None]] = 0
    out = tuple(a.astype(np.int32) for a in (lo, count, k))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def _device_table(in_size, out_size, device):
    """`tables` as the kernel reads them: one int32 tensor [lo | count | k] on `device`, and the number of taps."""
    lo, count, k = tables(in_size, out_size)
    return torch.from_numpy(np.concatenate([lo, count, k.reshape(-1)])).to(device), int(k.shape[1])


def _floats3(v, name):
    """Three fp32 values as Python floats: a sequence, or a tensor such as Sam.pixel_mean (3, 1, 1)."""
    if torch.is_tensor(v):
        v = v.detach().to(torch.float32).reshape(-1).cpu().numpy()
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    if v.shape[0] != 3:
        raise ValueError("sam6d_hip.samfront: %s must have 3 values, got %d" % (name, v.shape[0]))
    return [float(x) for x in v]


def _check(image, side, layout):
    """-> (image as (B, H, W, 3), (oh, ow))."""
    if not torch.is_tensor(image) or image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3:
        raise ValueError("sam6d_hip.samfront: the image must be a uint8 tensor (H, W, 3) or (B, H, W, 3), got %s %s"
                         % (getattr(image, "dtype", type(image).__name__), tuple(getattr(image, "shape", ()))))
    if layout not in LAYOUTS:
        raise ValueError("sam6d_hip.samfront: layout must be 'x' or 'rows', got %r" % (layout,))
    side = int(side)
    if side < 16 or side > 1024 or side % 16:
        raise ValueError("sam6d_hip.samfront: side must be a multiple of 16, 16 .. 1024, got %d" % side)
    img = image if image.dim() == 4 else image[None]
    H, W = int(img.shape[1]), int(img.shape[2])
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError("sam6d_hip.samfront: H and W must be 1 .. %d, got %d x %d" % (MAX_SIZE, H, W))
    oh, ow = amg.preprocess_shape(H, W, side)
    if oh < 1 or ow < 1:
        raise ValueError("sam6d_hip.samfront: a %d x %d image resizes to %d x %d at side %d" % (H, W, oh, ow, side))
    if H > 100 * W and oh < H:
        raise NotImplementedError("sam6d_hip.samfront: a %d x %d image is more than 100 times as tall as wide and shrinks vertically: "
                                  "Pillow's Image.resize runs the vertical pass first there, which is not implemented" % (H, W))
    for n_in, n_out in ((W, ow), (H, oh)):
        taps = tables(n_in, n_out)[2].shape[1]
        if taps > MAX_TAPS:
            raise NotImplementedError("sam6d_hip.samfront: %d -> %d pixels needs %d taps per output (up to %d are implemented: "
                                      "shrinking by up to 4)" % (n_in, n_out, taps, MAX_TAPS))
    return img, (oh, ow)


@on_tensor_device
def preprocess(image, mean, std, side=1024, layout="x", reverse=False, options=None):
    """image: uint8 (H, W, 3) or (B, H, W, 3) on the HIP device (any row and image stride: a crop view is read in place); mean, std:
    three values each (sequences or tensors such as sam.pixel_mean), used in fp32; reverse: read the channels in the opposite order (an
    image whose format is not the model's image_format).
    layout "x":    (B, 3, side, side) float32 = sam.preprocess of the resized image (B = 1 for a single image).
    layout "rows": (B * (side / 16)^2, 768) float32 = the patch rows of that tensor (what sam6d_sam_patch_rows writes from it; for
                   side = 1024, samenc.encode_rows takes them)."""
    img, (oh, ow) = _check(image, side, layout)
    mean, std = _floats3(mean, "mean"), _floats3(std, "std")
    if img.stride(3) != 1 or img.stride(2) != 3 or img.stride(1) < 3 * img.shape[2] or (img.shape[0] > 1 and img.stride(0) < 0):
        img = img.contiguous()  # (a crop view of an image keeps its strides)
    B, H, W = (int(v) for v in img.shape[:3])
    g = side // 16
    out = _empty((B, 3, side, side) if layout == "x" else (B * g * g, 3 * 256), img)
    if B == 0:
        return out
    (xt, xtaps), (yt, ytaps) = _device_table(W, ow, img.device), _device_table(H, oh, img.device)
    _lib.call("sam6d_sam_front", img.data_ptr(), img.stride(1), img.stride(0) if B > 1 else 0, B, H, W, 1 if reverse else 0,
              xt.data_ptr(), xtaps, yt.data_ptr(), ytaps, *mean, *std, side, _p(out), LAYOUTS[layout], _s())
    return out


def eager(image, mean, std, side=1024, layout="x", reverse=False):
    """`preprocess` in plain torch on the image's device (CPU included): the same tables, the two passes as int32 gathers and sums, the
    bytes in between, the fp32 subtraction and division, the zero padding; the rows layout by a reshape."""
    img, (oh, ow) = _check(image, side, layout)
    dev = img.device
    mean = torch.tensor(_floats3(mean, "mean"), dtype=torch.float32, device=dev)
    std = torch.tensor(_floats3(std, "std"), dtype=torch.float32, device=dev)
    v = img.flip(-1) if reverse else img
    v = v.to(torch.int32)                                           # (B, H, W, 3)
    for axis, n_out in ((2, ow), (1, oh)):                          # horizontal, then vertical
        lo, _, k = (torch.from_numpy(a.copy()).to(dev) for a in tables(v.shape[axis], n_out))
        idx = (lo[:, None].long() + torch.arange(k.shape[1], device=dev)[None, :]).clamp(max=v.shape[axis] - 1)   # (out, taps); k = 0 behind the count
        v = v.movedim(axis, 1)                                      # (B, n_in, other, 3)
        acc = torch.full((v.shape[0], n_out) + tuple(v.shape[2:]), 1 << (PRECISION_BITS - 1), dtype=torch.int32, device=dev)
        for j in range(k.shape[1]):
            acc += v[:, idx[:, j]] * k[:, j].view(1, -1, 1, 1)
        v = (acc >> PRECISION_BITS).clamp(0, 255).movedim(1, axis)  # the pass's bytes
    x = (v.permute(0, 3, 1, 2).to(torch.float32) - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    x = torch.nn.functional.pad(x, (0, side - ow, 0, side - oh)).contiguous()  # (the permuted bytes made it channels-last)
    if layout == "x":
        return x
    g = side // 16
    return x.reshape(-1, 3, g, 16, g, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, 3 * 256)


def pixel_stats(sam):
    """(mean, std) of a Sam model as fp32 values: its pixel_mean / pixel_std buffers (modeling/sam.py:45-46)."""
    for name in ("pixel_mean", "pixel_std"):
        if not torch.is_tensor(getattr(sam, name, None)):
            raise AttributeError("sam6d_hip.samfront: the model has no tensor `%s` (Sam registers pixel_mean and pixel_std as buffers)" % name)
    return _floats3(sam.pixel_mean, "pixel_mean"), _floats3(sam.pixel_std, "pixel_std")


def upload(image, device):
    """A (H, W, 3) uint8 numpy array (or tensor) as a tensor on `device`."""
    if not torch.is_tensor(image):
        image = np.asarray(image)
        if image.dtype != np.uint8:
            raise ValueError("sam6d_hip.samfront: the image must be uint8, got %s" % image.dtype)
        image = torch.from_numpy(np.ascontiguousarray(image))
    return image.to(device)


def encode_image(sam, image):
    """The ready-made `encode_image` hook of the drop-in (ISM/model/sam.py): image (H, W, 3) uint8 in the model's image_format ->
    (sam.image_encoder(preprocessed image), the resized image's (h, w))."""
    side = int(sam.image_encoder.img_size)
    mean, std = pixel_stats(sam)
    img = upload(image, sam.device)
    x = preprocess(img, mean, std, side=side, layout="x")
    return sam.image_encoder(x), amg.preprocess_shape(int(img.shape[0]), int(img.shape[1]), side)
