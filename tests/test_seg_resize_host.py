"""CPU checks of DESIGN section 8 row f11, the two resizes of `segmentor_width_size`: the rectangular numpy restatement of
cv2.resize (tests/cv2_resize_ref.py) against the square one that pins the rgb crops, a float64 bilinear, its special cases and cv2
itself where it imports; the package's plain-torch partners against the restatements; the drop-in's switch; the kernels' resources.

PARITY UNPINNED against cv2: it is not installed where this suite usually runs and the checkout holds no recorded cv2 output for whole
images, so test_restatement_matches_cv2 runs only where cv2 imports."""
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from tests import cv2_linear as CV
from tests import cv2_resize_ref as R


@pytest.mark.parametrize("S", [2, 7, 64, 224])
def test_restatement_equals_the_square_one(S):
    """Square targets from sources 2S (the area path), S (the copy), odd and smaller than S."""
    for n, side in enumerate((2 * S, S, 2 * S + 1, 3 * S + 2, max(1, S // 2), max(1, S - 1))):
        for src in (R.noise(100 * S + n, side, side), R.stripes(side, side)):
            assert np.array_equal(R.resize(src, S, S), CV.resize_linear(src, S)), (S, side)


@pytest.mark.parametrize("geom", R.GEOMETRIES + [R.FULL], ids=lambda g: "%dx%d-%d" % g)
def test_restatement_within_one_level_of_float64(geom):
    H, W, width = geom
    h, w = R.resized_shape((H, W), width)
    for src in (R.noise(H + W, H, W), R.stripes(H, W)):
        got = R.resize(src, h, w)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        if (H, W) == (2 * h, 2 * w):
            continue  # the area path is not a bilinear sample
        d = np.abs(got.astype(np.float64) - R.bilinear_f64(src, h, w))
        assert d.max() <= 1.0, (geom, d.max())


def test_restatement_special_cases():
    src = R.noise(5, 48, 64)
    assert np.array_equal(R.resize(src, 48, 64), src)
    big = R.noise(6, 96, 128)
    s = big.astype(np.int64)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize(big, 48, 64), want.astype(np.uint8))
    assert np.array_equal(R.resize_width(big, 64), want.astype(np.uint8))
    with pytest.raises(ValueError):
        R.resize(R.noise(7, 2, 3), 0, 1)


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_restatement_matches_cv2(geom):
    """tests/test_rgb_inputs.py's criterion: at most one level (OpenCV's scalar row tail), at least 99 % exact."""
    cv2 = pytest.importorskip("cv2")
    H, W, width = geom
    h, w = R.resized_shape((H, W), width)
    src = R.noise(H * W, H, W)
    d = np.abs(R.resize(src, h, w).astype(np.int64) - cv2.resize(src, (w, h)).astype(np.int64))
    assert d.max() <= 1 and (d == 0).mean() >= 0.99


@pytest.mark.parametrize("geom", R.GEOMETRIES + [R.FULL], ids=lambda g: "%dx%d-%d" % g)
def test_resize_image_eager_equals_restatement(geom):
    from sam6d_hip import amg
    H, W, width = geom
    size = amg.resized_shape((H, W), width)
    assert size == R.resized_shape((H, W), width)
    for src in (R.noise(H + 3 * W, H, W), R.stripes(H, W)):
        got = amg.resize_image_eager(torch.from_numpy(src), size)
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), R.resize(src, *size)), geom
    wide = torch.from_numpy(R.noise(1, H, W + 5))  # a crop view: the result does not depend on the stride
    assert torch.equal(amg.resize_image_eager(wide[:, 2:W + 2], size), amg.resize_image_eager(wide[:, 2:W + 2].contiguous(), size))


def test_resize_image_refusals():
    from sam6d_hip import amg
    img = torch.zeros((2, 3, 3), dtype=torch.uint8)
    assert amg.resized_shape((2, 3), 1) == (0, 1)
    for fn in (amg.resize_image_eager, amg.resize_image):
        with pytest.raises(ValueError, match="at least 1"):
            fn(img, amg.resized_shape((2, 3), 1))
        with pytest.raises(ValueError, match="3 channels"):
            fn(torch.zeros((4, 4, 4), dtype=torch.uint8), (2, 2))
        with pytest.raises(ValueError, match="uint8"):
            fn(torch.zeros((4, 4, 3)), (2, 2))
        with pytest.raises(ValueError, match="1 .. 4096"):
            fn(torch.zeros((1, 4097, 3), dtype=torch.uint8), (1, 8))
        with pytest.raises(ValueError, match="1 .. 4096"):
            fn(img, (1, 4097))
    with pytest.raises(RuntimeError, match="HIP device"):
        amg.resize_image(img, (1, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        amg.resize_masks(torch.zeros((1, 2, 2), dtype=torch.bool), (4, 4))
    for fn in (amg.resize_masks_eager, amg.resize_masks):
        with pytest.raises(ValueError, match="bool or uint8"):
            fn(torch.zeros((1, 2, 2)), (4, 4))
        with pytest.raises(ValueError, match="1 .. 8192"):
            fn(torch.zeros((1, 2, 2), dtype=torch.bool), (8193, 4))
        with pytest.raises(ValueError, match="1 .. 8192"):
            fn(torch.zeros((1, 2, 2), dtype=torch.bool), (0, 4))


# (h, w, H, W): 3x, 2x in one axis only, shrinking, one pixel, equal sizes
MASK_SHAPES = [(45, 80, 135, 240), (48, 64, 97, 128), (48, 64, 30, 40), (1, 1, 5, 7), (48, 64, 48, 64)]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_masks_eager_within_fp32_rounding(shape):
    """fp32 rounding, from the formats alone.  (a) Seven fp32 operations on values in [0, 1] (four products, three sums), each rounding
    by at most half an ulp of 1.0 = 2^-24: 7 * 2^-24 = 4.2e-7 against the same taps combined in float64.  (b) The source coordinate
    scale * (dst + 0.5) - 0.5 < n is itself an fp32 product and difference: torch's CPU build may fuse them (one rounding) where the
    restatement rounds twice, which moves the coordinate, and with it a weight, by at most one ulp of a value below n; a weight that
    moves by e moves the value by at most e (the taps are 0 or 1).  One such ulp per axis."""
    from sam6d_hip import amg
    h, w, H, W = shape
    masks = R.mask_patterns(5, h, w)
    want = R.masks_bilinear(masks, H, W)
    bound = 7 * 2.0 ** -24 + sum(float(np.spacing(np.nextafter(np.float32(n), np.float32(0)))) for n in (h, w))
    for t in (torch.from_numpy(masks), torch.from_numpy(masks.astype(np.uint8) * 255)):
        got = amg.resize_masks_eager(t, (H, W))
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, H, W)
        d = np.abs(got.numpy().astype(np.float64) - want).max()
        print("\n[seg_resize] %s: max |eager - restatement| = %.3e (bound %.3e)" % (shape, d, bound))
        assert d <= bound, (shape, d, bound)
    if (h, w) == (H, W):
        assert np.array_equal(want, masks.astype(np.float64))
    assert tuple(amg.resize_masks_eager(torch.zeros((0, h, w), dtype=torch.bool), (H, W)).shape) == (0, H, W)


def test_resized_shape_is_the_references_expression():
    from sam6d_hip import amg
    for (H, W), width in (((480, 640), 640), ((1080, 1920), 640), ((960, 1280), 640), ((1000, 1333), 640), ((53, 37), 64), ((2, 3), 1),
                          ((720, 1281), 640.0)):
        assert amg.resized_shape((H, W), width) == (int(width * H / W), int(width))
    assert amg.resized_shape((1000, 1333), 640) == (480, 640)  # 640 * 1000 / 1333 = 480.12: W is no multiple of the width


def test_dropin_switch():
    """The signature still starts with the reference's eight parameters, hip_resize is the last keyword, it follows SAM6D_HIP_SEGRESIZE
    when None, and on a CPU model it raises, naming the switch."""
    mod = importlib.import_module("model.sam")
    from tests.sam_amg_stub import StubSam, encode_image
    sig = inspect.signature(mod.CustomSamAutomaticMaskGenerator.__init__)
    want = [("sam", inspect.Parameter.empty), ("min_mask_region_area", 0), ("points_per_batch", 64), ("stability_score_thresh", 0.85),
            ("box_nms_thresh", 0.7), ("crop_overlap_ratio", 512 / 1500), ("segmentor_width_size", None), ("pred_iou_thresh", 0.88)]
    got = [(k, p.default) for k, p in list(sig.parameters.items())[1:]]
    assert got[:len(want)] == want and got[-1] == ("hip_resize", None), got
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image).hip_resize is False
    with pytest.raises(RuntimeError, match="SAM6D_HIP_SEGRESIZE"):
        mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, segmentor_width_size=160, hip_resize=True)
    old = os.environ.get("SAM6D_HIP_SEGRESIZE")
    os.environ["SAM6D_HIP_SEGRESIZE"] = "1"
    try:
        with pytest.raises(RuntimeError, match="SAM6D_HIP_SEGRESIZE"):
            mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image)
        assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_resize=False).hip_resize is False
    finally:
        if old is None:
            del os.environ["SAM6D_HIP_SEGRESIZE"]
        else:
            os.environ["SAM6D_HIP_SEGRESIZE"] = old


def test_kernel_resources():
    """the mask kernel keeps within 64 VGPRs (eight waves per SIMD) and uses no scratch; the image kernel
    uses no scratch and keeps within 48 VGPRs (built: 43)."""
    from tests._util import kernel_resources
    found = kernel_resources(b"seg_masks_resize_kernel", r"(seg_(?:masks|image)_resize_kernel)")
    assert set(found) == {"seg_masks_resize_kernel", "seg_image_resize_kernel"}, found
    print("\n[seg_resize] (VGPRs, scratch bytes, spilled): %s" % (found,))
    assert found["seg_masks_resize_kernel"][0] <= 64 and found["seg_masks_resize_kernel"][1:] == (0, 0), found
    assert found["seg_image_resize_kernel"][0] <= 48 and found["seg_image_resize_kernel"][1:] == (0, 0), found
