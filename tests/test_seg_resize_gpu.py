"""DESIGN section 8 row f11 on the GPU: sam6d_image_resize_linear against the numpy restatement of cv2.resize (tests/cv2_resize_ref.py;
byte for byte), sam6d_masks_resize_bilinear against the restatement of F.interpolate's bilinear that forms the taps in fp32 and
combines them in float64, and the drop-in with hip_resize switched on.

THE MASK BOUND is not a fixed number: it is 4 x the deviation that resize_masks_eager (F.interpolate on the device) shows against the
same restatement on the same masks in the same test, with a floor of one ulp of 1.0 (1.2e-7): the project's rule for every fp32 row."""
import functools
import importlib
import importlib.util

import numpy as np
import pytest
import torch

from tests import cv2_resize_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64  # bytes / floats on either side of an output buffer
ULP1 = 1.2e-7


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _image_case(H, W, width, kind):
    """(image, size, restatement), computed once."""
    src = R.noise(7 * H + W, H, W) if kind == "noise" else R.stripes(H, W)
    size = R.resized_shape((H, W), width)
    return src, size, R.resize(src, *size)


# ---------------------------------------------------------------------------------------------- 1. the image
@pytest.mark.parametrize("geom", R.GEOMETRIES + [R.FULL], ids=lambda g: "%dx%d-%d" % g)
def test_image_kernel_equals_restatement(geom):
    from sam6d_hip import amg
    H, W, width = geom
    for kind in ("noise",) if geom == R.FULL else ("noise", "stripes"):
        src, size, want = _image_case(H, W, width, kind)
        assert amg.resized_shape((H, W), width) == size
        got = amg.resize_image(torch.from_numpy(src).to(_dev()), size)
        assert got.dtype == torch.uint8 and tuple(got.shape) == size + (3,) and got.is_contiguous()
        n = int((got.cpu().numpy() != want).sum())
        print("\n[seg_resize] image %d x %d -> %d x %d, %s: %d bytes differ from the restatement" % (H, W, size[0], size[1], kind, n))
        assert n == 0, (geom, kind)


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_image_crop_view_guards_and_alignment(geom):
    """A crop view with a row stride above 3 W is read in place and gives what its contiguous copy gives; the launch writes its output
    and nothing around it, from a 4-byte boundary (whole words) and from an odd address (bytes) alike."""
    from sam6d_hip import amg
    H, W, width = geom
    size = R.resized_shape((H, W), width)
    wide = R.noise(H * W + 1, H + 3, W + 9)
    crop = torch.from_numpy(wide).to(_dev())[2:H + 2, 5:W + 5]
    assert crop.stride(0) > 3 * W and not crop.is_contiguous()
    want = R.resize(np.ascontiguousarray(wide[2:H + 2, 5:W + 5]), *size)
    n = want.size
    for off in (GUARD, GUARD + 1):
        buf = torch.full((n + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device=_dev())
        out = buf[off:off + n].view(size + (3,))
        assert amg.resize_image(crop, size, out=out) is out
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all(), "the launch wrote outside its output"
        assert np.array_equal(got[off:off + n].reshape(want.shape), want), (geom, off)
    assert torch.equal(amg.resize_image(crop.contiguous(), size), out)


def test_image_refusals_write_nothing():
    from sam6d_hip import _lib, amg
    dev = _dev()
    img = torch.from_numpy(R.noise(3, 30, 40)).to(dev)
    buf = torch.full((48 * 64 * 3 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf.data_ptr() + GUARD

    def raw(**change):
        a = dict(src=img.data_ptr(), row_stride=img.stride(0), H=30, W=40, channels=3, dst=out, h=48, w=64, stream=_stream())
        assert not set(change) - set(a)
        a.update(change)
        _lib.call("sam6d_image_resize_linear", *a.values())

    cases = [(dict(channels=4), "3 channels"), (dict(channels=1), "3 channels"), (dict(H=0), "H and W"), (dict(W=4097), "H and W"),
             (dict(h=0), "at least 1"), (dict(h=-2), "at least 1"), (dict(w=0), "h and w"), (dict(h=4097), "h and w"), (dict(w=4097), "h and w"),
             (dict(src=None), "null"), (dict(dst=None), "null"), (dict(row_stride=119), "row_stride"),
             (dict(dst=img.data_ptr()), "alias"), (dict(dst=img.data_ptr() + 3599, h=1, w=1), "alias")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=text):
            raw(**change)
    small = torch.from_numpy(R.noise(4, 2, 3)).to(dev)
    assert amg.resized_shape((2, 3), 1) == (0, 1)
    with pytest.raises(ValueError, match="at least 1"):  # 2 x 3 -> width 1 -> 0 x 1: cv2 raises there
        amg.resize_image(small, amg.resized_shape((2, 3), 1))
    with pytest.raises(ValueError, match="contiguous"):
        amg.resize_image(img, (48, 64), out=torch.empty((48, 64, 6), dtype=torch.uint8, device=dev)[:, :, ::2])
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a refused call wrote to the output"
    raw()  # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert np.array_equal(buf[GUARD:-GUARD].cpu().numpy().reshape(48, 64, 3), R.resize(img.cpu().numpy(), 48, 64))


# ---------------------------------------------------------------------------------------------- 2. the masks
def _mask_bound(masks_dev, want, size):
    """4 x the deviation of F.interpolate on the device from the restatement `want`, at least one ulp of 1.0."""
    from sam6d_hip import amg
    if masks_dev.shape[0] == 0:
        return ULP1, 0.0
    eager = amg.resize_masks_eager(masks_dev, size)
    dev = float(np.abs(eager.cpu().numpy().astype(np.float64) - want).max())
    return max(4.0 * dev, ULP1), dev


def _check_masks(masks_np, size, label):
    """The kernel on bool masks against the restatement, the exactness properties, and the count of values that differ in bits from
    F.interpolate on the device (recorded, not a pass condition) -> the kernel's output."""
    from sam6d_hip import amg
    H, W = size
    m = torch.from_numpy(masks_np).to(_dev())
    want = R.masks_bilinear(masks_np, H, W)
    got = amg.resize_masks(m, size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (masks_np.shape[0], H, W) and got.is_contiguous()
    g = got.cpu().numpy()
    bound, eager_dev = _mask_bound(m, want, size)
    d = float(np.abs(g.astype(np.float64) - want).max()) if g.size else 0.0
    nbits = int((bits(g) != bits(amg.resize_masks_eager(m, size).cpu().numpy())).sum()) if g.size else 0
    print("\n[seg_resize] masks %s: max |kernel - restatement| = %.3e, F.interpolate's %.3e, bound %.3e; %d of %d values differ in bits "
          "from F.interpolate" % (label, d, eager_dev, bound, nbits, g.size))
    assert d <= bound, (label, d, bound)
    assert (bits(g[want == 0.0]) == 0).all(), "a pixel whose four taps are 0 must be exactly 0.0f"
    assert g.size == 0 or float(g.max()) <= 1.0
    return got


# (h, w, H, W): 3x, 2x in one axis only, shrinking, one pixel, equal sizes
MASK_SHAPES = [(45, 80, 135, 240), (48, 64, 97, 128), (48, 64, 30, 40), (1, 1, 5, 7), (48, 64, 48, 64)]


@pytest.mark.parametrize("K", [1, 3, 5, 0])
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_masks_kernel_against_restatement(shape, K):
    """K = 5 runs through every pattern: blobs, all zeros, all ones, a checkerboard, the four corner pixels."""
    from sam6d_hip import amg
    h, w, H, W = shape
    masks = R.mask_patterns(K, h, w, seed=K)
    got = _check_masks(masks, (H, W), "%d x %d x %d -> %d x %d" % (K, h, w, H, W))
    m = torch.from_numpy(masks).to(_dev())
    as01, as255 = m.to(torch.uint8), m.to(torch.uint8) * 255
    assert torch.equal(amg.resize_masks(as01, (H, W)), got) and torch.equal(amg.resize_masks(as255, (H, W)), got)
    if (h, w) == (H, W) and K:
        assert torch.equal(got, m.float())
    if K == 5:
        assert float(got[1].abs().max()) == 0.0 and bool((got[2] == 1.0).all())


def test_masks_full_size():
    masks = R.mask_patterns(2, 360, 640, seed=9)
    masks[1] = R.mask_patterns(4, 360, 640, seed=9)[3]  # blobs and the checkerboard
    _check_masks(masks, (1080, 1920), "2 x 360 x 640 -> 1080 x 1920")


@pytest.mark.parametrize("shape", [(45, 80, 135, 240), (48, 64, 97, 127), (48, 64, 30, 40)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_masks_guards_and_alignment(shape):
    """Guard floats round the output stay untouched, from a 16-byte boundary (16-byte stores where W % 4 == 0) and from a 4-byte one
    (single floats); both give the same bits."""
    from sam6d_hip import amg
    h, w, H, W = shape
    m = torch.from_numpy(R.mask_patterns(3, h, w, seed=2)).to(_dev())
    n = 3 * H * W
    res = []
    for off in (GUARD, GUARD + 1):
        buf = torch.full((n + 2 * GUARD + 1,), -7.5, device=_dev())
        out = buf[off:off + n].view(3, H, W)
        assert amg.resize_masks(m, (H, W), out=out) is out
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:off] == -7.5).all() and (got[off + n:] == -7.5).all(), "the launch wrote outside its output"
        res.append(got[off:off + n])
    assert np.array_equal(bits(res[0]), bits(res[1]))
    assert np.array_equal(bits(res[0]), bits(amg.resize_masks(m, (H, W)).cpu().numpy()).reshape(-1))


def test_masks_refusals_write_nothing():
    from sam6d_hip import _lib, amg
    dev = _dev()
    m = torch.ones((2, 4, 6), dtype=torch.uint8, device=dev)
    buf = torch.full((2 * 8 * 12 + 2 * GUARD,), -7.5, device=dev)
    out = buf.data_ptr() + 4 * GUARD

    def raw(**change):
        a = dict(masks=m.data_ptr(), K=2, h=4, w=6, H=8, W=12, out=out, stream=_stream())
        assert not set(change) - set(a)
        a.update(change)
        _lib.call("sam6d_masks_resize_bilinear", *a.values())

    cases = [(dict(K=-1), "K must be"), (dict(K=65536), "K must be"), (dict(h=0), "sizes"), (dict(w=8193), "sizes"), (dict(H=0), "sizes"),
             (dict(W=8193), "sizes"), (dict(H=-4), "sizes"), (dict(masks=None), "null"), (dict(out=None), "null"), (dict(out=out + 2), "aligned")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=text):
            raw(**change)
    raw(K=0, masks=None, out=None)  # nothing to do: returns without a launch
    with pytest.raises(ValueError, match="contiguous"):
        amg.resize_masks(m, (8, 12), out=torch.empty((2, 8, 24), device=dev)[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        amg.resize_masks(m, (8, 12), out=torch.empty((2, 8, 12), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    assert bool((buf == -7.5).all()), "a refused call wrote to the output"
    raw()
    torch.cuda.synchronize()
    assert bool((buf[GUARD:-GUARD] == 1.0).all()) and bool((buf[:GUARD] == -7.5).all()) and bool((buf[-GUARD:] == -7.5).all())


# ---------------------------------------------------------------------------------------------- 3. the drop-in
WIDTH = 160


def _generator(sam, **kw):
    mod = importlib.import_module("model.sam")
    return mod.CustomSamAutomaticMaskGenerator(sam, points_per_batch=256, **kw)


def _check_against_small_run(out, ref, image, small):
    """`out` of a generator with segmentor_width_size = WIDTH and hip_resize against `ref`, the result of one without
    segmentor_width_size on the restated small image: the same survivors in the same order, their boxes through the reference's scale
    and clamp, their masks through the mask restatement."""
    H, W = image.shape[:2]
    K = ref["masks"].shape[0]
    assert K >= 1 and ref["masks"].dtype == torch.bool and tuple(ref["masks"].shape[1:]) == small.shape[:2]
    assert out["masks"].dtype == torch.float32 and out["boxes"].dtype == torch.float32
    assert tuple(out["masks"].shape) == (K, H, W) and tuple(out["boxes"].shape) == (K, 4)
    assert torch.equal(out["boxes"], R.scale_boxes(ref["boxes"], (H, W), WIDTH))
    want = R.masks_bilinear(ref["masks"].cpu().numpy(), H, W)
    bound, eager_dev = _mask_bound(ref["masks"], want, (H, W))
    d = float(np.abs(out["masks"].cpu().numpy().astype(np.float64) - want).max())
    print("\n[seg_resize] drop-in %d x %d, %d masks: max |masks - restatement| = %.3e, F.interpolate's %.3e, bound %.3e" % (H, W, K, d, eager_dev, bound))
    assert d <= bound


@pytest.mark.parametrize("min_area", [0, 50])
@pytest.mark.parametrize("hw", [(240, 320), (360, 480)], ids=["2x", "3x"])
def test_dropin_with_hook(hw, min_area):
    from tests.sam_amg_stub import StubSam, encode_image
    image = R.noise(hw[0], *hw)
    small = R.resize_width(image, WIDTH)
    assert small.shape == (120, 160, 3)
    seen = []

    def hook(sam, img):
        seen.append(img)
        return encode_image(sam, img)

    sam = StubSam(_dev())
    out = _generator(sam, encode_image=hook, segmentor_width_size=WIDTH, min_mask_region_area=min_area, hip_resize=True).generate_masks(image)
    assert len(seen) == 1 and isinstance(seen[0], np.ndarray) and seen[0].dtype == np.uint8 and np.array_equal(seen[0], small)
    ref = _generator(sam, encode_image=encode_image, min_mask_region_area=min_area).generate_masks(small)
    _check_against_small_run(out, ref, image, small)


def test_dropin_with_front(monkeypatch):
    """hip_front behind hip_resize: the resized image stays on the device (set_image receives a tensor, the encoder's input is the
    front's of the restated small image), and the one upload of generate_masks is the original image's."""
    from sam6d_hip import samfront
    from tests.sam_amg_stub import StubSam, encode_image
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

    class Encoder:
        img_size = 1024

        def __init__(self):
            self.inputs = []

        def __call__(self, x):
            self.inputs.append(x)
            return None

    sam = StubSam(_dev())
    sam.image_encoder = Encoder()
    sam.pixel_mean = torch.tensor(mean, device=_dev()).view(-1, 1, 1)
    sam.pixel_std = torch.tensor(std, device=_dev()).view(-1, 1, 1)
    image = R.noise(11, 240, 320)
    small = R.resize_width(image, WIDTH)
    uploads, set_images = [], []
    upload = samfront.upload
    monkeypatch.setattr(samfront, "upload", lambda img, device: (uploads.append(tuple(img.shape)), upload(img, device))[1])
    g = _generator(sam, segmentor_width_size=WIDTH, hip_front=True, hip_resize=True)
    set_image = g.predictor.set_image
    monkeypatch.setattr(g.predictor, "set_image", lambda img, *a: (set_images.append(img), set_image(img, *a))[1])
    for n in (1, 2):
        out = g.generate_masks(image)
        assert uploads == [(240, 320, 3)] * n, uploads
    assert len(set_images) == 2 and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 for t in set_images)
    assert np.array_equal(set_images[0].cpu().numpy(), small)
    x = samfront.preprocess(torch.from_numpy(small).to(_dev()), mean, std, side=1024, layout="x")
    assert len(sam.image_encoder.inputs) == 2 and torch.equal(sam.image_encoder.inputs[0], x)
    ref = _generator(StubSam(_dev()), encode_image=encode_image).generate_masks(small)
    _check_against_small_run(out, ref, image, small)


def test_dropin_old_route_untouched():
    """hip_resize=False still goes through cv2 for a real resize (an ImportError where cv2 is not installed), and through the same-size
    shortcut without it."""
    from tests.sam_amg_stub import StubSam, encode_image
    g = _generator(StubSam(_dev()), encode_image=encode_image, segmentor_width_size=WIDTH, hip_resize=False)
    assert g.hip_resize is False
    image = R.noise(12, 240, 320)
    if importlib.util.find_spec("cv2") is None:
        with pytest.raises(ImportError, match="cv2"):
            g.generate_masks(image)
    else:
        assert tuple(g.generate_masks(image)["masks"].shape[1:]) == (240, 320)
    same = R.resize_width(image, WIDTH)
    on = _generator(StubSam(_dev()), encode_image=encode_image, segmentor_width_size=WIDTH, hip_resize=True).generate_masks(same)
    off = g.generate_masks(same)
    assert off["masks"].dtype == torch.float32 and torch.equal(on["masks"], off["masks"]) and torch.equal(on["boxes"], off["boxes"])
