"""SAM's image front on the GPU: sam_front_kernel (sam6d_hip.samfront.preprocess) against the numpy restatement of the reference
(tests/pil_bilinear.py, held to Pillow itself by tests/test_sam_front_host.py), in both output layouts; samenc.encode_rows against
samenc.encode; and the drop-in with hip_front switched on against an `encode_image` hook built from the restatement.  Every comparison
is bitwise: the path is integer arithmetic followed by one fp32 subtraction and one correctly rounded fp32 division."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import gen_sam_front_golden as G
from tests import pil_bilinear as P
from tests._util import golden

pytestmark = pytest.mark.gpu
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
LARGE = G.LARGE + ((2047, 1025), (37, 53))  # side 1024: enlarging, 4 taps, portrait with 3 taps, 4 taps on odd sizes, strong enlarging
GUARD = 64                                  # floats on either side of an output buffer


def _dev():
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _large(h, w, reverse=False):
    """(image, restatement (3, 1024, 1024)) of a seeded h x w noise image, computed once."""
    img = G.noise(1000 + h + w, h, w)
    return img, P.preprocessed(img, MEAN, STD, 1024, reverse)


def _both_layouts(name, img_dev, want, side, reverse=False):
    """The kernel in both layouts on a device image (one image) against the restatement's (3, side, side)."""
    from sam6d_hip import samfront
    x = samfront.preprocess(img_dev, MEAN, STD, side=side, layout="x", reverse=reverse)
    rows = samfront.preprocess(img_dev, MEAN, STD, side=side, layout="rows", reverse=reverse)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (1, 3, side, side) and x.dtype == torch.float32 and tuple(rows.shape) == ((side // 16) ** 2, 768), name
    dx = int((bits(x[0].cpu().numpy()) != bits(want)).sum())
    dr = int((bits(rows.cpu().numpy()) != bits(P.patch_rows(want))).sum())
    print("\n[sam_front] %s, side %d%s: %d (x) and %d (rows) values differ from the restatement" % (name, side, ", reversed" if reverse else "", dx, dr))
    assert dx == 0 and dr == 0, name
    return x, rows


# ---------------------------------------------------------------------------------------------- 1. the kernel against the restatement
def test_fixture_geometries():
    """Every geometry of the fixture the package admits, at its small side: enlarging, shrinking with 4 .. 9 taps, a skipped pass,
    1 x 1, one row, one column, an output height that is no multiple of 16, all-0 and all-255."""
    z = golden("sam_front")
    n = 0
    for name in G.SMALL:
        if name == "tall":
            continue
        img, side = z["in_" + name], int(z["side_" + name])
        _both_layouts(name, torch.from_numpy(img).to(_dev()), P.preprocessed(img, MEAN, STD, side), side)
        n += 1
    assert n >= 15


@pytest.mark.parametrize("hw", LARGE, ids=lambda hw: "%dx%d" % hw)
def test_side_1024(hw):
    img, want = _large(*hw)
    _both_layouts("%d x %d" % hw, torch.from_numpy(img).to(_dev()), want, 1024)


def test_reverse_batch_and_strides():
    from sam6d_hip import samfront
    dev = _dev()
    img, want = _large(1080, 1920, True)
    _both_layouts("1080 x 1920", torch.from_numpy(img).to(dev), want, 1024, reverse=True)
    z = golden("sam_front")
    small = z["in_shrink_1p9"]
    _both_layouts("shrink_1p9", torch.from_numpy(small).to(dev), P.preprocessed(small, MEAN, STD, 160, True), 160, reverse=True)
    # B = 2 with an image stride, and a row stride larger than 3 W: crops of one larger image, read in place
    big = torch.from_numpy(G.noise(77, 2 * 300 + 7, 500)).to(dev)
    crops = big.view(-1)[:2 * 300 * 1500].view(2, 300, 500, 3)[:, 20:281, 30:431]  # (2, 261, 401, 3): strides (450000, 1500, 3, 1)
    assert not crops.is_contiguous() and crops.stride() == (450000, 1500, 3, 1)
    for layout in ("x", "rows"):
        got = samfront.preprocess(crops, MEAN, STD, side=304, layout=layout)
        torch.cuda.synchronize()
        for b in range(2):
            want = P.preprocessed(crops[b].cpu().numpy(), MEAN, STD, 304)
            if layout == "x":
                assert np.array_equal(bits(got[b].cpu().numpy()), bits(want)), (layout, b)
            else:
                assert np.array_equal(bits(got[b * 361:(b + 1) * 361].cpu().numpy()), bits(P.patch_rows(want))), (layout, b)
    one = samfront.preprocess(crops[1], MEAN, STD, side=304)  # a single crop view: the row stride alone
    assert torch.equal(one[0], samfront.preprocess(crops, MEAN, STD, side=304)[1])
    # the package's eager partner on the device gives the same bits
    assert torch.equal(samfront.eager(crops, MEAN, STD, side=304, layout="rows"), samfront.preprocess(crops, MEAN, STD, side=304, layout="rows"))


def _raw_call(image, size, out_ptr, lay=0, **change):
    """sam6d_sam_front through the binding with the package's own tables; `change` replaces arguments of the C entry by name."""
    from sam6d_hip import _lib, amg, samfront
    H, W = int(image.shape[0]), int(image.shape[1])
    oh, ow = amg.preprocess_shape(H, W, size)
    (xt, xtaps), (yt, ytaps) = samfront._device_table(W, max(ow, 1), image.device), samfront._device_table(H, max(oh, 1), image.device)
    a = dict(img=image.data_ptr(), row_stride=image.stride(0), image_stride=0, B=1, H=H, W=W, reverse=0, xtab=xt.data_ptr(), xtaps=xtaps,
             ytab=yt.data_ptr(), ytaps=ytaps, m0=MEAN[0], m1=MEAN[1], m2=MEAN[2], s0=STD[0], s1=STD[1], s2=STD[2], side=size, out=out_ptr,
             layout=lay, stream=torch.cuda.current_stream().cuda_stream)
    assert not set(change) - set(a)
    a.update(change)
    _lib.call("sam6d_sam_front", *a.values())


def test_guards_and_refusals():
    """The launch writes its output and nothing around it; a refused call returns non-zero (the binding raises) and launches nothing."""
    dev = _dev()
    z = golden("sam_front")
    img_np = z["in_enlarge_landscape"]
    img, side = torch.from_numpy(img_np).to(dev), 64
    want = P.preprocessed(img_np, MEAN, STD, side)
    for layout, ref in ((0, want), (1, P.patch_rows(want))):
        buf = torch.full((ref.size + 2 * GUARD,), -7.5, device=dev)
        _raw_call(img, side, buf.data_ptr() + 4 * GUARD, layout)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == -7.5).all() and (got[-GUARD:] == -7.5).all()
        assert np.array_equal(bits(got[GUARD:-GUARD]), bits(ref).reshape(-1))
    buf = torch.full((3 * side * side + 2 * GUARD,), -7.5, device=dev)
    out = buf.data_ptr() + 4 * GUARD
    wide = torch.zeros((1, 300, 3), dtype=torch.uint8, device=dev)
    cases = [(dict(img=None), "null"), (dict(xtab=None), "null"), (dict(ytab=None), "null"), (dict(out=None), "null"),
             (dict(H=0), "H and W"), (dict(W=4097), "H and W"), (dict(H=-3), "H and W"), (dict(side=24), "side"), (dict(side=1040), "side"),
             (dict(side=0), "side"), (dict(xtaps=10), "taps"), (dict(ytaps=0), "taps"), (dict(layout=2), "layout"),
             (dict(row_stride=3 * 47 - 1), "row_stride"), (dict(image_stride=-1), "image_stride"), (dict(out=out + 4), "aligned"),
             (dict(B=-1), "B"), (dict(B=70000), "B")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=text):
            _raw_call(img, side, out, **change)
    with pytest.raises(RuntimeError, match="resizes to"):  # 1 x 300 at side 64: no output row
        _raw_call(wide, side, out)
    torch.cuda.synchronize()
    assert bool((buf == -7.5).all()), "a refused call wrote to the output"


def test_rows_layout_equals_patch_rows_of_x():
    """The rows layout is what sam6d_sam_patch_rows writes from the x layout."""
    from sam6d_hip import _lib, samfront
    img, want = _large(480, 640)
    d = torch.from_numpy(img).to(_dev())
    x = samfront.preprocess(d, MEAN, STD, layout="x")
    rows = samfront.preprocess(d, MEAN, STD, layout="rows")
    A = torch.empty((4096, 768), device=_dev())
    _lib.call("sam6d_sam_patch_rows", x.data_ptr(), A.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(A, rows)


# ---------------------------------------------------------------------------------------------- 2. the encoder from patch rows, the drop-in
class _StubSam:
    """tests/sam_encoder_stub.StubSamWithEncoder (a seeded depth-2 encoder at ViT-H width in front of the decoder stub) with Sam's
    pixel_mean / pixel_std buffers, built once."""

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def get():
        from tests.sam_encoder_stub import PIXEL_MEAN, PIXEL_STD, SEEDS, StubSamWithEncoder

        class WithStats(StubSamWithEncoder):
            def __init__(self, device, *seeds):
                super().__init__(device, *seeds)
                self.pixel_mean = torch.tensor(PIXEL_MEAN, device=self._dev).view(-1, 1, 1)
                self.pixel_std = torch.tensor(PIXEL_STD, device=self._dev).view(-1, 1, 1)
        return WithStats(_dev(), *SEEDS)


def test_encode_rows_equals_encode():
    from sam6d_hip import samenc, samfront
    sam = _StubSam.get()
    W = samenc.SamEncoderWeights(sam.image_encoder, _dev())
    assert W.geom.windows == (14, 0)
    imgs = torch.from_numpy(np.stack([sam.test_image(7), sam.test_image(8)])).to(_dev())
    x = samfront.preprocess(imgs, MEAN, STD, layout="x")
    rows = samfront.preprocess(imgs, MEAN, STD, layout="rows")
    a, b = samenc.encode(x, W), samenc.encode_rows(rows, W)
    torch.cuda.synchronize()
    assert tuple(b.shape) == (2, 256, 64, 64) and torch.isfinite(b).all() and torch.equal(a, b)
    assert torch.equal(samenc.encode_rows(rows[4096:], W)[0], a[1])
    with pytest.raises(ValueError, match="patch rows"):
        samenc.encode_rows(rows[:100], W)


def _restatement_hook(sam, image):
    """An `encode_image` for the drop-in: the restatement's resize on the host, then sam.preprocess and sam.image_encoder."""
    oh, ow = P.preprocess_shape(image.shape[0], image.shape[1], sam.image_encoder.img_size)
    x = torch.as_tensor(P.resize(image, oh, ow), device=sam.device).permute(2, 0, 1).contiguous()[None]
    return sam.image_encoder(sam.preprocess(x)), (oh, ow)


@pytest.mark.parametrize("hip_encoder", [False, True], ids=["eager encoder", "library encoder"])
def test_dropin(hip_encoder):
    """64 points on the 480 x 640 test image: with hip_front on, the features are those of a hook built from the restatement and
    sam.preprocess, and masks and boxes are identical; the same with the library's encoder behind it (the rows layout into
    encode_rows)."""
    from sam6d_hip import amg
    mod = importlib.import_module("model.sam")
    sam = _StubSam.get()
    image = sam.test_image()
    res = {}
    for name, kw in (("front", dict(hip_front=True)), ("hook", dict(encode_image=_restatement_hook))):
        g = mod.CustomSamAutomaticMaskGenerator(sam, points_per_batch=32, pred_iou_thresh=-1e9, stability_score_thresh=0.0, hip_encoder=hip_encoder, **kw)
        g.points_per_side = 8
        g.point_grids = amg.layer_point_grids(8, 0, 1)
        assert g.predictor.hip_front is (name == "front") and g.predictor.hip_encoder is hip_encoder
        sam.image_encoder.calls = 0
        g.predictor.set_image(image)
        feats, size = g.predictor.features.clone(), g.predictor.input_size
        out = g.generate_masks(image)
        assert sam.image_encoder.calls == (0 if hip_encoder else 2)  # the library's encoder never calls the module
        res[name] = (feats, size, out)
    (f1, s1, o1), (f2, s2, o2) = res["front"], res["hook"]
    assert s1 == s2 == (768, 1024) and tuple(f1.shape) == (1, 256, 64, 64)
    assert torch.equal(f1, f2), "features differ: max |diff| %.3e" % float((f1 - f2).abs().max())
    assert o1["masks"].shape[0] >= 1 and torch.equal(o1["masks"], o2["masks"]) and torch.equal(o1["boxes"], o2["boxes"])
    # a BGR image through the front's `reverse` = the flipped image through it
    front = mod.Predictor(sam, hip_encoder=hip_encoder, hip_front=True)
    front.set_image(np.ascontiguousarray(image[..., ::-1]), "BGR")
    assert torch.equal(front.features, f1)
