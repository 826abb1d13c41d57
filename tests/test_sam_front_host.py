"""SAM's image front on the host: the numpy restatement (tests/pil_bilinear.py) against Pillow -- the fixture made with it
(tests/gen_sam_front_golden.py) and the library itself wherever PIL imports --, sam6d_hip.samfront's tables and its eager partner
against the restatement, the drop-in's switch with its refusals, and the kernel's resource budget.  Every comparison is bitwise: the
path is integer arithmetic followed by one fp32 subtraction and one fp32 division.  No GPU."""
import hashlib
import importlib
import sys

import numpy as np
import pytest
import torch

from tests import gen_sam_front_golden as G
from tests import pil_bilinear as P
from tests._util import golden

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)  # Sam's pixel_mean / pixel_std (build_sam.py)
VGPRS_BUILT = 132   # sam_front_kernel as built
VGPR_BUDGET = 136   # ... rounded up to a multiple of 8
# (in, out) pairs: enlarging, shrinking with 4 .. 9 taps, identity, one source pixel, the largest admitted axis
AXES = ((640, 1024), (480, 768), (1920, 1024), (1080, 576), (700, 478), (1500, 1024), (1025, 513), (2047, 1024), (37, 715), (53, 1024),
        (256, 64), (260, 64), (230, 64), (317, 96), (1024, 1024), (3, 3), (1, 64), (50, 64), (13, 3), (4096, 1024))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def small_cases():
    """[(name, image, side, Pillow's resized image)] of the fixture."""
    z = golden("sam_front")
    return [(name, z["in_" + name], int(z["side_" + name]), z["out_" + name]) for name in G.SMALL]


# ---------------------------------------------------------------------------------------------- 1. the restatement against Pillow
def test_restatement_equals_fixture():
    z = golden("sam_front")
    assert str(z["pillow_version"]) == "12.2.0"
    for i, (name, img, side, want) in enumerate(small_cases()):
        assert np.array_equal(img, G.small_input(i, name)), name  # the seeded generator still makes the fixture's input
        oh, ow = P.preprocess_shape(img.shape[0], img.shape[1], side)
        assert want.shape == (oh, ow, 3) and want.dtype == np.uint8, name
        got = P.resize(img, oh, ow)
        assert np.array_equal(got, want), "%s: %d bytes differ from Pillow's" % (name, int((got != want).sum()))
    # the cases the fixture is there for
    shapes = {name: (img.shape[:2], want.shape[:2]) for name, img, side, want in small_cases()}
    assert shapes["enlarge_landscape"][1][0] % 16 and shapes["one_pixel"] == ((1, 1), (64, 64))
    assert shapes["width_unchanged"][0][1] == shapes["width_unchanged"][1][1] and shapes["width_unchanged"][0][0] != shapes["width_unchanged"][1][0]
    assert shapes["one_row"][0][0] == 1 and shapes["one_column"][0][1] == 1
    taps = {name: max(len(k) for _, k in P.coefficients(s[0][1], s[1][1])) for name, s in shapes.items()}
    assert (taps["enlarge_landscape"], taps["shrink_1p9"], taps["shrink_3p3"], taps["shrink_3p6"], taps["shrink_4"]) == (2, 4, 7, 8, 9)
    assert P.vertical_first(*shapes["tall"][0], shapes["tall"][1][0]) and not P.vertical_first(480, 640, 768)
    for h, w in G.LARGE:
        img = G.noise(int(z["seed_%dx%d" % (h, w)]), h, w)
        got = P.resize(img, *P.preprocess_shape(h, w, 1024))
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(z["sha_%dx%d" % (h, w)]), (h, w)


def test_restatement_equals_pillow():
    """The library itself, where it is installed: geometries the fixture does not hold."""
    Image = pytest.importorskip("PIL.Image")
    for n, (h, w, side) in enumerate(((37, 53, 1024), (640, 480, 1024), (1025, 2047, 512), (3, 1024, 1024), (300, 1200, 304), (77, 131, 48))):
        img = G.noise(900 + n, h, w)
        oh, ow = P.preprocess_shape(h, w, side)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(P.resize(img, oh, ow), want), (h, w, side)


# ---------------------------------------------------------------------------------------------- 2. the package's host side
def test_tables_equal_the_restatements_coefficients():
    from sam6d_hip import samfront
    for n_in, n_out in AXES:
        lo, count, k = samfront.tables(n_in, n_out)
        ref = P.coefficients(n_in, n_out)
        assert lo.dtype == count.dtype == k.dtype == np.int32 and k.shape == (n_out, max(len(c) for _, c in ref))
        for i, (rlo, rk) in enumerate(ref):
            assert int(lo[i]) == rlo and int(count[i]) == len(rk) and k[i, :len(rk)].tolist() == rk and not k[i, len(rk):].any(), (n_in, n_out, i)
        assert int((lo + count).max()) <= n_in and int(lo.min()) >= 0 and int(k.min()) >= 0
    assert samfront.tables(4096, 1024)[2].shape[1] <= samfront.MAX_TAPS  # what 4096 pixels at side 1024 need fits the kernel
    with pytest.raises(ValueError):
        samfront.tables(0, 4)


@pytest.mark.parametrize("reverse", [False, True])
def test_eager_cpu_equals_restatement(reverse):
    """samfront.eager on the CPU = restatement + (x - mean) / std + pad, in both layouts, for every fixture geometry the package admits,
    one large one and a batch."""
    from sam6d_hip import samfront
    cases = [(name, img, side) for name, img, side, _ in small_cases() if name != "tall"] + [("1080x1920", G.noise(5, 1080, 1920), 1024)]
    for name, img, side in cases:
        want = P.preprocessed(img, MEAN, STD, side, reverse)
        x = samfront.eager(torch.from_numpy(img), MEAN, STD, side=side, layout="x", reverse=reverse)
        assert tuple(x.shape) == (1, 3, side, side) and x.dtype == torch.float32 and x.is_contiguous(), name
        assert np.array_equal(bits(x[0].numpy()), bits(want)), name
        rows = samfront.eager(torch.from_numpy(img), torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1), side=side, layout="rows",
                              reverse=reverse)
        assert np.array_equal(bits(rows.numpy()), bits(P.patch_rows(want))), name
        oh, ow = P.preprocess_shape(img.shape[0], img.shape[1], side)
        assert not want[:, oh:].any() and not want[:, :, ow:].any()  # zeros, not normalised zeros
    two = torch.from_numpy(np.stack([G.noise(6, 33, 47), G.noise(7, 33, 47)]))
    x = samfront.eager(two, MEAN, STD, side=64)
    for b in range(2):
        assert np.array_equal(bits(x[b].numpy()), bits(P.preprocessed(two[b].numpy(), MEAN, STD, 64)))


def test_refusals():
    from sam6d_hip import samfront
    img = torch.zeros((20, 30, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):  # CPU tensors, like everywhere else
        samfront.preprocess(img, MEAN, STD, side=64)
    for bad, text in ((img.float(), "uint8"), (img[..., :2], "uint8 tensor"), (torch.zeros((1, 4097, 3), dtype=torch.uint8), "4096")):
        with pytest.raises(ValueError, match=text):
            samfront.eager(bad, MEAN, STD, side=64)
    for side in (0, 24, 1040):
        with pytest.raises(ValueError, match="side"):
            samfront.eager(img, MEAN, STD, side=side)
    with pytest.raises(ValueError, match="layout"):
        samfront.eager(img, MEAN, STD, side=64, layout="nchw")
    with pytest.raises(ValueError, match="3 values"):
        samfront.eager(img, (1.0, 2.0), STD, side=64)
    with pytest.raises(ValueError, match="resizes to 0"):
        samfront.eager(torch.zeros((1, 300, 3), dtype=torch.uint8), MEAN, STD, side=64)
    with pytest.raises(NotImplementedError, match="taps"):  # shrinking by 8
        samfront.eager(torch.zeros((512, 512, 3), dtype=torch.uint8), MEAN, STD, side=64)
    with pytest.raises(NotImplementedError, match="vertical pass first"):
        samfront.eager(torch.zeros((1100, 10, 3), dtype=torch.uint8), MEAN, STD, side=64)
    with pytest.raises(AttributeError, match="pixel_mean"):
        samfront.pixel_stats(object())


# ---------------------------------------------------------------------------------------------- 3. the drop-in's switch
class _SamWithStats:
    """tests/sam_amg_stub.StubSam with Sam's pixel_mean / pixel_std buffers."""

    def __new__(cls, device, **without):
        from tests.sam_amg_stub import StubSam
        sam = StubSam(device)
        if "pixel_mean" not in without:
            sam.pixel_mean = torch.tensor(MEAN).view(-1, 1, 1)
        if "pixel_std" not in without:
            sam.pixel_std = torch.tensor(STD).view(-1, 1, 1)
        return sam


def test_dropin_switch(monkeypatch):
    from tests.sam_amg_stub import StubSam, encode_image
    import sam6d_hip
    mod = importlib.import_module("model.sam")
    for var in ("SAM6D_HIP_SAMFRONT", "SAM6D_HIP_SAMENC", "SAM6D_HIP_SAMDEC"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.delitem(sys.modules, "sam6d_hip.samfront", raising=False)
    if hasattr(sam6d_hip, "samfront"):
        monkeypatch.delattr(sam6d_hip, "samfront")
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    # switched off (the default, by keyword and by environment): nothing changes, the module is not even imported
    sam = StubSam("cpu")
    g = mod.CustomSamAutomaticMaskGenerator(sam, encode_image=encode_image)
    got = g.generate_masks(image)
    assert g.predictor.hip_front is False and got["masks"].shape[0] >= 5 and sam.calls == 16
    assert "sam6d_hip.samfront" not in sys.modules
    monkeypatch.setenv("SAM6D_HIP_SAMFRONT", "0")
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image).predictor.hip_front is False
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_front=False).predictor.hip_front is False
    monkeypatch.delenv("SAM6D_HIP_SAMFRONT")
    # switched on, each refusal by name and never a fall-back: a hook passed as well, the buffers missing, a CPU model
    with pytest.raises(ValueError, match="encode_image"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu"), encode_image=encode_image, hip_front=True)
    with pytest.raises(AttributeError, match="pixel_mean"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu", pixel_mean=None), hip_front=True)
    with pytest.raises(AttributeError, match="pixel_std"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu", pixel_std=None), hip_front=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu"), hip_front=True)
    monkeypatch.setenv("SAM6D_HIP_SAMFRONT", "1")
    with pytest.raises(RuntimeError, match="HIP device"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu"))
    with pytest.raises(ValueError, match="encode_image"):
        mod.CustomSamAutomaticMaskGenerator(_SamWithStats("cpu"), encode_image=encode_image)
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_front=False).predictor.hip_front is False


def test_encoder_embed_split_keeps_the_launches(monkeypatch):
    """Encoder.embed = the patch-rows launch + embed_rows (the patch GEMM alone): the ViT-B, DINOv2 and SAM descriptions launch what they
    launched, in the same order with the same arguments; embed_rows alone leaves the patch-rows launch out."""
    from sam6d_hip import encoder, samenc
    calls = []
    monkeypatch.setattr(encoder._lib, "call", lambda name, *a: calls.append((name,) + a))
    monkeypatch.setattr(encoder, "gemm", lambda *a, **kw: calls.append(("gemm", a[4:], sorted(kw))))
    monkeypatch.setattr(encoder, "_p", lambda t, off=0: (id(t), off))
    monkeypatch.setattr(encoder, "_s", lambda: 0)

    class W:
        cls = pos = object()
        patch = type("L", (), {"w": object(), "b": object(), "w16": staticmethod(lambda: None)})()
    images = torch.zeros((2, 3, 4, 4))
    samenc.ENC.embed(images, W, "X", "A")
    assert [c[0] for c in calls] == ["sam6d_sam_patch_rows", "gemm"] and calls[0][-2] == 2
    whole = list(calls)
    del calls[:]
    samenc.ENC.embed_rows("A", W, "X", 2)
    assert calls == whole[1:]
    del calls[:]
    from sam6d_hip import vit
    vit.ENC.embed(images, W, "X", "A")
    assert [c[0] for c in calls] == [vit.ENC.patch_rows, "gemm"] and len(calls[0]) == 8  # (with the cls token and pos_embed operands)


# ---------------------------------------------------------------------------------------------- 4. kernel resources
def test_kernel_resources():
    """DESIGN section 8 row f9 states the budget: sam_front_kernel builds at VGPRS_BUILT registers, held to the next allocation step of 8,
    and may not use scratch.  Read from the code object's metadata."""
    from tests._util import kernel_resources
    budget = {"sam_front_kernel": VGPR_BUDGET}
    found = kernel_resources(b"sam_front_kernel", r"(sam_front_kernel)")
    for name, cap in budget.items():
        assert name in found, "%s not found in the library's code objects" % name
        vgprs, scratch, spills = found[name]
        print("\n[sam_front] %s: %d VGPRs, %d bytes of scratch, %d spills" % (name, vgprs, scratch, spills))
        assert vgprs <= cap and scratch == 0 and spills == 0, (name, found[name])
