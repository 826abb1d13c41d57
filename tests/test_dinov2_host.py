"""ISM's descriptor path on the host: the restatement (tests/dinov2_ref.py) against fixtures captured from the reference
(tests/gen_dinov2_golden.py), the drop-in CustomDINOv2's construction and state-dict layout, LayerScale folding, and the
configurations sam6d_hip.dinov2 refuses.  No GPU."""
import importlib

import pytest
import torch

from tests import dinov2_ref as R
from tests._util import golden


def _small():
    z = golden("dinov2_small")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return z, sd


# ---------------------------------------------------------------------------------------------- 1. forward restatement
def test_restatement_reproduces_reference_tokens():
    z, sd = _small()
    x = torch.stack([R.rgb_normalize(torch.from_numpy(im)) for im in z["images"]]).double()
    cls, tok = R.forward(R.to_dtype(sd, torch.float64), x, int(z["num_heads"]))
    ref_cls, ref_tok = torch.from_numpy(z["x_norm_clstoken"]), torch.from_numpy(z["x_norm_patchtokens"])
    assert cls.dtype == torch.float64 and tuple(tok.shape) == (2, 256, 64)
    for got, ref, name in ((cls, ref_cls, "cls"), (tok, ref_tok, "patch")):
        e = float((got - ref).abs().max() / ref.abs().max())
        print("\n[dinov2] restatement %s: max|diff| / max|ref| = %.3e" % (name, e))
        assert e <= 1e-12, (name, e)


def test_interpolated_position_embedding_bitwise():
    from sam6d_hip import dinov2
    z, sd = _small()
    ref = torch.from_numpy(z["pos_interpolated"])
    assert ref.dtype == torch.float32 and tuple(ref.shape) == (1, 257, 64)
    assert torch.equal(R.interpolate_pos(sd["pos_embed"], 16), ref)
    assert torch.equal(dinov2.interpolate_pos_embed(sd["pos_embed"]), ref)


# ---------------------------------------------------------------------------------------------- 2. CropResizePad
def _crop_fixture():
    z = golden("crop_resize_pad")
    H, W = int(z["height"]), int(z["width"])
    coord = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    return z, coord, torch.from_numpy(z["boxes"])


def test_crop_resize_pad_restatement_exact_on_every_box():
    z, coord, boxes = _crop_fixture()
    assert int((z["resized_long_side"] == 223).sum()) >= 3 and len(boxes) == len(z["notes"]) >= 12
    got = R.crop_resize_pad(coord.expand(len(boxes), -1, -1, -1), boxes)[:, 0]
    ref = torch.from_numpy(z["out"])
    for i in range(len(boxes)):  # every box, none left out
        assert torch.equal(got[i].to(torch.int32), ref[i]), (i, str(z["notes"][i]))


def test_dropin_crop_resize_pad_matches_fixture():
    bb = importlib.import_module("utils.bbox_utils")
    z, coord, boxes = _crop_fixture()
    got = bb.CropResizePad(224)(coord.expand(len(boxes), -1, -1, -1), boxes)[:, 0]
    assert torch.equal(got.to(torch.int32), torch.from_numpy(z["out"]))


def test_resized_sides_and_second_resize():
    """What the crop kernel's square branch relies on: with torch's scale factor (reciprocal, times 224, float32) the resized long
    side is 223 or 224 for every box side, and the second resize of a 223 square gives 224 pixels (torch's size rule in double)."""
    import math
    sides = torch.arange(1, 20001)
    factor = (224 / sides).double()
    assert torch.equal(factor, (sides.float().reciprocal() * 224.0).double())
    resized = torch.floor(sides.double() * factor).long()
    assert set(resized.tolist()) == {223, 224}
    assert math.floor(223 * (224.0 / 223)) == 224


def test_package_crop_resize_pad_matches_fixture_and_refuses():
    from sam6d_hip import dinov2
    z, coord, boxes = _crop_fixture()
    ref = torch.from_numpy(z["out"])
    shared = dinov2.crop_resize_pad(coord[0], boxes)[:, 0]
    assert torch.equal(shared.to(torch.int32), ref)
    masks = (torch.rand(len(boxes), *coord.shape[-2:], generator=torch.Generator().manual_seed(2)) > 0.5).float()
    got = dinov2.crop_resize_pad(coord[0], boxes, masks=masks)
    want = R.crop_resize_pad(coord * masks[:, None], boxes)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        dinov2.crop_resize_pad(coord[0], boxes.float())
    with pytest.raises(ValueError, match="empty"):
        dinov2.crop_resize_pad(coord[0], torch.tensor([[5, 5, 6, 400]]))


def test_attention_kernel_resources():
    """DESIGN section 8 row f5 states the attention kernel's budget: at most 128 VGPRs (two workgroups' worth of waves per SIMD would
    fit the register file; LDS allows one) and no scratch.  Read from the code object's metadata."""
    from tests._util import kernel_resources
    found = kernel_resources(b"dino_attention_kernel", r"(dino_attention_kernel)").get("dino_attention_kernel")
    assert found is not None, "dino_attention_kernel not found in the library"
    print("\n[dinov2] attention kernel: %d VGPRs, %d B scratch, %d spilled" % found)
    assert found[0] <= 128 and found[1] == 0 and found[2] == 0, found


# ---------------------------------------------------------------------------------------------- 3. the drop-in
@pytest.fixture(scope="module")
def dropin():
    mod = importlib.import_module("model.dinov2")
    return mod, mod.CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")


def test_dropin_constructs_without_absent_packages(dropin):
    import sys
    mod, m = dropin
    for name in ("openvino", "torchvision", "pytorch_lightning"):
        assert name not in sys.modules or getattr(sys.modules[name], "__file__", None) is None, name
    src = open(mod.__file__).read()
    for name in ("openvino", "torchvision", "pytorch_lightning"):
        assert ("import " + name) not in src, name
    assert type(m).__mro__[1] is torch.nn.Module
    for a in ("model_name", "model", "validpatch_thresh", "token_name", "chunk_size", "patch_size", "proposal_size",
              "descriptor_width_size", "rgb_proposal_processor", "patch_kernel"):
        assert hasattr(m, a), a
    for f in ("process_rgb_proposals", "process_masks_proposals", "compute_features", "forward_by_chunk", "forward_cls_token",
              "forward_patch_tokens", "forward_by_chunk_v2", "compute_masked_patch_feature", "compute_cls_and_patch_features", "forward"):
        assert callable(getattr(m, f)), f


def test_dropin_state_dict_is_the_reference_layout(dropin):
    z, _ = _small()
    want = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(z["vitl14_names"], z["vitl14_shapes"])}
    got = {k: tuple(v.shape) for k, v in dropin[1].model.state_dict().items()}
    assert got == want, (set(got) ^ set(want))


def test_dropin_small_model_matches_reference():
    """The eager module (fp32) with the fixture's weights: its own forward against the reference's float64 tokens."""
    mod = importlib.import_module("model.dinov2")
    z, sd = _small()
    m = mod.DinoVisionTransformer(embed_dim=64, depth=2, num_heads=1).eval()
    m.load_state_dict(sd, strict=True)
    x = torch.stack([R.rgb_normalize(torch.from_numpy(im)) for im in z["images"]])
    with torch.no_grad():
        f = m.double().forward_features(x.double())
    ref = torch.from_numpy(z["x_norm_patchtokens"])
    assert float((f["x_norm_patchtokens"] - ref).abs().max() / ref.abs().max()) <= 1e-12
    assert float((f["x_norm_clstoken"] - torch.from_numpy(z["x_norm_clstoken"])).abs().max()) <= 1e-11


def test_dropin_cpu_forward_small_scene(dropin):
    """process_* on the CPU: shapes, the in-place unsqueeze of the caller's masks, one proposal keeps its leading dimension."""
    mod, m = dropin
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (60, 80, 3), generator=g, dtype=torch.uint8).numpy()
    masks = torch.zeros(2, 60, 80)
    masks[0, 10:40, 20:50] = 1
    masks[1, 5:30, 40:70] = 1
    boxes = torch.tensor([[20, 10, 50, 40], [40, 5, 70, 30]])
    rgbs = m.process_rgb_proposals(img, masks, boxes)
    assert tuple(rgbs.shape) == (2, 3, 224, 224)
    assert torch.equal(rgbs, R.process_rgb_proposals(torch.from_numpy(img), masks, boxes))
    one = masks[:1].clone()
    pm = m.process_masks_proposals(one, boxes[:1])
    assert tuple(one.shape) == (1, 1, 60, 80) and tuple(pm.shape) == (1, 224, 224)
    assert torch.equal(pm, R.process_masks_proposals(masks[:1], boxes[:1]))


def test_layerscale_folding_float64():
    from sam6d_hip import dinov2
    z, sd = _small()
    sd = R.to_dtype(sd, torch.float64)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 33, 64, generator=g, dtype=torch.float64)
    ref = R.block(sd, 1, x, 1)
    folded = dict(sd)
    p = "blocks.1."
    folded[p + "attn.proj.weight"], folded[p + "attn.proj.bias"] = dinov2.fold_layerscale(
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"], sd[p + "ls1.gamma"])
    folded[p + "mlp.fc2.weight"], folded[p + "mlp.fc2.bias"] = dinov2.fold_layerscale(
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], sd[p + "ls2.gamma"])
    folded[p + "ls1.gamma"] = torch.ones(64, dtype=torch.float64)
    folded[p + "ls2.gamma"] = torch.ones(64, dtype=torch.float64)
    assert not torch.equal(folded[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.weight"])
    got = R.block(folded, 1, x, 1)
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------- 4. refused configurations
def _fake_sd(dim=1024, depth=24, patch=14, hid=None, n_pos=1369, **extra):
    """Shapes only (expanded zero-stride tensors: no memory)."""
    z = lambda *s: torch.zeros(1).expand(*s)  # noqa: E731
    hid = hid or 4 * dim
    sd = {"cls_token": z(1, 1, dim), "pos_embed": z(1, 1 + n_pos, dim), "mask_token": z(1, dim),
          "patch_embed.proj.weight": z(dim, 3, patch, patch), "patch_embed.proj.bias": z(dim), "norm.weight": z(dim), "norm.bias": z(dim)}
    for i in range(depth):
        b = "blocks.%d." % i
        sd.update({b + "norm1.weight": z(dim), b + "norm1.bias": z(dim), b + "attn.qkv.weight": z(3 * dim, dim),
                   b + "attn.qkv.bias": z(3 * dim), b + "attn.proj.weight": z(dim, dim), b + "attn.proj.bias": z(dim),
                   b + "ls1.gamma": z(dim), b + "norm2.weight": z(dim), b + "norm2.bias": z(dim), b + "mlp.fc1.weight": z(hid, dim),
                   b + "mlp.fc1.bias": z(hid), b + "mlp.fc2.weight": z(dim, hid), b + "mlp.fc2.bias": z(dim), b + "ls2.gamma": z(dim)})
    sd.update(extra)
    return sd


@pytest.mark.parametrize("kw,word", [
    (dict(depth=12), "12"), (dict(dim=768), "768"), (dict(patch=16), "16"), (dict(hid=2048), "2048"), (dict(n_pos=1370), "1370"),
    (dict(register_tokens=torch.zeros(1, 4, 1024)), "register"),
])
def test_unsupported_configurations_raise(kw, word):
    from sam6d_hip import dinov2
    with pytest.raises(NotImplementedError, match=word):
        dinov2.DinoWeights(_fake_sd(**kw), "cpu")


def test_unsupported_ffn_chunks_and_image_size_raise():
    from sam6d_hip import dinov2
    sd = _fake_sd()
    sd["blocks.0.mlp.w12.weight"] = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="swiglu"):
        dinov2.DinoWeights(sd, "cpu")
    sd = {("blocks.0." + k[7:] if k.startswith("blocks.") else k): v for k, v in _fake_sd(depth=1).items()}
    with pytest.raises(NotImplementedError, match="chunk"):
        dinov2.DinoWeights(sd, "cpu")
    sd = _fake_sd()
    del sd["blocks.0.ls1.gamma"]
    with pytest.raises(NotImplementedError, match="LayerScale"):
        dinov2.DinoWeights(sd, "cpu")
    with pytest.raises(NotImplementedError, match="518"):
        dinov2.check_images(torch.zeros(1, 3, 518, 518))
    dinov2.check_state_dict({k[len("model."):]: v for k, v in {"model." + k: v for k, v in _fake_sd().items()}.items()})
    dinov2.check_state_dict(dinov2._strip({"model." + k: v for k, v in _fake_sd().items()}))
