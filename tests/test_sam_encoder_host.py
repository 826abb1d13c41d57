"""SAM's image encoder on the host: the float64 restatement (tests/sam_encoder_ref.py) against the fixture captured from the reference's
own ImageEncoderViT in .double() (tests/gen_sam_encoder_golden.py), sam6d_hip.samenc's eager partner and its library-shaped sequence
(index-based windows, pad_qkv rows, T_h / T_w indexing, gathered 3 x 3) against the restatement in float64, the configurations `check`
refuses, the drop-in's switch, and the kernels' resource budgets.  No GPU."""
import functools
import importlib
import sys

import numpy as np
import pytest
import torch

from tests import sam_encoder_ref as R
from tests._util import golden


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def _small():
    """The fixture's geometry, seeded weights and input, the reference's float64 output, and the restatement's (computed once)."""
    z = golden("sam_encoder_small")
    cfg = {k[4:]: (tuple(int(i) for i in z[k]) if z[k].ndim else int(z[k])) for k in z.files if k.startswith("cfg_")}
    sd = R.seeded_weights(int(z["seed"]), **cfg)
    x = R.seeded_input(int(z["input_seed"]), cfg["grid"] * cfg["patch"])
    out = R.forward(R.to_dtype(sd, torch.float64), x, cfg["heads"], R.windows_of(sd, cfg["window"]))
    return z, cfg, sd, x, out


def _weights(sd, dtype=torch.float64, **kw):
    from sam6d_hip import samenc
    return samenc.SamEncoderWeights(sd, "cpu", dtype=dtype, **kw)


# ---------------------------------------------------------------------------------------------- 1. the restatement
def test_restatement_reproduces_reference():
    z, cfg, sd, x, out = _small()
    # the seeded generators still make the tensors the fixture was captured with
    assert abs(sum(float(v.double().sum()) for v in sd.values()) - float(z["weight_sum"])) <= 1e-9 * abs(float(z["weight_sum"])) + 1e-9
    assert abs(float(x.double().sum()) - float(z["input_sum"])) <= 1e-9 * abs(float(z["input_sum"])) + 1e-9
    # the geometry has every case: padded windows (20 -> 28), a windowed and a global block, random rel-pos tables and pos_embed
    assert cfg == dict(dim=32, heads=2, depth=2, global_blocks=(1,), grid=20, window=14, patch=16, out=8)
    assert R.windows_of(sd, 14) == [14, 0]
    for k in ("blocks.0.attn.rel_pos_h", "blocks.1.attn.rel_pos_w", "pos_embed"):
        assert float(sd[k].abs().max()) > 0.1
    assert z["out"].dtype == np.float64
    e = rel(out, torch.from_numpy(z["out"]))
    print("\n[sam_encoder] restatement vs the reference's ImageEncoderViT in float64: %.3e" % e)
    assert tuple(out.shape) == (1, 8, 20, 20) and e <= 1e-12


def test_restatement_pad_rows_matter():
    """The padded positions are real keys: the same block with the padded rows' k and v changed gives another result in the windows
    that have padding, and the same in the one window that has none."""
    z, cfg, sd, x, out = _small()
    sd64 = R.to_dtype(sd, torch.float64)
    X = R.embed(sd64, x.double())
    p = "blocks.0."
    qkv = torch.nn.functional.linear(R.layer_norm(X, sd64[p + "norm1.weight"], sd64[p + "norm1.bias"], 1e-6), sd64[p + "attn.qkv.weight"],
                                     sd64[p + "attn.qkv.bias"])
    a = R.attention(qkv, sd64[p + "attn.qkv.bias"], sd64[p + "attn.rel_pos_h"], sd64[p + "attn.rel_pos_w"], 2, 14)
    b = R.attention(qkv, sd64[p + "attn.qkv.bias"] + 1.0, sd64[p + "attn.rel_pos_h"], sd64[p + "attn.rel_pos_w"], 2, 14)
    assert torch.equal(a[:, :14, :14], b[:, :14, :14])
    assert float((a[:, 14:, 14:] - b[:, 14:, 14:]).abs().max()) > 1e-3 and float((a[:, :14, 14:] - b[:, :14, 14:]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- 2. the package's torch partners
def test_eager_float64_matches_restatement():
    from sam6d_hip import samenc
    z, cfg, sd, x, out = _small()
    W = _weights(sd)
    assert W.geom.windows == (14, 0) and W.geom.num_heads == 2 and W.geom.grid == 20 and W.blocks is None
    got = samenc.eager(x, W)
    e = rel(got, out)
    print("\n[sam_encoder] eager float64 vs restatement: %.3e" % e)
    assert got.dtype == torch.float64 and got.shape == out.shape and e <= 1e-12


def test_library_shaped_sequence_float64_matches_restatement():
    """Windows by row number with the padding row, the bias read from T_h / T_w at q - k + S - 1, the 3 x 3 convolution as nine shifted
    rows and one product, LayerNorm2d as a row LayerNorm: the whole sequence, and the attention and the gather on their own.  Bound:
    float64 rounding through two blocks (about 1e-14)."""
    from sam6d_hip import samenc
    z, cfg, sd, x, out = _small()
    W = _weights(sd)
    e = rel(samenc.restructured(x, W), out)
    print("\n[sam_encoder] library-shaped sequence float64 vs restatement: %.3e" % e)
    assert e <= 2e-14
    # the two attention forms at the kernels' own geometry (64 x 64 grid, windows of 14, heads of 80), one image, two heads
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((4096, 480), generator=g, dtype=torch.float64)
    pad = torch.randn((480,), generator=g, dtype=torch.float64)
    for win, nrel in ((14, 27), (0, 127)):
        rh, rw = (0.1 * torch.randn((nrel, 80), generator=g, dtype=torch.float64) for _ in range(2))
        want = R.attention(qkv.view(1, 64, 64, 480), pad, rh, rw, 2, win).reshape(4096, 160)
        e = rel(samenc.rel_attention(qkv, pad, rh, rw, 1, 2, 64, win or 64), want)
        print("[sam_encoder] rel_attention (%s) float64 vs restatement: %.3e" % ("windows of 14" if win else "global", e))
        assert e <= 2e-14
    rows = samenc.window_rows(64, 14, "cpu")
    assert tuple(rows.shape) == (25, 196) and int((rows == 4096).sum()) == 70 * 70 - 4096
    assert int((rows[24] < 4096).sum()) == 64 and int((rows[4] < 4096).sum()) == 14 * 8 and rows[0, 15].item() == 64 + 1
    y = torch.randn((2 * 4096, 8), generator=g, dtype=torch.float64)
    w = torch.randn((5, 8, 3, 3), generator=g, dtype=torch.float64)
    conv = torch.nn.functional.conv2d(y.view(2, 64, 64, 8).permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, 5)
    e = rel(samenc.neck_gather(y, 2, 64) @ w.permute(0, 2, 3, 1).reshape(5, 72).t(), conv)
    print("[sam_encoder] gathered 3 x 3 vs conv2d: %.3e" % e)
    assert e <= 2e-14


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_check_refuses_by_name():
    from sam6d_hip import samenc
    full = R.seeded_weights(1, depth=2)
    g = samenc.check(full)  # SAM ViT-H at depth 2: accepted; depth and the global blocks are data
    assert g.windows == (14, 0) and g.depth == 2 and g.num_heads == 16
    assert samenc.check(R.seeded_weights(1, depth=3, global_blocks=(0, 2))).windows == (0, 14, 0)

    def edit(**changes):
        sd = dict(full)
        for k, v in changes.items():
            if v is None:
                del sd[k]
            else:
                sd[k] = v
        return sd
    cases = [
        (dict(image_encoder=R.seeded_weights(1, dim=768, heads=12, depth=1, global_blocks=())), "embed_dim = 768"),       # vit_b
        (dict(image_encoder=R.seeded_weights(1, dim=1280, heads=20, depth=1, global_blocks=())), "num_heads = 20"),       # head width 64
        (dict(image_encoder=R.seeded_weights(1, depth=1, global_blocks=(), mlp_ratio=2)), "mlp_dim = 2560"),
        (dict(image_encoder=R.seeded_weights(1, depth=1, global_blocks=(), out=128)), "out_chans = 128"),
        (dict(image_encoder=R.seeded_weights(1, depth=1, global_blocks=(), grid=32)), "img_size = 512"),
        (dict(image_encoder=R.seeded_weights(1, depth=1, global_blocks=(), patch=8)), "patch_size = 8"),
        (dict(image_encoder=full, eps=1e-5), "LayerNorm eps = 1e-05"),
        (dict(image_encoder=full, window_size=7), "window_size = 7"),
        # rel_pos of another length than 2 S - 1: get_rel_pos would interpolate
        (dict(image_encoder=edit(**{"blocks.0.attn.rel_pos_h": torch.zeros(13, 80)})), r"blocks.0.attn.rel_pos_h shape = \(13, 80\)"),
        (dict(image_encoder=edit(**{"blocks.1.attn.rel_pos_w": torch.zeros(27, 80)})), r"blocks.1.attn.rel_pos_w shape = \(27, 80\)"),
        (dict(image_encoder=full, global_attn_indexes=()), r"blocks.1.attn.rel_pos_h shape = \(127, 80\)"),
        (dict(image_encoder=edit(pos_embed=None)), "use_abs_pos = False"),
        (dict(image_encoder=edit(**{"blocks.0.attn.qkv.bias": None})), "qkv_bias = False"),
        (dict(image_encoder=edit(**{"blocks.0.attn.rel_pos_h": None})), "use_rel_pos = False"),
    ]
    for kw, text in cases:
        with pytest.raises(NotImplementedError, match=text):
            samenc.check(**kw)
    # the library entry points refuse a weight set that is not packed (CPU, or float64), and before that a wrong input
    z, cfg, sd, x, out = _small()
    with pytest.raises(RuntimeError):
        _weights(sd, torch.float32).require_library()
    with pytest.raises(ValueError, match="1024"):
        samenc.check_images(x)


# ---------------------------------------------------------------------------------------------- 4. the drop-in's switch
def test_dropin_switch(monkeypatch):
    from tests.sam_amg_stub import StubSam, encode_image
    from tests.sam_encoder_stub import SEEDS, StubSamWithEncoder
    import sam6d_hip
    mod = importlib.import_module("model.sam")
    monkeypatch.delenv("SAM6D_HIP_SAMENC", raising=False)
    monkeypatch.delenv("SAM6D_HIP_SAMDEC", raising=False)
    monkeypatch.delitem(sys.modules, "sam6d_hip.samenc", raising=False)
    if hasattr(sam6d_hip, "samenc"):
        monkeypatch.delattr(sam6d_hip, "samenc")
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    sam = StubSam("cpu")
    g = mod.CustomSamAutomaticMaskGenerator(sam, encode_image=encode_image)
    got = g.generate_masks(image)
    assert g.predictor.hip_encoder is False and g.predictor._encoder_model is sam
    assert "sam6d_hip.samenc" not in sys.modules  # switched off, the module is not even imported
    assert got["masks"].shape[0] >= 5 and sam.calls == 16
    monkeypatch.setenv("SAM6D_HIP_SAMENC", "0")
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image).predictor.hip_encoder is False
    assert mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_encoder=False).predictor.hip_encoder is False
    # switched on: an image encoder that is no module, another configuration, a CPU model -- refused, by keyword and by environment
    with pytest.raises(TypeError, match="state dict"):
        mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_encoder=True)
    monkeypatch.setenv("SAM6D_HIP_SAMENC", "1")
    with pytest.raises(TypeError, match="state dict"):
        mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image)
    monkeypatch.delenv("SAM6D_HIP_SAMENC")
    small = StubSamWithEncoder("cpu", *SEEDS, dim=32, heads=2, depth=1, global_blocks=())
    with pytest.raises(NotImplementedError, match="embed_dim = 32"):
        mod.CustomSamAutomaticMaskGenerator(small, hip_encoder=True)
    cpu = StubSamWithEncoder("cpu", *SEEDS, depth=1, global_blocks=())
    kind = type(cpu.image_encoder)
    with pytest.raises(RuntimeError, match="HIP device"):
        mod.CustomSamAutomaticMaskGenerator(cpu, hip_encoder=True)
    assert type(cpu.image_encoder) is kind  # the caller's object is as it was
    # the view: the library's encoder in the place of image_encoder, everything else the caller's
    view = mod._SamView(cpu, "encoder")
    assert view.image_encoder == "encoder" and view.mask_decoder is cpu.mask_decoder and view.device == cpu.device
    assert view.image_format == "RGB" and type(cpu.image_encoder) is kind


# ---------------------------------------------------------------------------------------------- 5. kernel resources
def test_kernel_resources():
    """DESIGN section 8 row f8 states the budgets: built values rounded up to the next allocation step of 8 registers -- the windowed
    kernel 124 -> 128 VGPRs (two waves per SIMD fit beside its 159 KB of LDS either way), the global kernel 162 -> 168 (three waves per
    SIMD), the gather 16; none may use scratch.  Read from the code object's metadata."""
    from tests._util import kernel_resources
    budget = {"sam_window_attention_kernel": 128, "sam_global_attention_kernel": 168, "sam_neck_gather_kernel": 16}
    found = kernel_resources(b"sam_window_attention_kernel", r"(sam_[a-z0-9_]+_kernel)")
    for name, cap in budget.items():
        assert name in found, "%s not found in the library" % name
        print("\n[sam_encoder] %s: %d VGPRs, %d B scratch, %d spilled" % ((name,) + found[name]))
        assert found[name][0] <= cap and found[name][1] == 0 and found[name][2] == 0, (name, found[name])
