"""SAM's point-prompt path and mask decoder on the host: the float64 restatement (tests/sam_decoder_ref.py) against fixtures captured
from the reference (tests/gen_sam_decoder_golden.py), sam6d_hip.samdec's eager partner and its restructured sequence (per-image
tables, stacked projections, folded out_proj) against the restatement in float64, the configurations it refuses, the drop-in's
switch, and the kernels' resource budgets.  No GPU."""
import functools
import importlib
import math
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sam_decoder_ref as R
from tests._util import golden


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _small():
    z = golden("sam_decoder_small")
    psd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("psd.")}
    dsd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("dsd.")}
    return z, psd, dsd


@functools.lru_cache(maxsize=None)
def _full():
    """The full-width fixture, its seeded weights and the restatement's float64 outputs on its two points (computed once)."""
    z = golden("sam_decoder_full")
    psd, dsd = R.seeded_weights(int(z["seed"]))
    feats = R.seeded_features(int(z["feature_seed"]))
    pts = torch.from_numpy(z["points"])
    low, iou = R.forward(R.to_dtype(psd, torch.float64), R.to_dtype(dsd, torch.float64), pts, feats, 8, (1024, 1024), (64, 64))
    return z, psd, dsd, feats, pts, low, iou


def _weights(psd, dsd, heads, input_size, grid, dtype=torch.float64):
    from sam6d_hip import samdec
    return samdec.SamDecoderWeights(psd, dsd, "cpu", dtype=dtype, num_heads=heads, input_image_size=input_size, grid=grid)


def _small_weights(dtype=torch.float64):
    z, psd, dsd = _small()
    return z, _weights(psd, dsd, int(z["num_heads"]), tuple(z["input_size"]), tuple(z["grid"]), dtype)


# ---------------------------------------------------------------------------------------------- 1. the restatement
def test_restatement_reproduces_reference_small():
    z, psd, dsd = _small()
    heads, grid, input_size = int(z["num_heads"]), tuple(z["grid"]), tuple(z["input_size"])
    sparse, pe = torch.from_numpy(z["sparse"]), torch.from_numpy(z["dense_pe"])
    assert sparse.dtype == torch.float32 and pe.dtype == torch.float32 and z["low"].dtype == np.float64
    sd64 = R.to_dtype(dsd, torch.float64)
    dense = R.dense_embeddings(R.to_dtype(psd, torch.float64), sparse.shape[0], grid)
    low, iou = R.decoder(sd64, torch.from_numpy(z["features"]).double(), pe.double(), sparse.double(), dense, heads)
    e_low, e_iou = rel(low, torch.from_numpy(z["low"])), rel(iou, torch.from_numpy(z["iou"]))
    print("\n[sam_decoder] restatement, small: low %.3e, iou %.3e" % (e_low, e_iou))
    assert tuple(low.shape) == (3, 3, 32, 32) and e_low <= 1e-10 and e_iou <= 1e-10
    # the prompt path in float64 (rounded to float32 where the reference rounds) against the reference's float32 values
    p64 = R.to_dtype(psd, torch.float64)
    e_sp = rel(R.embed_points(p64, torch.from_numpy(z["points"]), input_size), sparse.double())
    e_pe = rel(R.dense_pe(p64, grid), pe.double())
    print("[sam_decoder] prompt embeddings %.3e, dense PE %.3e" % (e_sp, e_pe))
    assert e_sp <= 1e-6 and e_pe <= 1e-6


def test_restatement_reproduces_reference_full():
    z, psd, dsd, feats, pts, low, iou = _full()
    px = torch.from_numpy(z["pixels"])
    e_low, e_iou = rel(low.flatten(2)[:, :, px], torch.from_numpy(z["low_at_pixels"])), rel(iou, torch.from_numpy(z["iou"]))
    print("\n[sam_decoder] restatement, full width: low %.3e (max |ref| %.3f), iou %.3e" % (e_low, float(np.abs(z["low_at_pixels"]).max()), e_iou))
    # the whole forward here starts from float64 prompt embeddings, the fixture from the reference's float32 ones: the prompt path's
    # own 1e-6 goes through the decoder, so the decoder is pinned at 1e-10 on the fixture's embeddings ...
    sd64 = R.to_dtype(dsd, torch.float64)
    p64 = R.to_dtype(psd, torch.float64)
    low2, iou2 = R.decoder(sd64, feats.double(), R.dense_pe(psd, (64, 64)).double(), torch.from_numpy(z["sparse"]).double(),
                           R.dense_embeddings(p64, 2, (64, 64)), 8)
    d_low, d_iou = rel(low2.flatten(2)[:, :, px], torch.from_numpy(z["low_at_pixels"])), rel(iou2, torch.from_numpy(z["iou"]))
    print("[sam_decoder] decoder on the fixture's embeddings: low %.3e, iou %.3e" % (d_low, d_iou))
    assert d_low <= 1e-10 and d_iou <= 1e-10
    # ... and the prompt path at 1e-6 against the reference's float32 values
    e_sp = rel(R.embed_points(p64, pts, (1024, 1024)), torch.from_numpy(z["sparse"]).double())
    tok = torch.from_numpy(z["pe_tokens"])
    e_pe = rel(R.dense_pe(p64, (64, 64)).flatten(2)[0][:, tok], torch.from_numpy(z["dense_pe_at_pixels"]).double())
    print("[sam_decoder] prompt embeddings %.3e, dense PE %.3e" % (e_sp, e_pe))
    assert e_sp <= 1e-6 and e_pe <= 1e-6
    assert e_low <= 1e-4 and e_iou <= 1e-4  # end to end: the float32 rounding of the reference's embeddings, amplified by the decoder


# ---------------------------------------------------------------------------------------------- 2. the package's eager partner
def test_eager_float64_matches_restatement():
    from sam6d_hip import samdec
    z, W = _small_weights()
    _, psd, dsd = _small()
    pts, feats = torch.from_numpy(z["points"]), torch.from_numpy(z["features"])
    ref = R.forward(R.to_dtype(psd, torch.float64), R.to_dtype(dsd, torch.float64), pts, feats, W.heads, W.input_size, W.grid)
    got = samdec.eager(pts, feats, W)
    zf, psd, dsd, feats_f, pts_f, low_f, iou_f = _full()
    got_f = samdec.eager(pts_f, feats_f, _weights(psd, dsd, 8, (1024, 1024), (64, 64)))
    for name, g, r in (("small low", got[0], ref[0]), ("small iou", got[1], ref[1]), ("full low", got_f[0], low_f), ("full iou", got_f[1], iou_f)):
        e = rel(g, r)
        print("\n[sam_decoder] eager float64 vs restatement, %s: %.3e" % (name, e))
        assert g.dtype == torch.float64 and e <= 1e-10, (name, e)


def test_restructured_sequence_float64_matches_eager():
    """Tables of layer 0, stacked image-side projections with the positional part as a table, folded out_proj, the 7-token attention as
    vector ops, ConvTranspose as GEMM operands and the pixel order of the mask product: the whole restructured sequence in float64
    against the reference's sequence.  Bound: float64 rounding (1e-16) times what the two-layer decoder amplifies, as for the
    restatement itself."""
    from sam6d_hip import samdec
    z, W = _small_weights()
    pts, feats = torch.from_numpy(z["points"]), torch.from_numpy(z["features"])
    zf, psd, dsd, feats_f, pts_f, low_f, iou_f = _full()
    Wf = _weights(psd, dsd, 8, (1024, 1024), (64, 64))
    for name, got, ref in (("small", samdec.restructured(pts, feats, W), samdec.eager(pts, feats, W)),
                           ("full", samdec.restructured(pts_f, feats_f, Wf), (low_f, iou_f))):
        e_low, e_iou = rel(got[0], ref[0]), rel(got[1], ref[1])
        print("\n[sam_decoder] restructured float64 vs eager, %s: low %.3e, iou %.3e" % (name, e_low, e_iou))
        assert got[0].shape == ref[0].shape and e_low <= 1e-10 and e_iou <= 1e-10


def test_layer0_hoist_equals_per_prompt_projections():
    """Layer 0's k_proj(src + pe), v_proj(src) of the token->image attention and q_proj(src + pe) of the image->token attention as one
    table over the image rows, against the projections of the P-fold repeated tensors."""
    from sam6d_hip import samdec
    z, W = _small_weights()
    zf, psd, dsd, feats_f, *_ = _full()
    for W, feats in ((W, torch.from_numpy(z["features"])), (_weights(psd, dsd, 8, (1024, 1024), (64, 64)), feats_f)):
        P, md, ci = 3, W.md, W.dim // 2
        tables = samdec._tables(samdec.TorchOps(W), feats, W)
        src = torch.repeat_interleave(feats.double(), P, dim=0) + W.pe["no_mask_embed.weight"].reshape(1, -1, 1, 1)
        src = src.flatten(2).permute(0, 2, 1)
        pos = torch.repeat_interleave(W.dense_pe[None], P, dim=0)
        p = "transformer.layers.0."
        want = torch.cat([F.linear(src + pos, md[p + "cross_attn_token_to_image.k_proj.weight"], md[p + "cross_attn_token_to_image.k_proj.bias"]),
                          F.linear(src, md[p + "cross_attn_token_to_image.v_proj.weight"], md[p + "cross_attn_token_to_image.v_proj.bias"]),
                          F.linear(src + pos, md[p + "cross_attn_image_to_token.q_proj.weight"], md[p + "cross_attn_image_to_token.q_proj.bias"])],
                         dim=2)
        assert tuple(tables.g0.shape) == (1, W.N, 3 * ci) and tuple(tables.src.shape) == (1, W.N, W.dim)
        e = rel(tables.g0.expand(P, -1, -1), want)
        print("\n[sam_decoder] layer-0 tables vs per-prompt projections (dim %d): %.3e" % (W.dim, e))
        assert e <= 1e-12
        assert torch.equal(tables.src.expand(P, -1, -1), src)


def test_out_proj_fold_equals_unfolded_attention():
    """The image->token attention with out_proj folded into the 7 x 8 value rows against Attention.forward followed by out_proj."""
    from sam6d_hip import samdec
    z, Ws = _small_weights()
    zf, psd, dsd, *_ = _full()
    g = torch.Generator().manual_seed(5)
    for W in (Ws, _weights(psd, dsd, 8, (1024, 1024), (64, 64))):
        P, ci, C, H, N = 3, W.dim // 2, W.dim, W.heads, W.N
        d = ci // H
        ops, p = samdec.TorchOps(W), "transformer.layers.1."
        G = torch.randn((P, N, 3 * ci), generator=g, dtype=torch.float64)
        ktok = torch.randn((P, 7, ci), generator=g, dtype=torch.float64)
        vtok = torch.randn((P, 7, ci), generator=g, dtype=torch.float64)
        keys = torch.randn((P, N, C), generator=g, dtype=torch.float64)
        got = ops.i2t(G, 2 * ci, ktok, ops.fold(vtok, p + "cross_attn_image_to_token.out_proj"), p, keys)

        def sep(x):
            return x.reshape(P, -1, H, d).transpose(1, 2)
        attn = torch.softmax(sep(G[:, :, 2 * ci:]) @ sep(ktok).permute(0, 1, 3, 2) / math.sqrt(d), dim=-1)
        out = (attn @ sep(vtok)).transpose(1, 2).reshape(P, N, ci)
        out = F.linear(out, W.md[p + "cross_attn_image_to_token.out_proj.weight"], W.md[p + "cross_attn_image_to_token.out_proj.bias"])
        want = F.layer_norm(keys + out, (C,), W.md[p + "norm4.weight"], W.md[p + "norm4.bias"], 1e-5)
        e = rel(got, want)
        print("\n[sam_decoder] folded out_proj vs unfolded (dim %d): %.3e" % (C, e))
        assert e <= 1e-12


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_check_state_dicts_refusals():
    from sam6d_hip import samdec
    psd, dsd = R.seeded_weights(1)
    samdec.check_state_dicts(psd, dsd, 8)  # the one configuration: accepted
    small = R.seeded_weights(1, dim=32, mlp_dim=64)
    ps3, ds3 = R.seeded_weights(1, depth=3)
    ps1, ds1 = R.seeded_weights(1, mlp_dim=1024)
    cases = [
        (dict(prompt_sd=small[0], decoder_sd=small[1], num_heads=8), "transformer_dim = 32"),
        (dict(prompt_sd=psd, decoder_sd=dsd, num_heads=4), "num_heads = 4"),
        (dict(prompt_sd=ps3, decoder_sd=ds3, num_heads=8), "depth = 3"),
        (dict(prompt_sd=ps1, decoder_sd=ds1, num_heads=8), "mlp_dim = 1024"),
        (dict(prompt_sd=psd, decoder_sd=dsd, num_heads=8, grid=(32, 32)), "image_embedding_size = (32, 32)"),
        (dict(prompt_sd=psd, decoder_sd=dsd, num_heads=8, boxes=torch.zeros(1, 4)), "box prompts"),
        (dict(prompt_sd=psd, decoder_sd=dsd, num_heads=8, masks=torch.zeros(1, 1, 256, 256)), "mask prompts"),
        (dict(prompt_sd=psd, decoder_sd=dsd, num_heads=8, multimask_output=False), "multimask_output = False"),
    ]
    for kw, text in cases:
        with pytest.raises(NotImplementedError, match=text.replace("(", r"\(").replace(")", r"\)")):
            samdec.check_state_dicts(**kw)
    # the library entry points refuse a weight set the kernels are not built for, and a CPU one
    _, Wsmall = _small_weights(torch.float32)
    with pytest.raises((NotImplementedError, RuntimeError)):
        Wsmall.require_library()


# ---------------------------------------------------------------------------------------------- 4. the drop-in's switch
def test_dropin_switch_off_is_todays_path(monkeypatch):
    from tests.sam_amg_stub import StubSam, encode_image
    import sam6d_hip
    mod = importlib.import_module("model.sam")
    monkeypatch.delenv("SAM6D_HIP_SAMDEC", raising=False)
    monkeypatch.delitem(sys.modules, "sam6d_hip.samdec", raising=False)
    if hasattr(sam6d_hip, "samdec"):
        monkeypatch.delattr(sam6d_hip, "samdec")
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    g = mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image)
    got = g.generate_masks(image)
    assert g.predictor.hip_decoder is False and g.predictor.tables is None
    assert "sam6d_hip.samdec" not in sys.modules and not hasattr(sam6d_hip, "samdec")
    assert g.predictor.model.calls == 16
    off = mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_decoder=False).generate_masks(image)
    monkeypatch.setenv("SAM6D_HIP_SAMDEC", "0")
    env0 = mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image).generate_masks(image)
    assert got["masks"].shape[0] >= 5
    for other in (off, env0):
        assert torch.equal(other["boxes"], got["boxes"]) and torch.equal(other["masks"], got["masks"])
    # switched on, a network without the reference's modules is refused (here: the stub's plain functions), by keyword and by environment
    with pytest.raises(TypeError, match="state dicts"):
        mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image, hip_decoder=True)
    monkeypatch.setenv("SAM6D_HIP_SAMDEC", "1")
    with pytest.raises(TypeError, match="state dicts"):
        mod.CustomSamAutomaticMaskGenerator(StubSam("cpu"), encode_image=encode_image)


def test_dropin_switch_on_refuses_other_configurations_and_cpu():
    from tests.sam_decoder_stub import StubSamNetwork
    mod = importlib.import_module("model.sam")
    with pytest.raises(RuntimeError, match="HIP device"):
        mod.CustomSamAutomaticMaskGenerator(StubSamNetwork("cpu", seed=3), hip_decoder=True)
    with pytest.raises(NotImplementedError, match="transformer_dim = 32"):
        mod.CustomSamAutomaticMaskGenerator(StubSamNetwork("cpu", seed=3, dim=32, mlp_dim=64), hip_decoder=True)


# ---------------------------------------------------------------------------------------------- 5. kernel resources
def test_kernel_resources():
    """DESIGN section 8 row f7 states the budgets: the image->token kernel keeps a 56-float table column per thread (<= 160 VGPRs), the
    token->image kernel <= 96, the upscaling kernel keeps a sub-pixel's 64 channels per thread (<= 200: two waves per SIMD); none
    may use scratch.  Read from the code object's metadata."""
    from tests._util import kernel_resources
    budget = {"samdec_i2t_kernel": 160, "samdec_t2i_kernel": 96, "samdec_upscale_kernel": 200}
    found = kernel_resources(b"samdec_i2t_kernel", r"(samdec_[a-z0-9_]+_kernel)")
    for name, cap in budget.items():
        assert name in found, "%s not found in the library" % name
        print("\n[sam_decoder] %s: %d VGPRs, %d B scratch, %d spilled" % ((name,) + found[name]))
        assert found[name][0] <= cap and found[name][1] == 0 and found[name][2] == 0, (name, found[name])
