"""Host side of the library's ViT image features (no GPU): the hip_vit switch, the refusals of unsupported configurations and inputs,
and a numpy model of csrc/vit.hip's chosen-pixel gather (tap and column mapping) against F.interpolate + get_chosen_pixel_feats."""
import importlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam6d_hip import pem, synth, vit


def test_options_hip_vit(monkeypatch):
    assert pem.Options().hip_vit is False
    assert pem.Options(hip_vit=True).hip_vit is True
    assert pem.Options(hip_vit=True).replace(matmul_mode=0).hip_vit is True
    assert pem.Options.ENV["hip_vit"] == "SAM6D_HIP_VIT"
    monkeypatch.delenv("SAM6D_HIP_VIT", raising=False)
    assert pem.Options.from_env().hip_vit is False
    monkeypatch.setenv("SAM6D_HIP_VIT", "1")
    assert pem.Options.from_env().hip_vit is True and pem.Options.from_env().describe()["hip_vit"] is True
    monkeypatch.setenv("SAM6D_HIP_VIT", "0")
    assert pem.Options.from_env().hip_vit is False
    assert pem.Options.from_env(hip_vit=True).hip_vit is True


def _cfg(**over):
    c = dict(synth.default_model_cfg().feature_extraction)
    c.update(over)
    return types.SimpleNamespace(**c)


def test_refuses_other_configurations():
    vit.check_config(_cfg())
    with pytest.raises(NotImplementedError):
        vit.check_config(_cfg(vit_type="vit_large"))
    with pytest.raises(NotImplementedError):
        vit.check_config(_cfg(up_type="deconv"))
    with pytest.raises(NotImplementedError):
        vit.check_config(_cfg(use_pyramid_feat=False))
    with pytest.raises(NotImplementedError):
        vit.VitWeights({}, "cpu", cfg=_cfg(vit_type="vit_large"))


def test_refuses_other_weight_shapes():
    fe = importlib.import_module("feature_extraction")
    sd = fe.ViT_AE(_cfg(vit_type="vit_large", embed_dim=1024)).state_dict()  # 24 blocks of 1024 channels
    with pytest.raises(NotImplementedError):
        vit.VitWeights(sd, "cpu")
    sd = fe.ViT_AE(_cfg(use_pyramid_feat=False)).state_dict()
    with pytest.raises(NotImplementedError):
        vit.VitWeights(sd, "cpu")
    sd = {k: v for k, v in fe.ViT_AE(_cfg()).state_dict().items() if not k.startswith("output_upscaling")}
    with pytest.raises(NotImplementedError):  # what an up_type 'deconv' checkpoint lacks
        vit.VitWeights(sd, "cpu")


def test_refuses_other_inputs():
    ch = torch.zeros(2, 10, dtype=torch.long)
    vit.check_inputs(torch.zeros(2, 3, 224, 224), ch)
    for bad in (torch.zeros(2, 3, 256, 256), torch.zeros(2, 3, 224, 200), torch.zeros(2, 1, 224, 224), torch.zeros(3, 224, 224)):
        with pytest.raises(ValueError):
            vit.check_inputs(bad, ch)
    with pytest.raises(ValueError):
        vit.check_inputs(torch.zeros(2, 3, 224, 224, dtype=torch.float64), ch)
    with pytest.raises(ValueError):
        vit.check_inputs(torch.zeros(2, 3, 224, 224), torch.zeros(3, 10, dtype=torch.long))
    with pytest.raises(ValueError):
        vit.check_inputs(torch.zeros(2, 3, 224, 224), torch.zeros(2, 10))


def _np_gather(U, choose):
    """The index arithmetic of vit_upsample_gather_kernel, restated in numpy (float64 weights)."""
    B, N = choose.shape
    out = np.empty((B, N, 256))

    def src(d):
        s = max(0.25 * (d + 0.5) - 0.5, 0.0)
        i0 = int(s)
        i1 = i0 + (1 if i0 < 55 else 0)
        l1 = s - i0
        return i0, i1, 1.0 - l1, l1

    def cell(b, gy, gx):
        tok = 14 * (gy >> 2) + (gx >> 2)
        col = ((gy & 3) * 4 + (gx & 3)) * 256
        return U[b * 196 + tok, col:col + 256]

    for b in range(B):
        for n in range(N):
            y, x = divmod(int(choose[b, n]), 224)
            y0, y1, ly0, ly1 = src(y)
            x0, x1, lx0, lx1 = src(x)
            out[b, n] = ly0 * (lx0 * cell(b, y0, x0) + lx1 * cell(b, y0, x1)) + ly1 * (lx0 * cell(b, y1, x0) + lx1 * cell(b, y1, x1))
    return out


def test_gather_index_model_matches_interpolate():
    mu = importlib.import_module("model_utils")
    g = np.random.default_rng(3)
    B = 2
    U = g.standard_normal((B * 196, 4096))
    border = [y * 224 + x for y in (0, 1, 2, 111, 221, 222, 223) for x in (0, 1, 2, 111, 221, 222, 223)]
    choose = np.stack([np.concatenate([border, g.integers(0, 224 * 224, 150)]) for _ in range(B)])
    Ut = torch.from_numpy(U)
    m = Ut.reshape(B, 14, 14, 4, 4, 256).permute(0, 5, 1, 3, 2, 4).reshape(B, 256, 56, 56)
    m = F.interpolate(m, (224, 224), mode="bilinear", align_corners=False)
    ref = mu.get_chosen_pixel_feats(m, torch.from_numpy(choose)).numpy()
    got = _np_gather(U, choose)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(U).max()
