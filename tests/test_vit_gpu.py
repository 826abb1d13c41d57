"""The ViT-B image features on the library (sam6d_hip.vit, csrc/vit.hip, the ViT layout of xattn.hip's self-attention, gemm.hip act 2)
against float64 restatements: the whole encoder + chosen-pixel gather, each piece alone, range safety, the GELU epilogue on every GEMM
route, the fused gather's index arithmetic, peak memory, and the drop-in ViTEncoder / Net with Options.hip_vit on."""
import copy
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from sam6d_hip import _lib, pem, synth, vit

pytestmark = pytest.mark.gpu

BOUND = {1: 5e-5, 0: 1e-5}  # max |HIP - float64| / max |float64| on dense_fm, per matmul mode


def _cfg():
    return synth.default_model_cfg().feature_extraction


def _randomize(m, seed):
    """Random weights: nonzero cls_token / pos_embed / biases, fan-in scaled Linear and conv weights, LayerNorms off identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("weight") and p.dim() >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(fan_in))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return m


def _vit_ae(seed=0):
    fe = importlib.import_module("feature_extraction")
    return _randomize(fe.ViT_AE(_cfg()), seed).eval()


def _inputs(B, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randn(B, 3, 224, 224, generator=g)
    choose = torch.randint(0, 224 * 224, (B, N), generator=g)
    return rgb, choose


def _ref64(m, rgb, choose):
    mu = importlib.import_module("model_utils")
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        return mu.get_chosen_pixel_feats(m64(rgb.double())[0], choose)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


@pytest.fixture(scope="module")
def model():
    return _vit_ae(1)


@pytest.fixture(scope="module")
def case(model, dev):
    rgb, choose = _inputs(2, 2048, 2, dev)
    return rgb, choose, _ref64(model, rgb, choose)


def _weights(model, dev, mode):
    return vit.VitWeights(model.state_dict(), dev, options=pem.Options(matmul_mode=mode), cfg=_cfg())


# ------------------------------------------------------------------------------------------------ 1. whole encoder
@pytest.mark.parametrize("mode", [1, 0])
def test_encoder_vs_float64(model, case, dev, mode):
    rgb, choose, ref = case
    W = _weights(model, dev, mode)
    got = vit.image_features(rgb.to(dev), choose.to(dev), W)
    torch.cuda.synchronize()
    mu = importlib.import_module("model_utils")
    m32 = copy.deepcopy(model).to(dev)
    with torch.no_grad():
        eager = mu.get_chosen_pixel_feats(m32(rgb.to(dev))[0], choose.to(dev))
    e_hip, e_eager = _rel(got, ref), _rel(eager, ref)
    print("\n[vit] mode %d: max|HIP - f64| / max|f64| = %.3e, eager fp32: %.3e" % (mode, e_hip, e_eager))
    assert got.shape == (2, 2048, 256) and torch.isfinite(got).all()
    assert e_hip <= BOUND[mode], (e_hip, BOUND[mode])


# ------------------------------------------------------------------------------------------------ 2. pieces
def test_patch_embedding(model, dev):
    rgb, _ = _inputs(3, 1, 5, dev)
    W = _weights(model, dev, 1)
    got = vit.embed(rgb.to(dev), W)
    v = copy.deepcopy(model.vit).double()
    with torch.no_grad():
        x = v.patch_embed(rgb.double())
        ref = torch.cat([v.cls_token.expand(3, -1, -1), x], dim=1) + v.pos_embed
    assert _rel(got, ref) <= 1e-5


@pytest.mark.parametrize("mode", [1, 0])
def test_one_block(model, dev, mode):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 197, 768, generator=g)
    W = _weights(model, dev, mode)
    got = vit.block(x.to(dev), W, 4)
    with torch.no_grad():
        ref = copy.deepcopy(model.vit.blocks[4]).double()(x.double())
    assert _rel(got, ref) <= BOUND[mode]


# (B, n): the encoder's 197 tokens; one token; one full 16-token group; a group plus one token; every key tile full and both groups of
# every wave in use
@pytest.mark.parametrize("B,n", [(1, 197), (3, 197), (2, 1), (2, 16), (2, 17), (1, 208)])
def test_attention_alone(dev, B, n):
    g = torch.Generator().manual_seed(11 + B + (n if n != 197 else 0))
    qkv = torch.randn(B * n, 2304, generator=g) * 3.0
    got = vit.attention(qkv.to(dev), B)
    q, k, v = qkv.double().reshape(B, n, 3, 12, 64).permute(2, 0, 3, 1, 4)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * n, 768)
    q32, k32, v32 = (t.float().to(dev) for t in (q, k, v))
    eager = F.scaled_dot_product_attention(q32, k32, v32).transpose(1, 2).reshape(B * n, 768)
    e, e_eager = _rel(got, ref), _rel(eager, ref)
    print("\n[vit] attention B=%d n=%d: max|HIP - f64| / max|f64| = %.3e, eager fp32 SDPA: %.3e" % (B, n, e, e_eager))
    assert got.shape == (B * n, 768)
    assert e <= 1e-5  # logits up to ~70 at n = 197 (fewer keys: smaller): fp32's own rounding of them is ~4e-6 relative in the probabilities


def test_attention_outliers(dev):
    """q near fp16's subnormals, k and v beyond fp16's range (same logits as moderate q, k): finite and as accurate as usual."""
    g = torch.Generator().manual_seed(17)
    B = 2
    qkv = torch.randn(B * 197, 2304, generator=g) * 3.0
    qkv[:, :768] /= 2e4
    qkv[:, 768:] *= 2e4
    qkv[5, 1536 + 7] = 3e9  # one huge value of v
    got = vit.attention(qkv.to(dev), B)
    q, k, v = qkv.double().reshape(B, 197, 3, 12, 64).permute(2, 0, 3, 1, 4)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * 197, 768)
    assert torch.isfinite(got).all()
    err = (got.double().cpu() - ref).abs()
    heads = ref.reshape(B * 197, 12, 64).abs().amax(dim=(0, 2))  # per head: one huge v sets that head's scale
    e = float((err.reshape(B * 197, 12, 64).amax(dim=(0, 2)) / heads).max())
    print("\n[vit] attention outliers: max per-head |HIP - f64| / max|f64| = %.3e" % e)
    assert e <= 1e-5


def test_pyramid_taps(model, dev):
    rgb, _ = _inputs(2, 1, 9, dev)
    W = _weights(model, dev, 1)
    _, cat = vit.encode(rgb.to(dev), W)
    with torch.no_grad():
        outs = copy.deepcopy(model.vit).double()(rgb.double())
    ref = torch.cat([o[:, 1:] for o in outs], dim=2)
    assert cat.shape == (2, 196, 3072)
    for j in range(4):
        assert _rel(cat[..., 768 * j:768 * (j + 1)], ref[..., 768 * j:768 * (j + 1)]) <= BOUND[1], j


# ------------------------------------------------------------------------------------------------ 3. range safety
def test_range_outliers(dev):
    m = _vit_ae(3)
    b = m.vit.blocks[6]
    with torch.no_grad():
        b.mlp.fc2.weight.mul_(1e3)  # a residual stream of ~1e3 .. 1e4 after block 6
        b.mlp.fc1.weight.mul_(2e4)  # fc2's A operand beyond fp16 (> 2^15): the GEMM's exact-tile fallback
        # v beyond fp16 (the attention's power-of-two operand scales) and proj shrunk by as much: the same block output in exact
        # arithmetic (well conditioned), while the attention output beyond fp16 sends the proj GEMM to the exact-tile fallback too.
        # (q and k keep their size: the pre-split qkv weight has ONE power-of-two scale, rows 1e8 apart would leave q in fp16's
        # subnormals -- test_attention_outliers covers q and k at the extremes)
        for t in (b.attn.qkv.weight, b.attn.qkv.bias):
            t[1536:].mul_(2e4)
        b.attn.proj.weight.div_(2e4)
    rgb, choose = _inputs(2, 1024, 4, dev)
    rgb[:, :, 50:53, 100:103] = 1e4  # a few 1e4-magnitude input channels
    # the outliers do reach both places (float64)
    v = copy.deepcopy(m.vit).double()
    with torch.no_grad():
        x = v.patch_embed(rgb.double())
        x = torch.cat([v.cls_token.expand(2, -1, -1), x], dim=1) + v.pos_embed
        for blk in v.blocks[:6]:
            x = blk(x)
        blk_in = v.blocks[6].norm1(x)
        qkv = v.blocks[6].attn.qkv(blk_in)
        qkv_max = float(qkv[..., 1536:].abs().max())  # of v
        x = x + v.blocks[6].attn(blk_in)
        h_max = float(F.gelu(v.blocks[6].mlp.fc1(v.blocks[6].norm2(x))).abs().max())
    assert qkv_max > 65504.0 and h_max > 32768.0, (qkv_max, h_max)
    ref = _ref64(m, rgb, choose)
    W = vit.VitWeights(m.state_dict(), dev, options=pem.Options(matmul_mode=1), cfg=_cfg())
    got = vit.image_features(rgb.to(dev), choose.to(dev), W)
    assert torch.isfinite(got).all()
    e = _rel(got, ref)
    print("\n[vit] outliers: max|HIP - f64| / max|f64| = %.3e" % e)
    assert e <= BOUND[1]


# ------------------------------------------------------------------------------------------------ 4. GELU epilogue
def _gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("M,N,K", [(394, 3072, 768), (6304, 3072, 768), (77, 3072, 768), (256, 256, 64), (512, 512, 768)])
def test_gelu_epilogue_every_route(dev, mode, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    Wt = torch.randn(N, K, generator=g) / math.sqrt(K) * 2.0
    b = torch.randn(N, generator=g)
    ref = _gelu64(A.double() @ Wt.double().t() + b.double())
    Ad, Wd, bd = A.to(dev), Wt.to(dev), b.to(dev)
    hi, lo, sc = pem.split_w16(Wd)
    routes = set()
    for w16 in (False, True):
        C = torch.full((M, N), float("nan"), device=dev)
        _lib.call("sam6d_set_thread_matmul_mode", mode)
        try:
            wh, wl = (hi.data_ptr(), lo.data_ptr()) if w16 else (None, None)
            rc = _lib.load().sam6d_gemm_route(Ad.data_ptr(), Wd.data_ptr(), wh, wl, float(sc if w16 else 0.0), bd.data_ptr(), None, None,
                                               C.data_ptr(), M, N, K, K, K, N, 0, 1, 0, 0, 0, 0, 1.0, 2, 1, 0, 0, 0)
            assert rc >= 0
            routes.add(rc)
            if w16:
                _lib.call("sam6d_gemm_nt_w16", Ad.data_ptr(), Wd.data_ptr(), hi.data_ptr(), lo.data_ptr(), float(sc), bd.data_ptr(), None,
                          None, C.data_ptr(), M, N, K, K, K, N, 0, 1, 0, 0, 0, 0, 1.0, 2, pem._s())
            else:
                _lib.call("sam6d_gemm_nt", Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), None, None, C.data_ptr(), M, N, K, K, K, N, 0, 1,
                          0, 0, 0, 0, 1.0, 2, pem._s())
        finally:
            _lib.call("sam6d_set_thread_matmul_mode", -1)
        e = float((C.double().cpu() - ref).abs().max()) / float(ref.abs().max())
        assert e <= (2e-5 if mode == 1 else 2e-6), (w16, rc, e)
    print("\n[vit] gelu M=%d N=%d K=%d mode %d routes %s" % (M, N, K, mode, sorted(routes)))


@pytest.mark.parametrize("mode", [1, 0])
def test_gemm_in_place_residual(dev, mode):
    """C == residual (the encoder's proj / fc2 GEMMs): the same bits as a separate output buffer on each route."""
    for M, K in ((394, 768), (6304, 3072), (256, 768)):
        g = torch.Generator().manual_seed(M + K)
        A = torch.randn(M, K, generator=g).to(dev)
        lin = pem.Linear(torch.randn(768, K, generator=g).to(dev) / math.sqrt(K), torch.randn(768, generator=g).to(dev))
        X = torch.randn(M, 768, generator=g).to(dev)
        opts = pem.Options(matmul_mode=mode)

        @pem.on_tensor_device
        def run(A, X, out, options=None):
            pem.gemm(A, lin.w, lin.b, out, M, 768, K, K, K, 768, residual=X, ldr=768, w16=lin.w16())
            return out
        sep = run(A, X, torch.empty_like(X), options=opts)
        Xc = X.clone()
        run(A, Xc, Xc, options=opts)
        assert torch.equal(Xc, sep), (M, K)


# ------------------------------------------------------------------------------------------------ 5. fused gather
def _gather_ref(U, choose):
    B = choose.shape[0]
    m = U.reshape(B, 14, 14, 4, 4, 256).permute(0, 5, 1, 3, 2, 4).reshape(B, 256, 56, 56)
    m = F.interpolate(m, (224, 224), mode="bilinear", align_corners=False)
    mu = importlib.import_module("model_utils")
    return mu.get_chosen_pixel_feats(m, choose)


def test_fused_gather(dev):
    g = torch.Generator().manual_seed(21)
    B, N = 3, 5000
    U = (torch.randn(B * 196, 4096, generator=g) * 4.0).to(dev)
    border = [(y, x) for y in (0, 1, 222, 223) for x in (0, 1, 2, 100, 221, 222, 223)]
    choose = torch.randint(0, 224 * 224, (B, N), generator=g)
    for i, (y, x) in enumerate(border):
        choose[:, i] = y * 224 + x
        choose[:, len(border) + i] = x * 224 + y
    choose[:, 200:260] = choose[:, 5:6]  # repeated indices
    choose = choose.to(dev)
    got = vit.upsample_gather(U, choose)
    ref = _gather_ref(U, choose)
    assert float((got - ref).abs().max()) <= 1e-6 * float(U.abs().max())


def test_fused_gather_out_of_range_gives_nan(dev):
    g = torch.Generator().manual_seed(22)
    U = torch.randn(2 * 196, 4096, generator=g).to(dev)
    choose = torch.randint(0, 224 * 224, (2, 40), generator=g)
    choose[0, 3], choose[1, 7], choose[1, 8] = -1, 224 * 224, 10 ** 9
    got = vit.upsample_gather(U, choose.to(dev)).cpu()
    bad = torch.zeros(2, 40, dtype=torch.bool)
    bad[0, 3] = bad[1, 7] = bad[1, 8] = True
    assert torch.isnan(got[bad]).all() and torch.isfinite(got[~bad]).all()


# ------------------------------------------------------------------------------------------------ 6. memory
def test_peak_memory_below_dense_map(model, dev):
    W = _weights(model, dev, 1)
    rgb, choose = _inputs(32, 2048, 31, dev)
    rgb, choose = rgb.to(dev), choose.to(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = vit.image_features(rgb, choose, W)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense_map = 32 * 256 * 224 * 224 * 4
    print("\n[vit] B=32 peak allocation %.1f MB (dense map %.1f MB)" % (peak / 1e6, dense_map / 1e6))
    assert out.shape == (32, 2048, 256) and peak < dense_map


# ------------------------------------------------------------------------------------------------ 7. drop-in
@pytest.fixture(scope="module")
def net(dev):
    m = importlib.import_module("pose_estimation_model").Net(synth.default_model_cfg())
    m.load_state_dict(synth.make_pem_weights(1), strict=False)
    _randomize(m.feature_extraction.rgb_net, 5)
    return m.to(dev).eval()


def _fm_rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


def test_dropin_vit_encoder_and_net(net, dev, monkeypatch):
    inp = synth.kat_inputs(B=2, seed=3)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    rgb, choose = _inputs(2, d["dense_pm"].shape[1], 6, dev)
    rgb, choose = rgb.to(dev), choose.to(dev)
    fe = net.feature_extraction
    with torch.no_grad():
        off = fe(d["dense_pm"], rgb, choose, d["dense_po"], d["dense_fo"])
        monkeypatch.setenv("SAM6D_HIP_VIT", "1")
        on = fe(d["dense_pm"], rgb, choose, d["dense_po"], d["dense_fo"])
    for i in (0, 2, 3, 4):  # dense_pm, dense_po, dense_fo, radius
        assert torch.equal(on[i], off[i]), i
    e = _fm_rel(on[1], off[1])
    print("\n[vit] drop-in dense_fm: max|HIP - eager| / max|eager| = %.3e" % e)
    assert e <= BOUND[1]
    net.coarse_point_matching.hypothesis_rand = d["rand"]
    try:
        with torch.no_grad():
            fwd = net(d["dense_pm"], rgb, choose, d["model"], d["dense_po"], d["dense_fo"])
            dpm, dfm, dpo, dfo, rad = fe(d["dense_pm"], rgb, choose, d["dense_po"], d["dense_fo"])
            mt = net.match(dpm, dfm, dpo, dfo, rad, d["model"])
    finally:
        net.coarse_point_matching.hypothesis_rand = None
    for a, b in zip(fwd, mt):
        assert torch.equal(a, b)


def test_dropin_templates_batched(net, dev, monkeypatch):
    T, N = 42, 5000
    g = torch.Generator().manual_seed(8)
    rgbs = [torch.randn(1, 3, 224, 224, generator=g).to(dev) for _ in range(T)]
    pts = [(torch.rand(1, N, 3, generator=g) - 0.5).to(dev) for _ in range(T)]
    chs = [torch.randint(0, 224 * 224, (1, N), generator=g).to(dev) for _ in range(T)]
    fe = net.feature_extraction
    with torch.no_grad():
        p_off, f_off = fe.get_obj_feats(rgbs, pts, chs)[:2]
        monkeypatch.setenv("SAM6D_HIP_VIT", "1")
        p_on, f_on = fe.get_obj_feats(rgbs, pts, chs)[:2]
    assert torch.equal(p_on, p_off)
    e = _fm_rel(f_on, f_off)
    print("\n[vit] templates T=42: max|HIP - eager| / max|eager| = %.3e" % e)
    assert e <= BOUND[1]


def test_dropin_device_pipeline(net, dev, monkeypatch):
    from tests.test_rgb_inputs_gpu import _detections, _device_templates, _device_test_data, _templates
    imgs, masks, xyz = _templates(13, T=6)
    img, depth, dmasks, scores, model = _detections(17)
    monkeypatch.setenv("SAM6D_HIP_VIT", "1")
    tem = _device_templates(dev, imgs, masks, xyz, 3)
    d, _ = _device_test_data(dev, img, depth, dmasks[:4], scores, model, 4)
    B = d["pts"].shape[0]
    with torch.no_grad():
        po, fo = net.feature_extraction.get_obj_feats(*tem)[:2]
        R, t, s = net(d["pts"], d["rgb"], d["rgb_choose"], d["model"], po.repeat(B, 1, 1), fo.repeat(B, 1, 1))
    assert R.shape == (B, 3, 3) and torch.isfinite(R).all() and torch.isfinite(t).all() and torch.isfinite(s).all()


def test_mode2_refused(model, dev):
    W = _weights(model, dev, 2)
    rgb, choose = _inputs(1, 8, 1, dev)
    with pytest.raises(NotImplementedError):
        vit.image_features(rgb.to(dev), choose.to(dev), W)
