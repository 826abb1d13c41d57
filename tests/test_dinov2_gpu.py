"""ISM's proposal descriptors on the library (sam6d_hip.dinov2, csrc/dinov2.hip) against the restatement of tests/dinov2_ref.py in
float64 and the eager fp32 module: crops bitwise, each piece alone, the whole ViT-L/14 encoder, masked patch descriptors, the drop-in
CustomDINOv2 end to end through the detector's scoring, the SAM6D_HIP_DINOV2 switch and range safety."""
import copy
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from sam6d_hip import dinov2, pem
from tests import dinov2_ref as R
from tests._util import golden

pytestmark = pytest.mark.gpu

HEADS = 16


def _mod():
    return importlib.import_module("model.dinov2")


def _randomize(m, seed, gamma=(1.0, 0.1)):
    """tests/test_vit_gpu.py::_randomize plus LayerScale gammas around gamma[0] with relative spread gamma[1]."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("gamma"):
                p.copy_(gamma[0] * (1.0 + gamma[1] * torch.randn(p.shape, generator=g)))
            elif name.endswith("weight") and p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return m


def _rel(got, ref):
    return float((got.double() - ref.to(got.device)).abs().max()) / float(ref.abs().max())


@pytest.fixture(scope="module")
def model():
    return _randomize(_mod().DinoVisionTransformer(), 1).eval()


@pytest.fixture(scope="module")
def sd64(model, dev):
    return R.to_dtype(model.state_dict(), torch.float64, dev)


def _weights(model, dev, mode):
    return dinov2.DinoWeights(model.state_dict(), dev, options=pem.Options(matmul_mode=mode))


def _images(N, seed):
    return torch.randn(N, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ 5. crops
def _scene(seed, n_random=12, H=480, W=640):
    """A 480 x 640 image, the box classes of tests/golden/crop_resize_pad.npz (moved into this image) and random Detections-style
    masks (rectangles and discs) with their tight boxes (exclusive ends)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    z = golden("crop_resize_pad")
    boxes = [tuple(int(v) for v in b) for b in z["boxes"]]
    boxes += [(0, 0, W, H), (W - 224, H - 100, W, H), (0, H - 1, 150, H), (W - 1, 0, W, 97), (100, 100, 400, 424)]
    masks = []
    for (x1, y1, x2, y2) in boxes:
        m = torch.zeros(H, W)
        m[y1:y2, x1:x2] = (torch.rand(y2 - y1, x2 - x1, generator=g) > 0.3).float()
        masks.append(m)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for _ in range(n_random):
        cx, cy = int(torch.randint(40, W - 40, (1,), generator=g)), int(torch.randint(40, H - 40, (1,), generator=g))
        rx, ry = int(torch.randint(3, 200, (1,), generator=g)), int(torch.randint(3, 200, (1,), generator=g))
        m = ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1.0).float()
        ys, xs = torch.nonzero(m.sum(1))[:, 0], torch.nonzero(m.sum(0))[:, 0]
        boxes.append((int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1))
        masks.append(m)
    return img, torch.stack(masks), torch.tensor(boxes, dtype=torch.long)


def test_crops_bitwise(dev):
    img, masks, boxes = _scene(3)
    want_rgb = R.process_rgb_proposals(img, masks, boxes)
    want_m = R.process_masks_proposals(masks, boxes)
    rgb, m224 = dinov2.crop_proposals(img.to(dev), masks.to(dev), boxes.to(dev))
    for i in range(len(boxes)):  # every proposal
        assert torch.equal(rgb[i].cpu(), want_rgb[i]), ("rgb", i, boxes[i].tolist())
        assert torch.equal(m224[i].cpu(), want_m[i]), ("mask", i, boxes[i].tolist())
    # the drop-in's methods reach the same kernel, one part each
    m = _mod().CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")
    md = masks.to(dev)
    assert torch.equal(m.process_rgb_proposals(img.numpy(), md, boxes.to(dev)).cpu(), want_rgb)
    got_m = m.process_masks_proposals(md, boxes.to(dev))
    assert tuple(md.shape) == (len(boxes), 1, 480, 640) and torch.equal(got_m.cpu(), want_m)


# ------------------------------------------------------------------------------------------------ 6. pieces
def test_token_assembly(model, sd64, dev):
    x = _images(3, 5)
    got = dinov2.embed(x.to(dev), _weights(model, dev, 1))
    assert _rel(got, R.embed(sd64, x.double().to(dev))) <= 1e-5


def test_layernorm1024(dev):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(515, 1024, generator=g) * 3.0 + 0.7
    w, b = 1.0 + 0.1 * torch.randn(1024, generator=g), 0.1 * torch.randn(1024, generator=g)
    got = dinov2.layernorm(x.to(dev), w.to(dev), b.to(dev))
    assert _rel(got, R.layernorm(x.double(), w.double(), b.double())) <= 2e-6


def _attn_ref(qkv, B):
    return R.attention(qkv.double().reshape(B, -1, 3072), HEADS).reshape(-1, 1024)


@pytest.mark.parametrize("n", [257, 1, 16, 17, 256])
def test_attention_alone(dev, n):
    B = 3
    qkv = torch.randn(B * n, 3072, generator=torch.Generator().manual_seed(11 + n)) * 3.0
    got = dinov2.attention(qkv.to(dev), B)
    ref = _attn_ref(qkv, B)
    q32, k32, v32 = (t.to(dev) for t in qkv.reshape(B, n, 3, HEADS, 64).permute(2, 0, 3, 1, 4))
    eager = F.scaled_dot_product_attention(q32, k32, v32).transpose(1, 2).reshape(B * n, 1024)
    e, e_eager = _rel(got, ref), _rel(eager, ref)
    print("\n[dinov2] attention n=%d: max|HIP - f64| / max|f64| = %.3e, eager fp32 SDPA: %.3e" % (n, e, e_eager))
    assert torch.isfinite(got).all()
    assert e <= 1e-5  # the bound of the ViT-B attention test: logits up to ~70, fp32's own rounding of them is ~4e-6


def test_attention_outliers(dev):
    """q near fp16's subnormals, k and v beyond fp16's range (same logits as moderate q, k): finite and as accurate as usual."""
    B, n = 2, 257
    qkv = torch.randn(B * n, 3072, generator=torch.Generator().manual_seed(17)) * 3.0
    qkv[:, :1024] /= 2e4
    qkv[:, 1024:] *= 2e4
    qkv[5, 2048 + 7] = 3e9  # one huge value of v
    got = dinov2.attention(qkv.to(dev), B)
    ref = _attn_ref(qkv, B)
    assert torch.isfinite(got).all()
    err = (got.double().cpu() - ref).abs()
    heads = ref.reshape(B * n, HEADS, 64).abs().amax(dim=(0, 2))  # per head: one huge v sets that head's scale
    e = float((err.reshape(B * n, HEADS, 64).amax(dim=(0, 2)) / heads).max())
    print("\n[dinov2] attention outliers: max per-head |HIP - f64| / max|f64| = %.3e" % e)
    assert e <= 1e-5


@pytest.mark.parametrize("mode", [1, 0])
def test_one_block(model, sd64, dev, mode):
    x = torch.randn(2, 257, 1024, generator=torch.Generator().manual_seed(7))
    got = dinov2.block(x.to(dev), _weights(model, dev, mode), 4)
    ref = R.block(sd64, 4, x.double().to(dev), HEADS)
    with torch.no_grad():
        eager = copy.deepcopy(model.blocks[4]).to(dev)(x.to(dev))
    e, e_eager = _rel(got, ref), _rel(eager, ref)
    print("\n[dinov2] block mode %d: HIP %.3e, eager fp32 %.3e" % (mode, e, e_eager))
    assert e <= 4.0 * e_eager, (e, e_eager)


# ------------------------------------------------------------------------------------------------ 7. whole encoder
def _encoder_case(m, dev, N, mode, seed=2):
    x = _images(N, seed)
    cls, tok = dinov2.encode(x.to(dev), _weights(m, dev, mode))
    sd = R.to_dtype(m.state_dict(), torch.float64, dev)
    refs = [R.forward(sd, x[i:i + 8].double().to(dev), HEADS) for i in range(0, N, 8)]
    ref_cls, ref_tok = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    m32 = copy.deepcopy(m).to(dev)
    with torch.no_grad():
        fs = [m32.forward_features(x[i:i + 8].to(dev)) for i in range(0, N, 8)]
    e_cls, e_tok = torch.cat([f["x_norm_clstoken"] for f in fs]), torch.cat([f["x_norm_patchtokens"] for f in fs])
    assert cls.shape == (N, 1024) and tok.shape == (N, 256, 1024) and torch.isfinite(cls).all() and torch.isfinite(tok).all()
    return (_rel(cls, ref_cls), _rel(e_cls, ref_cls)), (_rel(tok, ref_tok), _rel(e_tok, ref_tok))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("N", [2, 45])
def test_encoder_vs_float64(model, dev, N, mode):
    """Bound: the HIP path within 4x of the eager fp32 module's own error against the same float64 reference, measured here (fp16 x3
    carries ~22 mantissa bits against fp32's 24).  Measured on MI355X: see DESIGN section 8 row f5."""
    (c, ce), (t, te) = _encoder_case(model, dev, N, mode)
    print("\n[dinov2] encoder N=%d mode %d: cls HIP %.3e eager %.3e | patch HIP %.3e eager %.3e" % (N, mode, c, ce, t, te))
    assert c <= 4.0 * ce, ("cls", c, ce)
    assert t <= 4.0 * te, ("patch", t, te)


@pytest.mark.parametrize("mode", [1, 0])
def test_encoder_small_layerscale(dev, mode):
    """LayerScale gammas around 1e-5, the released checkpoint's init range."""
    m = _randomize(_mod().DinoVisionTransformer(), 4, gamma=(1e-5, 0.1)).eval()
    (c, ce), (t, te) = _encoder_case(m, dev, 2, mode, seed=8)
    print("\n[dinov2] encoder gamma 1e-5 mode %d: cls HIP %.3e eager %.3e | patch HIP %.3e eager %.3e" % (mode, c, ce, t, te))
    assert c <= 4.0 * ce, ("cls", c, ce)
    assert t <= 4.0 * te, ("patch", t, te)


# ------------------------------------------------------------------------------------------------ 8. masked patch descriptors
def test_masked_patch_descriptors(model, sd64, dev):
    img, masks, boxes = _scene(5, n_random=4)
    keep_rows = [0, 1, 2, 5, 11, 15, 23, 24, 25, 26]
    masks, boxes = masks[keep_rows], boxes[keep_rows]
    masks = (masks > 0).float()  # binary: the pooled sum is an integer
    rgbs, m224 = dinov2.crop_proposals(img.to(dev), masks.to(dev), boxes.to(dev))
    W = _weights(model, dev, 1)
    cls, desc = dinov2.descriptors(rgbs, m224, W)
    _, tok64 = R.forward(sd64, rgbs.double(), HEADS)
    keep, ref = R.masked_patch_features(tok64.cpu(), R.process_masks_proposals(masks, boxes).double())
    got_keep = desc.abs().amax(-1).cpu() > 0
    assert torch.equal(got_keep, keep) and 0 < int(keep.sum()) < keep.numel()
    assert float(desc.cpu()[~keep].abs().max()) == 0.0
    m32 = copy.deepcopy(model).to(dev)
    with torch.no_grad():
        e_tok = m32.forward_features(rgbs)["x_norm_patchtokens"]
    _, eager = R.masked_patch_features(e_tok.cpu(), R.process_masks_proposals(masks, boxes))
    e, ee = _rel(desc.cpu()[keep], ref[keep]), _rel(eager[keep], ref[keep])
    print("\n[dinov2] masked patch descriptors: HIP %.3e eager %.3e" % (e, ee))
    assert e <= 4.0 * ee, (e, ee)


# ------------------------------------------------------------------------------------------------ 9. drop-in end to end
class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _Det:
    def __init__(self, masks, boxes):
        self.masks, self.boxes = masks, boxes


def _scores_cpu(q, ref, k=5):
    """cosine similarity (Nq, n_obj, T) and its avg_5 aggregation, plain torch (ISM/model/detector.py:260-296)."""
    sim = torch.einsum("qd,otd->qot", F.normalize(q.double(), dim=-1), F.normalize(ref.double(), dim=-1))
    return sim, sim.topk(k, dim=-1)[0].mean(-1)


def test_dropin_end_to_end(dev):
    mod = _mod()
    loss = importlib.import_module("model.loss")
    det = importlib.import_module("model.detector")
    d = mod.CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")
    _randomize(d.model, 9)
    d.eval()
    # scene: three textured objects; templates are six views (shifts / flips) of each object's patch, proposals cut them from the image
    g = torch.Generator().manual_seed(21)
    H, W, n_obj, T = 240, 320, 3, 6
    img = torch.randint(0, 40, (H, W, 3), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    spots = [(20, 30, 110, 130), (130, 20, 230, 100), (200, 120, 300, 220)]
    for o, (x1, y1, x2, y2) in enumerate(spots):
        f = 0.15 + 0.2 * o
        tex = torch.stack([127 + 120 * torch.sin(f * xx + o), 127 + 120 * torch.cos(f * yy * (o + 1)), 127 + 120 * torch.sin(f * (xx + yy))], -1)
        img[y1:y2, x1:x2] = tex[y1:y2, x1:x2].to(torch.uint8)
    prop_boxes = torch.tensor([(20, 30, 110, 130), (130, 20, 230, 100), (200, 120, 300, 220), (25, 40, 100, 120), (140, 25, 225, 95)])
    tmpl_boxes = torch.tensor([(x1 + 3 * t, y1 + 2 * t, x2 - 2 * t, y2 - 3 * t) for (x1, y1, x2, y2) in spots for t in range(T)])

    def masks_of(boxes):
        m = torch.zeros(len(boxes), H, W)
        for i, (x1, y1, x2, y2) in enumerate(boxes.tolist()):
            m[i, y1:y2, x1:x2] = 1.0
        return m

    def run(device):
        tm = _Det(masks_of(tmpl_boxes).to(device), tmpl_boxes.to(device))
        t_cls, t_patch = d.forward(img.numpy(), tm)
        pm = _Det(masks_of(prop_boxes).to(device), prop_boxes.to(device))
        q_cls, q_patch = d.forward(img.numpy(), pm)
        assert tuple(pm.masks.shape) == (len(prop_boxes), 1, H, W)
        return t_cls.reshape(n_obj, T, 1024), t_patch.reshape(n_obj, T, 256, 1024), q_cls, q_patch

    c_ref, c_appe, c_q, c_qp = run(torch.device("cpu"))
    g_ref, g_appe, g_q, g_qp = run(dev)
    assert g_q.is_cuda and tuple(g_q.shape) == (5, 1024) and tuple(g_qp.shape) == (5, 256, 1024)
    # the CPU path alone: no tie closer than 1e-3 (ten times the 1e-4 contract) at any arg-max or at the threshold
    thresh = 0.2
    sim, agg = _scores_cpu(c_q, c_ref)
    top2 = agg.topk(2, dim=-1)[0]
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3, "object arg-max too close to a tie"
    assert float((top2[:, 0] - thresh).abs().min()) > 1e-3, "semantic score too close to the threshold"
    obj_cpu = agg.argmax(-1)
    t2 = sim[torch.arange(5), obj_cpu].topk(2, dim=-1)[0]
    assert float((t2[:, 0] - t2[:, 1]).min()) > 1e-3, "best template too close to a tie"

    m = det.Instance_Segmentation_Model(segmentor_model=None, descriptor_model=d, onboarding_config=None,
                                        matching_config=_Cfg(metric=loss.PairwiseSimilarity("cosine", 16), aggregation_function="avg_5",
                                                             confidence_thresh=thresh),
                                        post_processing_config=None, log_interval=5, log_dir=".", visible_thred=0.5, pointcloud_sample_num=2048)

    def score(ref, appe, q, qp):
        m.ref_data = {"descriptors": ref.to(dev).contiguous(), "appe_descriptors": appe.to(dev).contiguous()}
        sel, obj, sem, best = m.compute_semantic_score(q.to(dev).contiguous())
        a, _ = m.compute_appearance_score(best, obj, qp.to(dev)[sel].contiguous())
        return sel.cpu(), obj.cpu(), sem.cpu(), best.cpu(), a.cpu()

    s_c, s_g = score(c_ref, c_appe, c_q, c_qp), score(g_ref, g_appe, g_q, g_qp)
    assert len(s_c[0]) > 0
    for i, name in ((0, "selected proposals"), (1, "object ids"), (3, "best templates")):
        assert torch.equal(s_c[i], s_g[i]), name
    assert torch.equal(s_c[1].long(), obj_cpu[s_c[0].long()])
    for i, name in ((2, "semantic score"), (4, "appearance score")):
        e = float((s_c[i] - s_g[i]).abs().max())
        print("\n[dinov2] drop-in %s: max |GPU - CPU| = %.3e" % (name, e))
        assert e <= 1e-4, (name, e)


# ------------------------------------------------------------------------------------------------ 10. switch, range safety
def test_switch_selects_eager(model, dev, monkeypatch):
    d = _mod().CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")
    d.model = copy.deepcopy(model).to(dev)
    x = _images(2, 12).to(dev)
    m224 = (torch.rand(2, 224, 224, generator=torch.Generator().manual_seed(1)) > 0.4).float().to(dev)
    on = d.compute_cls_and_patch_features(x, m224)
    monkeypatch.setenv("SAM6D_HIP_DINOV2", "0")
    off = d.compute_cls_and_patch_features(x, m224)
    with torch.no_grad():
        f = d.model.forward_features(x)
    assert torch.equal(off[0], f["x_norm_clstoken"])
    keep, eager = R.masked_patch_features(f["x_norm_patchtokens"], m224)
    assert torch.equal(off[1], eager)
    assert not torch.equal(on[0], off[0]) and _rel(on[0], off[0].double()) <= 1e-4
    img, masks, boxes = _scene(3, n_random=0)
    want = R.process_rgb_proposals(img, masks[:4], boxes[:4])
    assert torch.equal(d.process_rgb_proposals(img.numpy(), masks[:4].to(dev), boxes[:4].to(dev)).cpu(), want)


def test_range_outliers(dev):
    m = _randomize(_mod().DinoVisionTransformer(), 3).eval()
    b = m.blocks[6]
    with torch.no_grad():
        b.mlp.fc2.weight.mul_(1e3)
        b.mlp.fc1.weight.mul_(2e4)  # fc2's A operand beyond fp16: the GEMM's exact-tile fallback
        for t in (b.attn.qkv.weight, b.attn.qkv.bias):
            t[2048:].mul_(2e4)      # v beyond fp16 (the attention's power-of-two operand scales), proj shrunk by as much
        b.attn.proj.weight.div_(2e4)
    x = _images(2, 4)
    x[:, :, 50:53, 100:103] = 1e4  # a few 1e4-magnitude input pixels
    sd = R.to_dtype(m.state_dict(), torch.float64, dev)
    ref_cls, ref_tok = R.forward(sd, x.double().to(dev), HEADS)
    cls, tok = dinov2.encode(x.to(dev), _weights(m, dev, 1))
    assert torch.isfinite(cls).all() and torch.isfinite(tok).all()
    m32 = copy.deepcopy(m).to(dev)
    with torch.no_grad():
        f = m32.forward_features(x.to(dev))
    e, ee = _rel(tok, ref_tok), _rel(f["x_norm_patchtokens"], ref_tok)
    print("\n[dinov2] outliers: patch HIP %.3e eager %.3e, cls HIP %.3e" % (e, ee, _rel(cls, ref_cls)))
    assert e <= 4.0 * ee, (e, ee)


def test_mode2_refused(model, dev):
    with pytest.raises(NotImplementedError):
        dinov2.encode(_images(1, 1).to(dev), _weights(model, dev, 2))
