"""Host orchestration of PEM's image features on the library: the ViT-B/16 encoder, the pyramid taps, output_upscaling and the
chosen-pixel bilinear gather (PEM/model/feature_extraction.py:21-35 ViT.forward, :98-118 ViT_AE.forward, :141-142 get_img_feats,
PEM/utils/model_utils.py:86-98 get_chosen_pixel_feats).  torch provides device buffers only.

The encoder itself (patch embedding, blocks, LayerNorm launches) is encoder.py's, described by ENC below: the residual stream is
X (B*197, 768) fp32, row 0 of each image the cls token.
After blocks 2, 5, 8 and 11 the final norm writes the 196 patch rows of each image into the (B*196, 3072) concat buffer at column
768 j; output_upscaling reads that buffer and the fused gather reads only the four bilinear taps of each chosen pixel, so the
(B, 256, 224, 224) map of the eager path is never formed.
"""
import torch

from . import _lib, encoder
from .runtime import Linear, _empty, _getter, _p, _s, gemm, on_tensor_device

D = 768        # embed_dim of vit_base
NP = 196       # patches of a 224 x 224 image
NT = NP + 1    # tokens: cls + patches
HID = 4 * D    # MLP hidden width
DEPTH = 12
TAPS = (2, 5, 8, 11)  # ViT.forward's `want` blocks, in the order their norms are concatenated
OUT = 256      # out_dim
IMG = 224
EPS = 1e-6     # partial(nn.LayerNorm, eps=1e-6)
ENC = encoder.Encoder("sam6d_hip.vit", "image encoder", D, HID, DEPTH, NP, NT, 3 * 16 * 16, EPS, "sam6d_vit_patch_rows",
                      "sam6d_vit_layernorm768", "sam6d_vit_attention")


def check_config(cfg):
    """The one configuration this path implements (PEM/config/base.yaml:19-25): vit_base, up_type linear, pyramid features."""
    if cfg is None:
        return
    vt, up = getattr(cfg, "vit_type", "vit_base"), getattr(cfg, "up_type", "linear")
    if vt != "vit_base":
        raise NotImplementedError("sam6d_hip.vit: only vit_type 'vit_base' is implemented (got %r)" % vt)
    if up != "linear":
        raise NotImplementedError("sam6d_hip.vit: only up_type 'linear' is implemented (got %r)" % up)
    if not getattr(cfg, "use_pyramid_feat", True):
        raise NotImplementedError("sam6d_hip.vit: only use_pyramid_feat True is implemented")
    if getattr(cfg, "embed_dim", D) != D or getattr(cfg, "out_dim", OUT) != OUT:
        raise NotImplementedError("sam6d_hip.vit: only embed_dim 768 / out_dim 256 are implemented")


def check_inputs(rgb, choose):
    """rgb (B,3,224,224) float32, choose (B,N) integer pixel indices."""
    if rgb.dim() != 4 or tuple(rgb.shape[1:]) != (3, IMG, IMG):
        raise ValueError("sam6d_hip.vit: images must be (B, 3, 224, 224), got %s" % (tuple(rgb.shape),))
    if rgb.dtype != torch.float32:
        raise ValueError("sam6d_hip.vit: images must be float32, got %s" % rgb.dtype)
    if choose.dim() != 2 or choose.shape[0] != rgb.shape[0]:
        raise ValueError("sam6d_hip.vit: choose must be (B, N) with the images' B, got %s" % (tuple(choose.shape),))
    if choose.dtype.is_floating_point or choose.dtype == torch.bool:
        raise ValueError("sam6d_hip.vit: choose must hold integer pixel indices, got %s" % choose.dtype)


def _check_images(rgb):
    check_inputs(rgb, torch.zeros((rgb.shape[0], 0), dtype=torch.long))


class VitWeights(encoder.Weights):
    """feature_extraction.rgb_net.* packed once: the patch conv as a (768, 768) matrix in (c, kh, kw) column order, qkv / proj / fc1 /
    fc2 of the 12 blocks and output_upscaling as Linear objects (fp32 + the pre-split fp16 halves of the w16 GEMM route), the norms,
    cls_token and pos_embed.  sd: a Net state_dict (keys under feature_extraction.rgb_net.) or the ViT_AE's own.  cfg: the
    feature_extraction config, checked when given; the weights' shapes are checked always."""

    def __init__(self, sd, dev, options=None, cfg=None):
        check_config(cfg)
        pre = "feature_extraction.rgb_net."
        if pre + "vit.cls_token" not in sd:
            pre = ""
        if pre + "output_upscaling.weight" not in sd:
            raise NotImplementedError("sam6d_hip.vit: no output_upscaling.weight (up_type 'deconv' is not implemented)")
        depth = 0
        while ("%svit.blocks.%d.attn.qkv.weight" % (pre, depth)) in sd:
            depth += 1
        dim = sd[pre + "vit.cls_token"].shape[-1]
        if dim != D or depth != DEPTH:
            raise NotImplementedError("sam6d_hip.vit: only vit_base (768 channels, 12 blocks) is implemented, got %d x %d" % (dim, depth))
        if tuple(sd[pre + "output_upscaling.weight"].shape) != (16 * OUT, 4 * D):
            raise NotImplementedError("sam6d_hip.vit: output_upscaling must be (4096, 3072) (pyramid features, out_dim 256)")
        dev = torch.device(dev)
        self.dev = dev
        self.options = options
        g = _getter(sd, dev)
        v = pre + "vit."
        with encoder.device_of(dev):
            self.patch = Linear(g(v + "patch_embed.proj.weight").reshape(D, ENC.K), g(v + "patch_embed.proj.bias"))
            self.cls = g(v + "cls_token").reshape(D)
            self.pos = g(v + "pos_embed").reshape(NT * D)
            self.blocks = [encoder.pack_block(g, "%sblocks.%d." % (v, i)) for i in range(ENC.depth)]
            self.norm = (g(v + "norm.weight"), g(v + "norm.bias"))
            self.up = Linear(g(pre + "output_upscaling.weight"), g(pre + "output_upscaling.bias"))
            self.cut_w16()

    def linears(self):
        yield from super().linears()
        yield self.up


@on_tensor_device
def encode(rgb, W, options=None):
    """rgb (B,3,224,224) -> (X (B,197,768) after the last block, cat (B,196,3072) = the four normalised pyramid taps)."""
    ENC.require_mode()
    _check_images(rgb)
    rgb = rgb.contiguous()
    B = rgb.shape[0]
    X = _empty((B * NT, D), rgb)
    Y = _empty((B * NT, D), rgb)
    T = _empty((B * NT, HID), rgb)
    cat = _empty((B * NP, 4 * D), rgb)
    ENC.embed(rgb, W, X, cat)  # (the patch rows live in the concat buffer until the first tap)
    for i, blk in enumerate(W.blocks):
        ENC.block(X, blk, B, Y, T)
        if i in TAPS:
            j = TAPS.index(i)
            ENC.ln(X, W.norm, cat, B, NP, D, NT * D, 4 * D, NP * 4 * D, x_off=D, y_off=D * j)
    return X.view(B, NT, D), cat.view(B, NP, 4 * D)


@on_tensor_device
def upsample_gather(U, choose, options=None):
    """U (B*196, 4096) output_upscaling output, choose (B,N) -> (B,N,256) = get_chosen_pixel_feats(bilinear 224 x 224 map, choose)."""
    B, N = choose.shape
    if U.dtype != torch.float32 or tuple(U.shape) != (B * NP, 16 * OUT) or not U.is_contiguous():
        raise ValueError("sam6d_hip.vit: U must be a contiguous float32 (B*196, 4096) tensor")
    choose = choose.to(device=U.device, dtype=torch.long).contiguous()
    out = _empty((B, N, OUT), U)
    _lib.call("sam6d_vit_upsample_gather", _p(U), choose.data_ptr(), _p(out), B, N, _s())
    return out


@on_tensor_device
def image_features(rgb, choose, W, options=None):
    """dense_fm (B,N,256) = get_chosen_pixel_feats(ViT_AE(rgb)[0], choose) (feature_extraction.py:141-142)."""
    ENC.require_mode()
    check_inputs(rgb, choose)
    B = rgb.shape[0]
    _, cat = encode(rgb, W)
    U = _empty((B * NP, 16 * OUT), rgb)
    gemm(cat, W.up.w, W.up.b, U, B * NP, 16 * OUT, 4 * D, 4 * D, 4 * D, 16 * OUT, w16=W.up.w16())
    return upsample_gather(U, choose)


# embed(rgb, W), layernorm(x, gamma, beta), attention(qkv, B), block(x, W, i): single stages of the encoder, for the tests
embed, layernorm, attention, block = encoder.pieces(ENC, _check_images)
