"""Host orchestration of PEM's image features on the library: the ViT-B/16 encoder, the pyramid taps, output_upscaling and the
chosen-pixel bilinear gather (PEM/model/feature_extraction.py:21-35 ViT.forward, :98-118 ViT_AE.forward, :141-142 get_img_feats,
PEM/utils/model_utils.py:86-98 get_chosen_pixel_feats).  torch provides device buffers only.

Layout: the residual stream is X (B*197, 768) fp32, row 0 of each image the cls token.  Per block:
    LN1 -> qkv GEMM -> attention -> proj GEMM (+ X, in place) -> LN2 -> fc1 GEMM (GELU) -> fc2 GEMM (+ X, in place)
In-place residual: every GEMM route loads the residual element it adds before it stores that same element of C (the stored value
depends on it), and each element of C belongs to exactly one lane, so C == residual is safe (tests/test_vit_gpu.py checks every route).
After blocks 2, 5, 8 and 11 the final norm writes the 196 patch rows of each image into the (B*196, 3072) concat buffer at column
768 j; output_upscaling reads that buffer and the fused gather reads only the four bilinear taps of each chosen pixel, so the
(B, 256, 224, 224) map of the eager path is never formed.
"""
import torch

from . import _lib
from .pem import Linear, _empty, _flags, _getter, _p, _s, gemm, on_tensor_device

D = 768        # embed_dim of vit_base
NP = 196       # patches of a 224 x 224 image
NT = NP + 1    # tokens: cls + patches
HID = 4 * D    # MLP hidden width
DEPTH = 12
TAPS = (2, 5, 8, 11)  # ViT.forward's `want` blocks, in the order their norms are concatenated
OUT = 256      # out_dim
IMG = 224
EPS = 1e-6     # partial(nn.LayerNorm, eps=1e-6)


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


class VitWeights:
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
        with torch.cuda.device(dev) if dev.type == "cuda" else _nullctx():
            self.patch = Linear(g(v + "patch_embed.proj.weight").reshape(D, 3 * 16 * 16), g(v + "patch_embed.proj.bias"))
            self.cls = g(v + "cls_token").reshape(D)
            self.pos = g(v + "pos_embed").reshape(NT * D)
            self.blocks = []
            for i in range(DEPTH):
                b = "%sblocks.%d." % (v, i)
                self.blocks.append(dict(
                    n1=(g(b + "norm1.weight"), g(b + "norm1.bias")),
                    qkv=Linear(g(b + "attn.qkv.weight"), g(b + "attn.qkv.bias")),
                    proj=Linear(g(b + "attn.proj.weight"), g(b + "attn.proj.bias")),
                    n2=(g(b + "norm2.weight"), g(b + "norm2.bias")),
                    fc1=Linear(g(b + "mlp.fc1.weight"), g(b + "mlp.fc1.bias")),
                    fc2=Linear(g(b + "mlp.fc2.weight"), g(b + "mlp.fc2.bias"))))
            self.norm = (g(v + "norm.weight"), g(v + "norm.bias"))
            self.up = Linear(g(pre + "output_upscaling.weight"), g(pre + "output_upscaling.bias"))
            if dev.type == "cuda":
                for lin in self.linears():
                    lin.w16()  # the fp16 halves, cut once here

    def linears(self):
        yield self.patch
        for b in self.blocks:
            yield from (b["qkv"], b["proj"], b["fc1"], b["fc2"])
        yield self.up


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ------------------------------------------------------------------------------------------------- launches
def _ln(x, gb, y, nimg, rows, ldx, sx, ldy, sy, x_off=0, y_off=0):
    _lib.call("sam6d_vit_layernorm768", _p(x, x_off), _p(gb[0]), _p(gb[1]), _p(y, y_off), nimg, rows, ldx, sx, ldy, sy, EPS, _s())


def _embed(rgb, W, X, A):
    """X (B*197, 768) = [cls_token; patch_embed(rgb)] + pos_embed; A (B*196, 768) is the patch-row workspace."""
    B = rgb.shape[0]
    _lib.call("sam6d_vit_patch_rows", _p(rgb), _p(W.cls), _p(W.pos), _p(A), _p(X), B, _s())
    # one problem per image: rows land one below the image's cls row, pos_embed[1:] is the residual (batch stride 0)
    gemm(A, W.patch.w, W.patch.b, X, NP, D, D, D, D, D, c_off=D, residual=W.pos, r_off=D, ldr=D, batch=B, sA=NP * D, sW=0,
         sC=NT * D, sR=0, w16=W.patch.w16())


def _block(X, blk, B, Y, T):
    """One ViT block on X (B*197, 768) in place; Y (B*197, 768) and T (>= B*197*3072 floats) are workspaces."""
    M = B * NT
    _ln(X, blk["n1"], Y, 1, M, D, 0, D, 0)
    gemm(Y, blk["qkv"].w, blk["qkv"].b, T, M, 3 * D, D, D, D, 3 * D, w16=blk["qkv"].w16())
    _lib.call("sam6d_vit_attention", _p(T), _p(Y), B, NT, _s())
    gemm(Y, blk["proj"].w, blk["proj"].b, X, M, D, D, D, D, D, residual=X, ldr=D, w16=blk["proj"].w16())
    _ln(X, blk["n2"], Y, 1, M, D, 0, D, 0)
    gemm(Y, blk["fc1"].w, blk["fc1"].b, T, M, HID, D, D, D, HID, act=2, w16=blk["fc1"].w16())
    gemm(T, blk["fc2"].w, blk["fc2"].b, X, M, D, HID, HID, HID, D, residual=X, ldr=D, w16=blk["fc2"].w16())


def _require_mode():
    if _flags().mode == 2:
        raise NotImplementedError("sam6d_hip.vit: matmul mode 2 is not implemented for the image encoder (modes 0 and 1 are)")


@on_tensor_device
def encode(rgb, W, options=None):
    """rgb (B,3,224,224) -> (X (B,197,768) after the last block, cat (B,196,3072) = the four normalised pyramid taps)."""
    _require_mode()
    check_inputs(rgb, torch.zeros((rgb.shape[0], 0), dtype=torch.long))
    rgb = rgb.contiguous()
    B = rgb.shape[0]
    X = _empty((B * NT, D), rgb)
    Y = _empty((B * NT, D), rgb)
    T = _empty((B * NT, HID), rgb)
    cat = _empty((B * NP, 4 * D), rgb)
    _embed(rgb, W, X, cat)  # (the patch rows live in the concat buffer until the first tap)
    for i, blk in enumerate(W.blocks):
        _block(X, blk, B, Y, T)
        if i in TAPS:
            j = TAPS.index(i)
            _ln(X, W.norm, cat, B, NP, D, NT * D, 4 * D, NP * 4 * D, x_off=D, y_off=D * j)
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
    _require_mode()
    check_inputs(rgb, choose)
    B = rgb.shape[0]
    _, cat = encode(rgb, W)
    U = _empty((B * NP, 16 * OUT), rgb)
    gemm(cat, W.up.w, W.up.b, U, B * NP, 16 * OUT, 4 * D, 4 * D, 4 * D, 16 * OUT, w16=W.up.w16())
    return upsample_gather(U, choose)


@on_tensor_device
def attention(qkv, B, options=None):
    """qkv (B*n, 2304) -> (B*n, 768): the block's multi-head attention alone (sam6d_vit_attention)."""
    qkv = qkv.contiguous()
    out = _empty((qkv.shape[0], D), qkv)
    _lib.call("sam6d_vit_attention", _p(qkv), _p(out), B, qkv.shape[0] // B, _s())
    return out


@on_tensor_device
def block(x, W, i, options=None):
    """x (B,197,768) -> block i of the encoder applied to a copy."""
    _require_mode()
    B = x.shape[0]
    X = x.reshape(B * NT, D).contiguous().clone()
    _block(X, W.blocks[i], B, _empty((B * NT, D), X), _empty((B * NT, HID), X))
    return X.view(B, NT, D)


@on_tensor_device
def embed(rgb, W, options=None):
    """rgb (B,3,224,224) -> X (B,197,768) = cat(cls_token, patch_embed(rgb)) + pos_embed."""
    check_inputs(rgb, torch.zeros((rgb.shape[0], 0), dtype=torch.long))
    rgb = rgb.contiguous()
    B = rgb.shape[0]
    X = _empty((B * NT, D), rgb)
    _embed(rgb, W, X, _empty((B * NP, D), rgb))
    return X.view(B, NT, D)
