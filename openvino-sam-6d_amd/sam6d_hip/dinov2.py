"""Host orchestration of ISM's proposal descriptors on the library: CropResizePad and the DINOv2 ViT-L/14 encoder
(ISM/model/dinov2.py:115-326 CustomDINOv2, ISM/utils/bbox_utils.py:89-126, ISM/model/vision_transformer.py:179-266, ISM/model/layers).
torch provides device buffers only (and, once at pack time on the host, the bicubic interpolation of the position embedding).

The encoder itself (patch embedding, blocks, LayerNorm launches) is encoder.py's, described by ENC below: the residual stream is
X (N*257, 1024) fp32, row 0 of each image the cls token.
LayerScale (ls1.gamma, ls2.gamma) is folded into the rows of proj / fc2 and their biases at pack time: gamma * (W y + b) =
(gamma W) y + gamma b, so the GEMMs with the in-place residual are the ones the ViT-B encoder uses.  The patch GEMM reads K = 608
columns: the 588 = 3 x 14 x 14 values of a patch and 20 zeros in both operands, so that K is a multiple of the 32-wide k-step and every
GEMM route applies.  The final LayerNorm writes x_norm_clstoken and x_norm_patchtokens straight into their own tensors.

Memory: the images are worked through in slices of SLICE = 64.  A slice holds X and Y (64 * 257 * 1024 floats each), T
(64 * 257 * 4096 floats: the qkv rows, then the MLP hidden rows) and the patch rows A (64 * 256 * 608 floats): 443 MB at most,
whatever N is; beside them only the outputs ((N, 1024) and (N, 256, 1024)) grow with N.
"""
import math

import torch
import torch.nn.functional as F

from . import _lib, encoder
from .ism import masked_patch_features
from .runtime import Linear, _empty, _getter, _p, _s, on_tensor_device

D = 1024       # embed_dim of vit_large
HEADS = 16
PATCH = 14
IMG = 224
GRID = IMG // PATCH   # 16
NP = GRID * GRID      # 256 patches
NT = NP + 1           # tokens: cls + patches
HID = 4 * D
DEPTH = 24
KP = 3 * PATCH * PATCH  # 588 values of a patch
KPAD = 608              # ... padded to 19 k-steps of 32
EPS = 1e-6              # partial(nn.LayerNorm, eps=1e-6)
SLICE = 64              # images per pass of the encoder (see the module docstring)
MAXN = 272              # sam6d_dino_attention's token limit
ENC = encoder.Encoder("sam6d_hip.dinov2", "descriptor model", D, HID, DEPTH, NP, NT, KPAD, EPS, "sam6d_dino_patch_rows",
                      "sam6d_dino_layernorm1024", "sam6d_dino_attention")


def interpolate_pos_embed(pos_embed, grid=GRID, offset=0.1):
    """interpolate_pos_encoding of the reference (ISM/model/vision_transformer.py:179-207) for a grid x grid patch grid: bicubic,
    scale_factor = (grid + offset) / sqrt(N), no antialias.  pos_embed (1, 1 + N, dim) -> (1, 1 + grid * grid, dim), on pos_embed's
    device and in float32 as the reference computes it (`.float()`), cast back to pos_embed's dtype."""
    prev = pos_embed.dtype
    n = pos_embed.shape[1] - 1
    if n == grid * grid:
        return pos_embed
    pe = pos_embed.float()
    dim = pe.shape[-1]
    sqrt_n = math.sqrt(n)
    s = float(grid + offset) / sqrt_n
    patch = F.interpolate(pe[:, 1:].reshape(1, int(sqrt_n), int(sqrt_n), dim).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic",
                          antialias=False)
    assert patch.shape[-2] == grid and patch.shape[-1] == grid
    patch = patch.permute(0, 2, 3, 1).reshape(1, -1, dim)
    return torch.cat((pe[:, 0].unsqueeze(0), patch), dim=1).to(prev)


def fold_layerscale(w, b, gamma):
    """(gamma[:, None] * w, gamma * b): ls(x) = gamma * (W x + b) as one Linear (ISM/model/layers/layer_scale.py:27-28)."""
    return gamma[:, None] * w, gamma * b


def _strip(sd):
    if "cls_token" not in sd and "model.cls_token" in sd:
        return {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    return sd


def check_state_dict(sd):
    """The one configuration this path implements: vit_large(patch_size=14, img_size=518, init_values=1.0, block_chunks=0), MLP FFN,
    no register tokens.  Anything else raises NotImplementedError with the offending value."""
    if "cls_token" not in sd:
        raise NotImplementedError("sam6d_hip.dinov2: no cls_token in the state dict (keys of a DinoVisionTransformer are expected)")
    if "register_tokens" in sd:
        raise NotImplementedError("sam6d_hip.dinov2: register tokens are not implemented (got %d)" % sd["register_tokens"].shape[1])
    if any(k.startswith("blocks.0.0.") for k in sd):
        raise NotImplementedError("sam6d_hip.dinov2: chunked blocks (block_chunks > 0) are not implemented")
    if "blocks.0.mlp.w12.weight" in sd:
        raise NotImplementedError("sam6d_hip.dinov2: the swiglu FFN is not implemented (only 'mlp')")
    if "blocks.0.ls1.gamma" not in sd:
        raise NotImplementedError("sam6d_hip.dinov2: blocks without LayerScale (init_values None) are not implemented")
    depth = 0
    while ("blocks.%d.attn.qkv.weight" % depth) in sd:
        depth += 1
    dim = sd["cls_token"].shape[-1]
    if dim != D or depth != DEPTH:
        raise NotImplementedError("sam6d_hip.dinov2: only vit_large (1024 channels, 24 blocks) is implemented, got %d x %d" % (dim, depth))
    pw = tuple(sd["patch_embed.proj.weight"].shape)
    if pw != (D, 3, PATCH, PATCH):
        raise NotImplementedError("sam6d_hip.dinov2: only patch size 14 on 3 channels is implemented, got a patch weight %s" % (pw,))
    hid = sd["blocks.0.mlp.fc1.weight"].shape[0]
    if hid != HID:
        raise NotImplementedError("sam6d_hip.dinov2: only mlp_ratio 4 is implemented, got a hidden width of %d" % hid)
    n = sd["pos_embed"].shape[1] - 1
    if int(math.sqrt(n)) ** 2 != n:
        raise NotImplementedError("sam6d_hip.dinov2: pos_embed must hold a square patch grid, got %d positions" % n)


class DinoWeights(encoder.Weights):
    """A dinov2_vitl14 state dict (with or without a `model.` prefix) packed once: the patch conv as a (1024, 608) matrix in
    (c, kh, kw) column order with zero columns 588..607, qkv / proj / fc1 / fc2 of the 24 blocks as Linear objects (fp32 + the pre-split
    fp16 halves of the w16 GEMM route) with LayerScale folded into proj and fc2, the norms, cls_token and the position embedding
    interpolated to the 16 x 16 grid of a 224 x 224 image with the reference's own recipe (torch on the host, in float32: the
    reference's tensor bit for bit)."""

    def __init__(self, sd, dev, options=None):
        sd = _strip(sd)
        check_state_dict(sd)
        dev = torch.device(dev)
        self.dev = dev
        self.options = options
        g = _getter(sd, dev)
        g64 = lambda k: sd[k].detach().to(device="cpu", dtype=torch.float64)  # noqa: E731
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731

        def fold(lin, ls):  # in float64, rounded to fp32 once
            return map(f32, fold_layerscale(g64(lin + ".weight"), g64(lin + ".bias"), g64(ls + ".gamma")))

        with encoder.device_of(dev):
            pw = torch.zeros((D, KPAD), dtype=torch.float32, device=dev)
            pw[:, :KP] = g("patch_embed.proj.weight").reshape(D, KP)
            self.patch = Linear(pw, g("patch_embed.proj.bias"))
            self.cls = g("cls_token").reshape(D)
            self.pos_full = interpolate_pos_embed(sd["pos_embed"].detach().to("cpu"))  # (1, 257, 1024), host
            self.pos = self.pos_full.to(device=dev, dtype=torch.float32).reshape(NT * D).contiguous()
            self.blocks = [encoder.pack_block(g, "blocks.%d." % i, fold) for i in range(ENC.depth)]
            self.norm = (g("norm.weight"), g("norm.bias"))
            self.cut_w16()


def check_images(images):
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("sam6d_hip.dinov2: images must be (N, 3, 224, 224), got %s" % (tuple(images.shape),))
    if tuple(images.shape[2:]) != (IMG, IMG):
        raise NotImplementedError("sam6d_hip.dinov2: only 224 x 224 images are implemented, got %d x %d" % tuple(images.shape[2:]))
    if images.dtype != torch.float32:
        raise ValueError("sam6d_hip.dinov2: images must be float32, got %s" % images.dtype)


# ------------------------------------------------------------------------------------------------- crops in plain torch
def _nearest_map(out, scale, size):
    """Source index of every output index of a nearest resize that was given `scale`: min(floor(dst * fl32(1 / scale)), size - 1),
    the product in float32 (ATen's upsample_nearest)."""
    step = torch.tensor(1.0 / scale, dtype=torch.float32)
    return (torch.arange(out, dtype=torch.float32) * step).floor().long().clamp_(max=size - 1)


def crop_index_maps(boxes, H, W, target=IMG):
    """The gather that CropResizePad(target) amounts to (ISM/utils/bbox_utils.py:89-126), as index maps: for N integer xyxy boxes
    (exclusive ends) on an H x W image, rows (N, target) and cols (N, target) of the source pixel of every output row / column, and
    row_ok / col_ok (N, target) bool, False where the output is padding.  Composed per box from the second resize, the padding
    (top / left get max((target - side) // 2, 0)) and the first resize by target / max(box side); that scale factor is formed the way
    torch forms `number / tensor`: reciprocal, then times the number, both in float32.  Host tensors."""
    b = boxes.detach().to("cpu")
    if b.dim() != 2 or b.shape[1] != 4 or b.dtype.is_floating_point or b.dtype == torch.bool:
        raise ValueError("sam6d_hip.dinov2: boxes must be (N, 4) integers, got %s %s" % (tuple(b.shape), b.dtype))
    b = b.long()
    long_side = torch.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    factor = (long_side.to(torch.float32).reciprocal() * float(target)).tolist()
    N = b.shape[0]
    rows = torch.zeros((N, target), dtype=torch.long)
    cols = torch.zeros((N, target), dtype=torch.long)
    row_ok = torch.zeros((N, target), dtype=torch.bool)
    col_ok = torch.zeros((N, target), dtype=torch.bool)
    ident = torch.arange(target)
    for i, (bx, s) in enumerate(zip(b.tolist(), factor)):
        x1, x2 = (min(max(v, 0), W) for v in (bx[0], bx[2]))
        y1, y2 = (min(max(v, 0), H) for v in (bx[1], bx[3]))
        cw, ch = x2 - x1, y2 - y1
        if cw <= 0 or ch <= 0 or not math.isfinite(s):
            raise ValueError("sam6d_hip.dinov2: box %d = %s is empty" % (i, bx))
        rw, rh = math.floor(cw * s), math.floor(ch * s)
        if rw <= 0 or rh <= 0:
            raise ValueError("sam6d_hip.dinov2: box %d = %s resizes to an empty crop (%d x %d)" % (i, bx, rw, rh))
        top = left = 0
        back = ident  # output pixel -> pixel of the padded square
        if rw != rh:
            top, left = max((target - rh) // 2, 0), max((target - rw) // 2, 0)
        elif rw != target:
            if math.floor(rw * (target / rw)) != target:
                raise ValueError("sam6d_hip.dinov2: box %d = %s: the second resize of side %d does not give %d" % (i, bx, rw, target))
            back = _nearest_map(target, target / rw, rw)
        ry, rx = back - top, back - left
        row_ok[i], col_ok[i] = (ry >= 0) & (ry < rh), (rx >= 0) & (rx < rw)
        rows[i] = y1 + _nearest_map(rh, s, ch)[ry.clamp(0, rh - 1)]
        cols[i] = x1 + _nearest_map(rw, s, cw)[rx.clamp(0, rw - 1)]
    return rows, cols, row_ok, col_ok


def crop_resize_pad(images, boxes, target=IMG, masks=None):
    """CropResizePad(target)(images, boxes) in plain torch on the images' device, any dtype: the eager partner of crop_proposals.
    images (N, C, H, W), or (C, H, W) for one image shared by all boxes; masks (N, H, W), when given, multiply the gathered pixels
    (the same product as masking before the crop, without N copies of the image).  -> (N, C, target, target)."""
    shared = images.dim() == 3
    H, W = images.shape[-2:]
    dev = images.device
    rows, cols, row_ok, col_ok = (t.to(dev) for t in crop_index_maps(boxes, H, W, target))
    N = rows.shape[0]
    if N == 0:
        return images.new_zeros((0, images.shape[-3], target, target))
    yy, xx = rows[:, :, None], cols[:, None, :]
    if shared:
        out = images[:, yy, xx].permute(1, 0, 2, 3)
    else:
        out = images[torch.arange(N, device=dev)[:, None, None], :, yy, xx].permute(0, 3, 1, 2)
    if masks is not None:
        out = out * masks.to(dev)[torch.arange(N, device=dev)[:, None, None], yy, xx].to(out.dtype)[:, None]
    inside = (row_ok[:, :, None] & col_ok[:, None, :])[:, None]
    return torch.where(inside, out, torch.zeros((), dtype=out.dtype, device=dev)).contiguous()


@on_tensor_device
def crop_proposals(image_u8, masks, boxes, rgb=True, mask=True, options=None):
    """process_rgb_proposals + process_masks_proposals (ISM/model/dinov2.py:160-173, 221-232) in one launch.  image_u8 (H, W, 3) uint8,
    masks (N, H, W) (any dtype: used as float32, as `rgbs * masks` promotes them), boxes (N, 4) integer xyxy with exclusive ends ->
    (rgbs (N, 3, 224, 224), masks224 (N, 224, 224)) float32; a part that is not asked for is None
    (and image_u8 may be None when only the masks are asked for).  Floating-point boxes raise ValueError, here as in the eager
    crop_resize_pad (the drop-in's `Detections` holds int64 boxes)."""
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if image_u8 is None and not rgb:  # masks alone: no image is read
        H, Wd = masks.shape[-2:]
    elif image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError("sam6d_hip.dinov2: the image must be (H, W, 3) uint8, got %s %s" % (tuple(image_u8.shape), image_u8.dtype))
    else:
        H, Wd = image_u8.shape[:2]
    if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, Wd):
        raise ValueError("sam6d_hip.dinov2: masks must be (N, %d, %d), got %s" % (H, Wd, tuple(masks.shape)))
    N = masks.shape[0]
    if tuple(boxes.shape) != (N, 4) or boxes.dtype.is_floating_point:
        raise ValueError("sam6d_hip.dinov2: boxes must be (N, 4) integers, got %s %s" % (tuple(boxes.shape), boxes.dtype))
    dev = masks.device
    img = image_u8.to(dev).contiguous() if rgb else None
    m = masks.to(torch.float32).contiguous()
    bx = boxes.to(device=dev, dtype=torch.long).contiguous()
    out = _empty((N, 3, IMG, IMG), m) if rgb else None
    om = _empty((N, IMG, IMG), m) if mask else None
    for i0 in range(0, N, 65535):
        n = min(65535, N - i0)
        _lib.call("sam6d_dino_crop_proposals", img.data_ptr() if rgb else None, _p(m, i0 * H * Wd), bx.data_ptr() + 32 * i0, n, H, Wd,
                  _p(out, i0 * 3 * IMG * IMG) if rgb else None, _p(om, i0 * IMG * IMG) if mask else None, _s())
    return out, om


@on_tensor_device
def encode(images, W, options=None):
    """images (N, 3, 224, 224) -> (x_norm_clstoken (N, 1024), x_norm_patchtokens (N, 256, 1024)), in slices of SLICE images."""
    ENC.require_mode()
    check_images(images)
    images = images.contiguous()
    N = images.shape[0]
    cls = _empty((N, D), images)
    tok = _empty((N, NP, D), images)
    if N == 0:
        return cls, tok
    S = min(SLICE, N)
    X = _empty((S * NT, D), images)
    Y = _empty((S * NT, D), images)
    T = _empty((S * NT, HID), images)
    A = _empty((S * NP, KPAD), images)
    for i0 in range(0, N, S):
        B = min(S, N - i0)
        ENC.embed(images[i0:i0 + B], W, X, A)
        for blk in W.blocks:
            ENC.block(X, blk, B, Y, T)
        ENC.ln(X, W.norm, cls, B, 1, D, NT * D, D, D, y_off=i0 * D)
        ENC.ln(X, W.norm, tok, B, NP, D, NT * D, D, NP * D, x_off=D, y_off=i0 * NP * D)
    return cls, tok


@on_tensor_device
def descriptors(images, masks224, W, patch_size=PATCH, validpatch_thresh=0.5, options=None):
    """compute_cls_and_patch_features (ISM/model/dinov2.py:308-326): images (N, 3, 224, 224), masks224 (N, 224, 224) ->
    (cls (N, 1024), masked, L2-normalised patch descriptors (N, 256, 1024))."""
    cls, tok = encode(images, W)
    if tok.shape[0] == 0:
        return cls, tok
    return cls, masked_patch_features(tok, masks224, patch_size, validpatch_thresh)


# embed(images, W), layernorm(x, gamma, beta), attention(qkv, B), block(x, W, i) with n <= MAXN tokens: single stages, for the tests
embed, layernorm, attention, block = encoder.pieces(ENC, check_images)
