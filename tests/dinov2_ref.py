"""The project's own restatement of ISM's descriptor path in plain torch, in whatever dtype the state dict and inputs have: the
DINOv2 forward on a state dict (ISM/model/vision_transformer.py:179-266, ISM/model/layers) and CropResizePad as an explicit gather
(ISM/utils/bbox_utils.py:89-126).  tests/test_dinov2_host.py pins both against fixtures captured from the reference; the GPU tests use
them in float64."""
import math

import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------------ DINOv2 forward
def interpolate_pos(pos_embed, grid, offset=0.1):
    """vision_transformer.py:179-207: float32 bicubic to grid x grid with scale_factor (grid + offset) / sqrt(N); cast back."""
    prev = pos_embed.dtype
    n = pos_embed.shape[1] - 1
    if n == grid * grid:
        return pos_embed
    pe = pos_embed.float()
    dim = pe.shape[-1]
    side = int(math.sqrt(n))
    s = float(grid + offset) / math.sqrt(n)
    pp = F.interpolate(pe[:, 1:].reshape(1, side, side, dim).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic", antialias=False)
    assert tuple(pp.shape[-2:]) == (grid, grid)
    return torch.cat((pe[:, :1], pp.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1).to(prev)


def layernorm(x, w, b, eps=1e-6):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def embed(sd, images, patch=14):
    """[cls_token; patch_embed(images)] + interpolated pos_embed: (B, 1 + (S / patch)^2, dim)."""
    B, _, S, _ = images.shape
    g = S // patch
    w = sd["patch_embed.proj.weight"]
    dim = w.shape[0]
    rows = images.reshape(B, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * patch * patch)
    x = rows @ w.reshape(dim, -1).t() + sd["patch_embed.proj.bias"]
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    return x + interpolate_pos(sd["pos_embed"], g).to(x.dtype)


def attention(qkv, heads):
    """qkv (B, n, 3 dim) -> (B, n, dim): softmax(q k^T / sqrt(head_dim)) v per head (layers/attention.py:49-62, before proj)."""
    B, n, c3 = qkv.shape
    dim = c3 // 3
    q, k, v = qkv.reshape(B, n, 3, heads, dim // heads).permute(2, 0, 3, 1, 4)
    a = ((q * (dim // heads) ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, n, dim)


def block(sd, i, x, heads):
    """layers/block.py:82-98 with LayerScale (layers/layer_scale.py:27-28), unfolded."""
    p = "blocks.%d." % i
    y = layernorm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    y = attention(y @ sd[p + "attn.qkv.weight"].t() + sd[p + "attn.qkv.bias"], heads)
    y = y @ sd[p + "attn.proj.weight"].t() + sd[p + "attn.proj.bias"]
    x = x + y * sd[p + "ls1.gamma"]
    y = layernorm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    y = gelu(y @ sd[p + "mlp.fc1.weight"].t() + sd[p + "mlp.fc1.bias"])
    y = y @ sd[p + "mlp.fc2.weight"].t() + sd[p + "mlp.fc2.bias"]
    return x + y * sd[p + "ls2.gamma"]


def depth_of(sd):
    d = 0
    while ("blocks.%d.attn.qkv.weight" % d) in sd:
        d += 1
    return d


def forward(sd, images, heads, patch=14):
    """-> (x_norm_clstoken (B, dim), x_norm_patchtokens (B, P, dim))."""
    x = embed(sd, images, patch)
    for i in range(depth_of(sd)):
        x = block(sd, i, x, heads)
    x = layernorm(x, sd["norm.weight"], sd["norm.bias"])
    return x[:, 0], x[:, 1:]


def to_dtype(sd, dtype, device=None):
    return {k: v.detach().to(dtype=dtype, device=device) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------ CropResizePad
def _nearest_src(out, scale, size):
    """Source indices of F.interpolate's nearest mode when it is given a scale factor: min(floor(dst * fl32(1 / scale)), size - 1),
    the product in float32."""
    inv = torch.tensor(1.0 / scale, dtype=torch.float32)
    idx = torch.floor(torch.arange(out, dtype=torch.float32) * inv).to(torch.long)
    return torch.clamp(idx, max=size - 1)


def crop_resize_pad(images, boxes, target=224):
    """images (N, C, H, W), boxes (N, 4) integer xyxy (exclusive ends) -> (N, C, target, target): bbox_utils.py:89-126 as a gather.
    Per image: index maps of the second resize, the padding and the first resize are composed; padding reads as zero."""
    N, C, H, W = images.shape
    out = torch.zeros((N, C, target, target), dtype=images.dtype, device=images.device)
    b = boxes.to("cpu", torch.long)
    sizes = b[:, 2:] - b[:, :2]
    sf32 = (target / torch.max(sizes, dim=-1)[0])  # float32, as the reference forms it
    for i in range(N):
        x1, y1, x2, y2 = (int(v) for v in b[i])
        x1, x2 = min(max(x1, 0), W), min(max(x2, 0), W)
        y1, y2 = min(max(y1, 0), H), min(max(y2, 0), H)
        cw, ch = x2 - x1, y2 - y1
        s = float(sf32[i])  # the fp32 value as a double
        rw, rh = math.floor(cw * s), math.floor(ch * s)
        if rw <= 0 or rh <= 0:
            raise ValueError("box %d gives an empty resized crop" % i)
        sx = x1 + _nearest_src(rw, s, cw)  # resized column -> image column
        sy = y1 + _nearest_src(rh, s, ch)
        if rw == rh:
            side, top, left = rw, 0, 0
        else:
            side = target
            top, left = max((target - rh) // 2, 0), max((target - rw) // 2, 0)
        if side == target:
            py = px = torch.arange(target)
        else:
            s2 = target / side
            assert math.floor(side * s2) == target
            py = px = _nearest_src(target, s2, side)
        ry, rx = py - top, px - left  # final pixel -> resized-crop pixel
        vy, vx = (ry >= 0) & (ry < rh), (rx >= 0) & (rx < rw)
        yy = sy[ry.clamp(0, rh - 1)].to(images.device)
        xx = sx[rx.clamp(0, rw - 1)].to(images.device)
        g = images[i][:, yy][:, :, xx]
        valid = (vy[:, None] & vx[None, :]).to(images.device)
        out[i] = torch.where(valid, g, torch.zeros((), dtype=images.dtype, device=images.device))
    return out


def rgb_normalize(image_u8):
    """ToTensor + Normalize (ISM/model/dinov2.py:144-149): (H, W, 3) uint8 tensor -> (3, H, W) float32."""
    x = image_u8.permute(2, 0, 1).to(torch.float32).div(255)
    mean = torch.tensor(MEAN, dtype=torch.float32, device=x.device)[:, None, None]
    std = torch.tensor(STD, dtype=torch.float32, device=x.device)[:, None, None]
    return (x - mean) / std


def process_rgb_proposals(image_u8, masks, boxes):
    """ISM/model/dinov2.py:160-173: masks (N, H, W) float."""
    rgb = rgb_normalize(image_u8).to(masks.device)
    return crop_resize_pad(rgb.unsqueeze(0) * masks.float().unsqueeze(1), boxes)


def process_masks_proposals(masks, boxes):
    """ISM/model/dinov2.py:221-232 -> (N, 224, 224)."""
    return crop_resize_pad(masks.float().unsqueeze(1), boxes)[:, 0]


def masked_patch_features(tokens, masks224, patch=14, thresh=0.5):
    """ISM/model/dinov2.py:322-324 -> (kept (N, P) bool, normalised masked tokens)."""
    keep = F.avg_pool2d(masks224.unsqueeze(1).to(tokens.dtype), patch).flatten(1) > thresh
    return keep, F.normalize(tokens * keep.unsqueeze(-1), dim=-1)
