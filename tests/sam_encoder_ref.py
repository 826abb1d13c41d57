"""SAM's image encoder restated in float64-capable plain torch (ISM/segment_anything/modeling/image_encoder.py, whole file; LayerNorm2d
common.py:38-43): padded windows, both forms of the decomposed relative-position bias, the neck.  Written per window and per head, with
explicit bias tensors, independently of sam6d_hip.samenc; tests/test_sam_encoder_host.py pins it to the reference's own ImageEncoderViT
run in .double() (tests/golden/sam_encoder_small.npz).  Also the seeded weights and inputs the tests share."""
import math

import torch
import torch.nn.functional as F


def to_dtype(sd, dtype, device=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def seeded_weights(seed, dim=1280, heads=16, depth=2, global_blocks=(1,), grid=64, window=14, patch=16, out=256, mlp_ratio=4):
    """A float32 state dict with ImageEncoderViT's names.  rel_pos_h / _w and pos_embed are random (the reference initialises them to
    zero, which would hide every rel-pos error); norms are 1 + 0.1 noise; Linear weights have unit gain."""
    g = torch.Generator().manual_seed(seed)
    hd = dim // heads

    def rn(*shape, scale=1.0):
        return scale * torch.randn(shape, generator=g)

    def lin(p, n_out, n_in, sd):
        sd[p + ".weight"] = rn(n_out, n_in, scale=n_in ** -0.5)
        sd[p + ".bias"] = rn(n_out, scale=0.2)

    def norm(p, n, sd):
        sd[p + ".weight"] = 1.0 + rn(n, scale=0.1)
        sd[p + ".bias"] = rn(n, scale=0.1)

    sd = {"pos_embed": rn(1, grid, grid, dim, scale=0.5),
          "patch_embed.proj.weight": rn(dim, 3, patch, patch, scale=(3 * patch * patch) ** -0.5),
          "patch_embed.proj.bias": rn(dim, scale=0.2)}
    for i in range(depth):
        b = "blocks.%d." % i
        side = grid if i in global_blocks else window
        norm(b + "norm1", dim, sd)
        sd[b + "attn.rel_pos_h"] = rn(2 * side - 1, hd, scale=0.1)
        sd[b + "attn.rel_pos_w"] = rn(2 * side - 1, hd, scale=0.1)
        lin(b + "attn.qkv", 3 * dim, dim, sd)
        lin(b + "attn.proj", dim, dim, sd)
        norm(b + "norm2", dim, sd)
        lin(b + "mlp.lin1", mlp_ratio * dim, dim, sd)
        lin(b + "mlp.lin2", dim, mlp_ratio * dim, sd)
    sd["neck.0.weight"] = rn(out, dim, 1, 1, scale=dim ** -0.5)
    norm("neck.1", out, sd)
    sd["neck.2.weight"] = rn(out, out, 3, 3, scale=(9 * out) ** -0.5)
    norm("neck.3", out, sd)
    return sd


def seeded_input(seed, size, batch=1):
    """(batch, 3, size, size) float32: what sam.preprocess leaves (normalised pixels: unit scale)."""
    return torch.randn((batch, 3, size, size), generator=torch.Generator().manual_seed(seed))


def windows_of(sd, window=14):
    """Per block: 0 for a global block (rel_pos_h has 2 grid - 1 rows), else `window`."""
    grid = sd["pos_embed"].shape[1]
    out, i = [], 0
    while ("blocks.%d.attn.rel_pos_h" % i) in sd:
        out.append(0 if sd["blocks.%d.attn.rel_pos_h" % i].shape[0] == 2 * grid - 1 else window)
        i += 1
    return out


def rel_bias(q, rel, side, axis):
    """q (side, side, hd) of one window and head -> (side, side, side): [qh, qw, k] = q[qh, qw] . rel[q_axis - k + side - 1], q_axis the
    query's coordinate along `axis` (0: rows, 1: columns).  get_rel_pos without interpolation + the einsum of add_decomposed_rel_pos."""
    assert rel.shape[0] == 2 * side - 1
    c = torch.arange(side, device=q.device)
    R = rel[c[:, None] - c[None, :] + side - 1]                          # (q coordinate, k coordinate, hd)
    return torch.einsum("hwc,hkc->hwk", q, R) if axis == 0 else torch.einsum("hwc,wkc->hwk", q, R)


def attention_one(qkv, rel_h, rel_w, heads):
    """One window (or whole image): qkv (S, S, 3 D) -> (S, S, D).  Attention.forward between qkv and proj."""
    S, Dm = qkv.shape[0], qkv.shape[2] // 3
    hd = Dm // heads
    out = torch.empty((S, S, Dm), dtype=qkv.dtype, device=qkv.device)
    for h in range(heads):
        q, k, v = (qkv[:, :, i * Dm + h * hd:i * Dm + (h + 1) * hd] for i in range(3))
        s = (q.reshape(S * S, hd) * hd ** -0.5) @ k.reshape(S * S, hd).t()
        s = s.view(S, S, S, S) + rel_bias(q, rel_h, S, 0)[:, :, :, None] + rel_bias(q, rel_w, S, 1)[:, :, None, :]
        out[:, :, h * hd:(h + 1) * hd] = (torch.softmax(s.view(S * S, S * S), dim=-1) @ v.reshape(S * S, hd)).view(S, S, hd)
    return out


def attention(qkv, pad_row, rel_h, rel_w, heads, win):
    """qkv (B, G, G, 3 D) of whole images -> (B, G, G, D).  win > 0: the grid is padded to a multiple of win with `pad_row` (3 D: what
    the qkv Linear makes of a zero token, its bias), cut into windows, and the padding dropped again; win = 0: one window."""
    B, G = qkv.shape[0], qkv.shape[1]
    if win == 0:
        return torch.stack([attention_one(qkv[b], rel_h, rel_w, heads) for b in range(B)])
    Gp = win * math.ceil(G / win)
    padded = pad_row.view(1, 1, 1, -1).expand(B, Gp, Gp, -1).clone()
    padded[:, :G, :G] = qkv
    out = torch.empty((B, Gp, Gp, qkv.shape[3] // 3), dtype=qkv.dtype, device=qkv.device)
    for b in range(B):
        for y in range(0, Gp, win):
            for x in range(0, Gp, win):
                out[b, y:y + win, x:x + win] = attention_one(padded[b, y:y + win, x:x + win], rel_h, rel_w, heads)
    return out[:, :G, :G]


def layer_norm(x, w, b, eps):
    u = x.mean(-1, keepdim=True)
    s = ((x - u) ** 2).mean(-1, keepdim=True)
    return (x - u) / torch.sqrt(s + eps) * w + b


def block(sd, p, x, heads, win, eps=1e-6):
    """Block.forward: x (B, G, G, D).  The reference pads the normalised tokens with zeros; their qkv rows are the qkv bias."""
    qkv = F.linear(layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps), sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    a = attention(qkv, sd[p + "attn.qkv.bias"], sd[p + "attn.rel_pos_h"], sd[p + "attn.rel_pos_w"], heads, win)
    x = x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    h = F.linear(layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps), sd[p + "mlp.lin1.weight"], sd[p + "mlp.lin1.bias"])
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return x + F.linear(h, sd[p + "mlp.lin2.weight"], sd[p + "mlp.lin2.bias"])


def neck(sd, x):
    """x (B, G, G, D) -> (B, out, G, G): 1 x 1 conv, LayerNorm2d, 3 x 3 conv with padding 1, LayerNorm2d (channel-last until the end)."""
    B, G = x.shape[0], x.shape[1]
    y = layer_norm(x @ sd["neck.0.weight"][:, :, 0, 0].t(), sd["neck.1.weight"], sd["neck.1.bias"], 1e-6)
    yp = F.pad(y, (0, 0, 1, 1, 1, 1))
    z = sum(yp[:, ky:ky + G, kx:kx + G] @ sd["neck.2.weight"][:, :, ky, kx].t() for ky in range(3) for kx in range(3))
    return layer_norm(z, sd["neck.3.weight"], sd["neck.3.bias"], 1e-6).permute(0, 3, 1, 2)


def embed(sd, x):
    """x (B, 3, S, S) -> (B, G, G, D): PatchEmbed + pos_embed."""
    w = sd["patch_embed.proj.weight"]
    Dm, p = w.shape[0], w.shape[-1]
    B, G = x.shape[0], x.shape[-1] // p
    rows = x.reshape(B, 3, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(B, G, G, 3 * p * p)
    return rows @ w.reshape(Dm, -1).t() + sd["patch_embed.proj.bias"] + sd["pos_embed"]


def forward(sd, x, heads, windows, eps=1e-6):
    """ImageEncoderViT.forward in sd's dtype: x (B, 3, S, S) -> (B, out, G, G)."""
    x = embed(sd, x.to(sd["pos_embed"].dtype))
    for i, win in enumerate(windows):
        x = block(sd, "blocks.%d." % i, x, heads, win, eps)
    return neck(sd, x)
