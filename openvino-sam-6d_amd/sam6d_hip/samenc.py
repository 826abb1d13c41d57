"""SAM's ViT-H image encoder on the library: the preprocessed (B, 3, 1024, 1024) tensor `sam.image_encoder` is called on -> the
(B, 256, 64, 64) image embedding (ISM/segment_anything/modeling/image_encoder.py, whole file; LayerNorm2d common.py:38-43).

The blocks run encoder.py's launch sequence (LN -> qkv GEMM -> attention -> proj GEMM + residual -> LN -> fc1 GEMM + GELU -> fc2 GEMM +
residual) on the residual stream X (B*4096, 1280), image row order, no cls row; 4096 rows per image are a multiple of the GEMM's 128-row
tile, so every block GEMM takes the whole-tile route.  What is this encoder's own is the attention with decomposed relative-position
bias (csrc/samenc.hip): windowed blocks never form the (B*25, 14, 14, C) partition -- the kernel indexes the windows, and a padded
position is a key whose k and v are the qkv bias (the reference pads after norm1, so the padded token is zero) -- and global blocks run
an online softmax over the 4096 keys.  The neck: 1 x 1 conv as a GEMM, LayerNorm2d as a 256-wide row LayerNorm on channel-last rows,
the 3 x 3 conv as a gather of the nine shifted rows + one GEMM, LayerNorm2d again, one transpose to (B, 256, 64, 64).

One configuration: SAM ViT-H (CONFIG); depth and which blocks are global are data.  Anything else raises NotImplementedError naming the
value (`check`), matmul mode 2 raises too.  `eager` is the same function in plain torch ops on any device and dtype, written after the
reference (any geometry: the tests pin it at a small one); `restructured` runs the library-shaped sequence (index-based windows, pad
rows, T_h / T_w indexing, gathered 3 x 3) in plain torch, which is how the restructuring is checked in float64 on the host.
"""
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _lib, encoder
from .runtime import Linear, _empty, _p, _s, gemm, gemm_route, library_call

CONFIG = dict(embed_dim=1280, num_heads=16, mlp_dim=5120, patch_size=16, grid=64, window_size=14, out_chans=256, eps=1e-6)
D, HEADS, HD, HID, PATCH, GRID, WIN, OUT, EPS = 1280, 16, 80, 5120, 16, 64, 14, 256, 1e-6
NP = GRID * GRID
IMG = PATCH * GRID
K = 3 * PATCH * PATCH
SLICE = 4  # images per pass (X, Y, T and the patch rows of a slice: 0.5 GB)


class Geometry(NamedTuple):
    """What a state dict (and, where it says nothing, the module or the caller) fixes about an encoder."""
    embed_dim: int
    num_heads: int
    mlp_dim: int
    patch_size: int
    grid: int
    out_chans: int
    depth: int
    windows: tuple   # per block: the window size, 0 for a global block
    eps: float


def _sd(m):
    return m.state_dict() if hasattr(m, "state_dict") else m


def _ref_key(k):
    """encoder.pack_block's names for the MLP (fc1, fc2) in the reference's MLPBlock (lin1, lin2; common.py:13-28)."""
    return k.replace("mlp.fc1.", "mlp.lin1.").replace("mlp.fc2.", "mlp.lin2.")


def geometry(image_encoder, window_size=None, global_attn_indexes=None, eps=None):
    """The Geometry of an ImageEncoderViT module or of its state dict.  A module says its own window sizes and LayerNorm eps; for a state
    dict they are arguments (defaults: the blocks whose rel_pos_h has 2 * grid - 1 rows are global, the others have windows of
    CONFIG's size; eps 1e-6)."""
    sd = _sd(image_encoder)
    for key, what in (("pos_embed", "use_abs_pos"), ("blocks.0.attn.rel_pos_h", "use_rel_pos")):
        if key not in sd:
            raise NotImplementedError("sam6d_hip.samenc: %s = False is not implemented (no %s in the state dict)" % (what, key))
    depth = 0
    while ("blocks.%d.attn.qkv.weight" % depth) in sd:
        depth += 1
    dim, grid = int(sd["pos_embed"].shape[-1]), int(sd["pos_embed"].shape[1])
    blocks = getattr(image_encoder, "blocks", None)
    if blocks is not None and hasattr(blocks, "__getitem__") and hasattr(blocks[0], "window_size"):
        windows = tuple(int(b.window_size) for b in blocks)
        heads = int(blocks[0].attn.num_heads)
        if eps is None:
            eps = float(blocks[0].norm1.eps)
    else:
        if global_attn_indexes is None:
            global_attn_indexes = [i for i in range(depth) if int(sd["blocks.%d.attn.rel_pos_h" % i].shape[0]) == 2 * grid - 1]
        ws = CONFIG["window_size"] if window_size is None else int(window_size)
        windows = tuple(0 if i in tuple(global_attn_indexes) else ws for i in range(depth))
        heads = dim // int(sd["blocks.0.attn.rel_pos_h"].shape[1])
    return Geometry(dim, heads, int(sd["blocks.0.mlp.lin1.weight"].shape[0]), int(sd["patch_embed.proj.weight"].shape[-1]), grid,
                    int(sd["neck.0.weight"].shape[0]), depth, windows, CONFIG["eps"] if eps is None else float(eps))


def check(image_encoder, window_size=None, global_attn_indexes=None, eps=None):
    """Raises NotImplementedError, naming the value, for anything but the configuration the kernels are built for; returns the Geometry."""
    g = geometry(image_encoder, window_size, global_attn_indexes, eps)
    _check(g, _sd(image_encoder))
    return g


def _check(g, sd):
    def refuse(what, got, want):
        raise NotImplementedError("sam6d_hip.samenc: %s = %s is not implemented (the kernels are built for %s)" % (what, got, want))
    for name in ("embed_dim", "num_heads", "mlp_dim", "patch_size", "out_chans"):
        if getattr(g, name) != CONFIG[name]:
            refuse(name, getattr(g, name), CONFIG[name])
    if g.grid != CONFIG["grid"]:
        refuse("img_size", g.grid * g.patch_size, CONFIG["grid"] * CONFIG["patch_size"])
    if tuple(sd["patch_embed.proj.weight"].shape) != (D, 3, PATCH, PATCH):
        refuse("patch_embed.proj.weight shape", tuple(sd["patch_embed.proj.weight"].shape), (D, 3, PATCH, PATCH))
    if "blocks.0.attn.qkv.bias" not in sd:  # (the windowed kernel's padding row is that bias)
        refuse("qkv_bias", False, True)
    if abs(g.eps - CONFIG["eps"]) > 1e-12:
        refuse("LayerNorm eps", g.eps, CONFIG["eps"])
    for i, w in enumerate(g.windows):
        if w not in (0, CONFIG["window_size"]):
            refuse("window_size", w, "%d, or 0 for a global block" % CONFIG["window_size"])
        side = w if w else g.grid
        for name in ("rel_pos_h", "rel_pos_w"):
            shape = tuple(sd["blocks.%d.attn.%s" % (i, name)].shape)
            if shape != (2 * side - 1, HD):  # (another length is get_rel_pos's interpolating branch)
                refuse("blocks.%d.attn.%s shape" % (i, name), shape, "%s for a block of side %d" % ((2 * side - 1, HD), side))
    if tuple(sd["neck.2.weight"].shape) != (OUT, OUT, 3, 3) or "neck.0.bias" in sd or "neck.2.bias" in sd:
        refuse("neck", tuple(sd["neck.2.weight"].shape), "bias-free 1 x 1 and 3 x 3 convolutions to %d channels" % OUT)


class _SamEncoder(encoder.Encoder):
    """encoder.Encoder whose attention launch depends on the block: windowed or global, each with the block's rel-pos tables."""
    __slots__ = ()

    def attend(self, T, Y, B, n, blk):
        heads = blk["qkv"].w.shape[0] // (3 * HD)
        if blk["window"]:
            _lib.call(self.attention, _p(T), _p(blk["qkv"].b), _p(blk["rel_h"]), _p(blk["rel_w"]), _p(Y), B, heads, _s())
        else:
            _lib.call("sam6d_sam_global_attention", _p(T), _p(blk["rel_h"]), _p(blk["rel_w"]), _p(Y), B, heads, _s())


ENC = _SamEncoder("sam6d_hip.samenc", "SAM image encoder", D, HID, 0, NP, NP, K, EPS, "sam6d_sam_patch_rows", "sam6d_sam_layernorm1280",
                  "sam6d_sam_window_attention", False, True)


class SamEncoderWeights(encoder.Weights):
    """An ImageEncoderViT (module, or state dict with window_size / global_attn_indexes / eps where they differ from the defaults of
    `geometry`) on `dev` in `dtype`.  float32 on a HIP device: checked against CONFIG and packed once for the library -- the patch
    conv as a (1280, 768) matrix, qkv / proj / fc1 / fc2 of every block and the neck's two convolutions as Linear objects with their
    fp16 halves cut (Weights.cut_w16), rel-pos tables, norms, pos_embed.  Otherwise (CPU, float64, or pack=False): the tensors alone,
    for `eager` and `restructured`."""

    def __init__(self, image_encoder, dev, dtype=torch.float32, options=None, window_size=None, global_attn_indexes=None, eps=None,
                 pack=True):
        self.dev, self.dtype, self.options = torch.device(dev), dtype, options
        self.geom = geometry(image_encoder, window_size, global_attn_indexes, eps)
        self.sd = {k: v.detach().to(self.dev, dtype).contiguous() for k, v in _sd(image_encoder).items()}
        self.blocks = None
        if pack and self.dev.type == "cuda" and dtype == torch.float32:
            _check(self.geom, self.sd)
            with encoder.device_of(self.dev):
                self._pack()

    def _pack(self):
        sd = self.sd
        g = lambda k: sd[_ref_key(k)]  # noqa: E731
        self.patch = Linear(g("patch_embed.proj.weight").reshape(D, K), g("patch_embed.proj.bias"))
        self.pos = g("pos_embed").reshape(NP * D)
        self.blocks = []
        for i, w in enumerate(self.geom.windows):
            blk = encoder.pack_block(g, "blocks.%d." % i)
            blk.update(rel_h=g("blocks.%d.attn.rel_pos_h" % i), rel_w=g("blocks.%d.attn.rel_pos_w" % i), window=bool(w))
            self.blocks.append(blk)
        self.neck1 = Linear(g("neck.0.weight").reshape(OUT, D), None)
        self.neck2 = Linear(g("neck.2.weight").permute(0, 2, 3, 1).reshape(OUT, 9 * OUT), None)  # column 256 (3 ky + kx) + c
        self.norms = ((g("neck.1.weight"), g("neck.1.bias")), (g("neck.3.weight"), g("neck.3.bias")))
        self.cut_w16()

    def linears(self):
        yield from super().linears()
        yield from (self.neck1, self.neck2)

    def require_library(self):
        if self.blocks is None:
            raise RuntimeError("sam6d_hip.samenc: the library path needs float32 weights on a HIP device (this build has no CPU path)")


def pack_block(sd, dev):
    """One block's weights from a state dict with unprefixed keys (norm1.weight, attn.qkv.weight, attn.rel_pos_h ...) for `pieces`:
    windowed when its rel_pos_h has 27 rows."""
    g = lambda k: sd[_ref_key(k)].detach().to(dev, torch.float32).contiguous()  # noqa: E731
    blk = encoder.pack_block(g, "")
    blk.update(rel_h=g("attn.rel_pos_h"), rel_w=g("attn.rel_pos_w"), window=int(sd["attn.rel_pos_h"].shape[0]) == 2 * WIN - 1)
    return blk


def check_images(x):
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, IMG, IMG):
        raise ValueError("sam6d_hip.samenc: the input must be (B, 3, %d, %d), got %s" % (IMG, IMG, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise ValueError("sam6d_hip.samenc: the input must be float32, got %s" % x.dtype)


# ------------------------------------------------------------------------------------------------- eager: the reference's sequence
def _rel_index(side, device):
    """get_rel_pos's index for q_size == k_size == side and a table of 2 side - 1 rows (image_encoder.py:317-322): (side, side)."""
    c = torch.arange(side, device=device)
    return c[:, None] - c[None, :] + (side - 1)


def _eager_attention(sd, p, x, heads):
    """Attention.forward (image_encoder.py:224-240) with add_decomposed_rel_pos (:325-361): x (B, H, W, C)."""
    B, H, W, C = x.shape
    qkv = F.linear(x, sd[p + "qkv.weight"], sd[p + "qkv.bias"]).reshape(B, H * W, 3, heads, -1).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.reshape(3, B * heads, H * W, -1).unbind(0)
    attn = (q * (q.shape[-1] ** -0.5)) @ k.transpose(-2, -1)
    rh, rw = sd[p + "rel_pos_h"], sd[p + "rel_pos_w"]
    if rh.shape[0] != 2 * H - 1 or rw.shape[0] != 2 * W - 1:
        raise NotImplementedError("sam6d_hip.samenc: %srel_pos_h / _w of %d / %d rows for a %d x %d block (get_rel_pos would interpolate)"
                                  % (p, rh.shape[0], rw.shape[0], H, W))
    Rh, Rw = rh[_rel_index(H, x.device)], rw[_rel_index(W, x.device)]
    r_q = q.reshape(B * heads, H, W, -1)
    rel_h = torch.einsum("bhwc,hkc->bhwk", r_q, Rh)
    rel_w = torch.einsum("bhwc,wkc->bhwk", r_q, Rw)
    attn = (attn.view(B * heads, H, W, H, W) + rel_h[:, :, :, :, None] + rel_w[:, :, :, None, :]).view(B * heads, H * W, H * W)
    attn = attn.softmax(dim=-1)
    x = (attn @ v).view(B, heads, H, W, -1).permute(0, 2, 3, 1, 4).reshape(B, H, W, -1)
    return F.linear(x, sd[p + "proj.weight"], sd[p + "proj.bias"])


def _eager_block(sd, p, x, heads, win, eps):
    """Block.forward (image_encoder.py:166-182) with window_partition / window_unpartition (:243-289)."""
    shortcut = x
    x = F.layer_norm(x, (x.shape[-1],), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    if win > 0:
        B, H, W, C = x.shape
        ph, pw = (win - H % win) % win, (win - W % win) % win
        x = F.pad(x, (0, 0, 0, pw, 0, ph))
        Hp, Wp = H + ph, W + pw
        x = x.view(B, Hp // win, win, Wp // win, win, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, win, win, C)
    x = _eager_attention(sd, p + "attn.", x, heads)
    if win > 0:
        x = x.view(B, Hp // win, Wp // win, win, win, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, -1)[:, :H, :W, :]
    x = shortcut + x
    h = F.layer_norm(x, (x.shape[-1],), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return x + F.linear(F.gelu(F.linear(h, sd[p + "mlp.lin1.weight"], sd[p + "mlp.lin1.bias"])), sd[p + "mlp.lin2.weight"], sd[p + "mlp.lin2.bias"])


def _ln2d(x, w, b, eps=1e-6):
    """LayerNorm2d (common.py:38-43)."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


def eager(x, W):
    """ImageEncoderViT.forward (image_encoder.py:106-116) op for op in W's dtype on W's device: x (B, 3, S, S) -> (B, out, S/p, S/p)."""
    sd, g = W.sd, W.geom
    x = F.conv2d(x.to(W.dev, W.dtype), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=g.patch_size).permute(0, 2, 3, 1)
    x = x + sd["pos_embed"]
    for i, win in enumerate(g.windows):
        x = _eager_block(sd, "blocks.%d." % i, x, g.num_heads, win, g.eps)
    x = _ln2d(F.conv2d(x.permute(0, 3, 1, 2), sd["neck.0.weight"]), sd["neck.1.weight"], sd["neck.1.bias"])
    return _ln2d(F.conv2d(x, sd["neck.2.weight"], padding=1), sd["neck.3.weight"], sd["neck.3.bias"])


# ------------------------------------------------------------------------------------------------- the library-shaped sequence in torch
def window_rows(grid, win, device):
    """(windows, win * win) row numbers of the window positions in an image's (grid * grid) rows; `grid * grid` stands for the padding
    row.  win = grid: one window, no padding (a global block)."""
    nw = -(-grid // win)
    j = torch.arange(win, device=device)
    y = (torch.arange(nw, device=device)[:, None] * win + j[None, :])                       # (nw, win)
    yy = y[:, None, :, None].expand(nw, nw, win, win)
    xx = y[None, :, None, :].expand(nw, nw, win, win)
    rows = torch.where((yy < grid) & (xx < grid), yy * grid + xx, torch.full_like(yy, grid * grid))
    return rows.reshape(nw * nw, win * win)


def rel_attention(qkv, pad_qkv, rel_h, rel_w, B, heads, grid, win):
    """What the two attention kernels compute, in plain torch (any dtype): qkv (B * grid^2, 3 * heads * hd) in image row order -> (B *
    grid^2, heads * hd).  Windows are gathered by row number, position `grid^2` being the padding row pad_qkv; the bias is read from
    T_h = q . rel_h^T and T_w = q . rel_w^T (2 win - 1 columns each) at column q position - k position + win - 1, with the unscaled q;
    padded queries are dropped."""
    N, Dm = grid * grid, qkv.shape[1] // 3
    hd = Dm // heads
    rows = window_rows(grid, win, qkv.device)
    allrows = torch.cat([qkv.view(B, N, 3 * Dm), pad_qkv.view(1, 1, 3 * Dm).expand(B, 1, 3 * Dm)], dim=1)
    out = qkv.new_zeros((B, N + 1, Dm))
    ri = _rel_index(win, qkv.device)                                   # (win, win)
    ih = ri[:, None, :, None].expand(win, win, win, win).reshape(win * win, win * win)   # [q, k] -> qh - kh + win - 1
    iw = ri[None, :, None, :].expand(win, win, win, win).reshape(win * win, win * win)
    for w in range(rows.shape[0]):
        g = allrows[:, rows[w]].view(B, win * win, 3, heads, hd)
        q, k, v = (g[:, :, i].permute(0, 2, 1, 3) for i in range(3))   # (B, heads, win^2, hd)
        s = (q * (hd ** -0.5)) @ k.transpose(-2, -1)
        th, tw = q @ rel_h.t(), q @ rel_w.t()                          # (B, heads, win^2, 2 win - 1)
        s = s + torch.gather(th, 3, ih.expand(B, heads, -1, -1)) + torch.gather(tw, 3, iw.expand(B, heads, -1, -1))
        o = (s.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, win * win, Dm)
        out[:, rows[w]] = o                                            # (padded queries all land in the spare row N)
    return out[:, :N].reshape(B * N, Dm)


def neck_gather(x, B, grid):
    """x (B * grid^2, C) channel-last -> (B * grid^2, 9 C): columns C (3 ky + kx) + c = x at (y + ky - 1, x + kx - 1), zeros outside."""
    C = x.shape[1]
    m = F.pad(x.view(B, grid, grid, C), (0, 0, 1, 1, 1, 1))
    return torch.cat([m[:, ky:ky + grid, kx:kx + grid] for ky in range(3) for kx in range(3)], dim=-1).reshape(B * grid * grid, 9 * C)


def restructured(x, W):
    """`eager`'s result through the library-shaped sequence in plain torch, any geometry and dtype."""
    sd, g = W.sd, W.geom
    B, N, Dm = x.shape[0], g.grid * g.grid, g.embed_dim
    p = g.patch_size
    A = x.to(W.dev, W.dtype).reshape(B, 3, g.grid, p, g.grid, p).permute(0, 2, 4, 1, 3, 5).reshape(B * N, 3 * p * p)
    X = (A @ sd["patch_embed.proj.weight"].reshape(Dm, -1).t() + sd["patch_embed.proj.bias"]).view(B, N, Dm) + sd["pos_embed"].reshape(1, N, Dm)
    X = X.reshape(B * N, Dm)
    for i, win in enumerate(g.windows):
        b = "blocks.%d." % i
        Y = F.layer_norm(X, (Dm,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], g.eps)
        T = F.linear(Y, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"])
        Y = rel_attention(T, sd[b + "attn.qkv.bias"], sd[b + "attn.rel_pos_h"], sd[b + "attn.rel_pos_w"], B, g.num_heads, g.grid, win or g.grid)
        X = X + F.linear(Y, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        Y = F.layer_norm(X, (Dm,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], g.eps)
        X = X + F.linear(F.gelu(F.linear(Y, sd[b + "mlp.lin1.weight"], sd[b + "mlp.lin1.bias"])), sd[b + "mlp.lin2.weight"], sd[b + "mlp.lin2.bias"])
    C = g.out_chans
    Y = F.layer_norm(X @ sd["neck.0.weight"].reshape(C, Dm).t(), (C,), sd["neck.1.weight"], sd["neck.1.bias"], 1e-6)
    Y = neck_gather(Y, B, g.grid) @ sd["neck.2.weight"].permute(0, 2, 3, 1).reshape(C, 9 * C).t()
    Y = F.layer_norm(Y, (C,), sd["neck.3.weight"], sd["neck.3.bias"], 1e-6)
    return Y.view(B, g.grid, g.grid, C).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------- the library
_entry = library_call(ENC.name, ENC.role)


def _neck(X, W, B, Y, T, out, o_off):
    """X (B*4096, 1280) -> out[o_off:] as (B, 256, 64, 64); Y (>= B*4096*256 floats) and T (>= B*4096*2560) are workspaces."""
    M = B * NP
    gemm(X, W.neck1.w, None, Y, M, OUT, D, D, D, OUT, w16=W.neck1.w16())
    _lib.call("sam6d_layernorm256", _p(Y), _p(W.norms[0][0]), _p(W.norms[0][1]), _p(T), M, OUT, OUT, 1e-6, _s())
    _lib.call("sam6d_sam_neck_gather", _p(T), _p(T, M * OUT), B, _s())
    gemm(T, W.neck2.w, None, Y, M, OUT, 9 * OUT, 9 * OUT, 9 * OUT, OUT, a_off=M * OUT, w16=W.neck2.w16())
    _lib.call("sam6d_layernorm256", _p(Y), _p(W.norms[1][0]), _p(W.norms[1][1]), _p(T), M, OUT, OUT, 1e-6, _s())
    _lib.call("sam6d_transpose", _p(T), OUT, NP * OUT, B, NP, OUT, _p(out, o_off), NP, OUT * NP, _s())


def _encode(W, B, like, embed):
    """The launch sequence behind `encode` and `encode_rows`: embed(i0, b, X) fills X (b*4096, 1280) for images i0 .. i0 + b - 1."""
    out = _empty((B, OUT, GRID, GRID), like)
    if B == 0:
        return out
    S = min(SLICE, B)
    X, Y, T = (_empty((S * NP, c), like) for c in (D, D, HID))
    for i0 in range(0, B, S):
        b = min(S, B - i0)
        embed(i0, b, X)
        for blk in W.blocks:
            ENC.block(X, blk, b, Y, T)
        _neck(X, W, b, Y, T, out, i0 * OUT * NP)
    return out


@_entry
def encode(x, W):
    """x (B, 3, 1024, 1024) float32 on the HIP device, preprocessed as `sam.image_encoder` expects it -> (B, 256, 64, 64)."""
    W.require_library()
    check_images(x)
    x = x.contiguous()
    A = _empty((min(SLICE, x.shape[0]) * NP, K), x)
    return _encode(W, x.shape[0], x, lambda i0, b, X: ENC.embed(x[i0:i0 + b], W, X, A))


@_entry
def encode_rows(A, W):
    """`encode` from the patch rows: A (B*4096, 768) float32 on the HIP device, row 4096 b + 64 py + px = the patch's values of the
    preprocessed image in (c, kh, kw) order (samfront.preprocess(..., layout="rows"), or sam6d_sam_patch_rows) -> (B, 256, 64, 64).  The
    same launches as `encode` without the patch-rows one."""
    W.require_library()
    if A.dim() != 2 or A.shape[1] != K or A.shape[0] % NP:
        raise ValueError("sam6d_hip.samenc: the patch rows must be (B*%d, %d), got %s" % (NP, K, tuple(A.shape)))
    if A.dtype != torch.float32:
        raise ValueError("sam6d_hip.samenc: the patch rows must be float32, got %s" % A.dtype)
    A = A.contiguous()
    return _encode(W, A.shape[0] // NP, A, lambda i0, b, X: ENC.embed_rows(A[i0 * NP:(i0 + b) * NP], W, X, b))


def block_gemm_routes(W, B=1):
    """The SAM6D_GEMM_ROUTE_* codes of the four GEMMs of a block at B images, in the calling thread's matmul mode (nothing is
    launched): [qkv, proj, fc1, fc2]."""
    W.require_library()
    blk, M = W.blocks[0], B * NP
    a = _empty((16,), blk["qkv"].w)
    return [gemm_route(a, blk[n].w, blk[n].b, a, M, blk[n].w.shape[0], blk[n].w.shape[1], blk[n].w.shape[1], blk[n].w.shape[1],
                       blk[n].w.shape[0], residual=a if n in ("proj", "fc2") else None, ldr=blk[n].w.shape[0] if n in ("proj", "fc2") else 0,
                       act=(2 if n == "fc1" else 0) + (32 if ENC.whole_tiles else 0), w16=blk[n].w16()) for n in ("qkv", "proj", "fc1", "fc2")]


class _Pieces:
    """Single stages behind the public entry-point conventions, for the tests (as encoder.pieces)."""

    @staticmethod
    @_entry
    def window_attention(qkv, pad_qkv, rel_h, rel_w, B):
        """qkv (B*4096, 3*80*heads), pad_qkv (3*80*heads), rel_h / rel_w (27, 80) -> (B*4096, 80*heads)."""
        return _Pieces._attention("sam6d_sam_window_attention", qkv, pad_qkv, rel_h, rel_w, B, 2 * WIN - 1)

    @staticmethod
    @_entry
    def global_attention(qkv, rel_h, rel_w, B):
        """qkv (B*4096, 3*80*heads), rel_h / rel_w (127, 80) -> (B*4096, 80*heads)."""
        return _Pieces._attention("sam6d_sam_global_attention", qkv, None, rel_h, rel_w, B, 2 * GRID - 1)

    @staticmethod
    def _attention(name, qkv, pad_qkv, rel_h, rel_w, B, nrel):
        if qkv.dim() != 2 or B < 1 or qkv.shape[0] != B * NP or qkv.shape[1] % (3 * HD):
            raise ValueError("sam6d_hip.samenc: qkv must be (B*%d, 3*%d*heads), got %s for B = %d" % (NP, HD, tuple(qkv.shape), B))
        heads = qkv.shape[1] // (3 * HD)
        for t, shape in ((rel_h, (nrel, HD)), (rel_w, (nrel, HD))) + (((pad_qkv, (qkv.shape[1],)),) if pad_qkv is not None else ()):
            if tuple(t.shape) != shape or t.dtype != torch.float32:
                raise ValueError("sam6d_hip.samenc: expected a float32 tensor of shape %s, got %s %s" % (shape, tuple(t.shape), t.dtype))
        if qkv.dtype != torch.float32:
            raise ValueError("sam6d_hip.samenc: qkv must be float32, got %s" % qkv.dtype)
        qkv = qkv.contiguous()
        out = _empty((B * NP, heads * HD), qkv)
        args = [_p(qkv)] + ([_p(pad_qkv.contiguous())] if pad_qkv is not None else []) + [_p(rel_h.contiguous()), _p(rel_w.contiguous())]
        _lib.call(name, *args, _p(out), B, heads, _s())
        return out

    @staticmethod
    @_entry
    def block(x, blk):
        """x (B, 4096, 1280) -> one block (a `pack_block` dictionary, or W.blocks[i]) applied to a copy."""
        if x.dim() != 3 or tuple(x.shape[1:]) != (NP, D) or x.dtype != torch.float32:
            raise ValueError("sam6d_hip.samenc: x must be float32 (B, %d, %d), got %s %s" % (NP, D, tuple(x.shape), x.dtype))
        B = x.shape[0]
        X = x.reshape(B * NP, D).contiguous().clone()
        ENC.block(X, blk, B, _empty((B * NP, D), X), _empty((B * NP, HID), X))
        return X.view(B, NP, D)

    @staticmethod
    @_entry
    def neck(x, W):
        """x (B, 4096, 1280), the residual stream after the last block -> (B, 256, 64, 64)."""
        W.require_library()
        if x.dim() != 3 or tuple(x.shape[1:]) != (NP, D) or x.dtype != torch.float32:
            raise ValueError("sam6d_hip.samenc: x must be float32 (B, %d, %d), got %s %s" % (NP, D, tuple(x.shape), x.dtype))
        B = x.shape[0]
        X = x.reshape(B * NP, D).contiguous()
        out = _empty((B, OUT, GRID, GRID), X)
        _neck(X, W, B, _empty((B * NP, OUT), X), _empty((B * NP, 10 * OUT), X), out, 0)
        return out


pieces = _Pieces


class EncoderView:
    """What the drop-in puts in the place of `sam.image_encoder`: a callable with .img_size that runs `encode` on packed weights."""

    def __init__(self, W, options=None):
        self.W, self.options, self.img_size = W, options, IMG

    def __call__(self, x):
        return encode(x, self.W, options=self.options)

    def from_rows(self, A):
        return encode_rows(A, self.W, options=self.options)
