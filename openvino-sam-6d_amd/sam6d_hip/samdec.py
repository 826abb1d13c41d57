"""SAM's prompt encoder (point prompts) and mask decoder on the library: points in the model's input frame -> low-resolution logits
(ISM/segment_anything/modeling/prompt_encoder.py:73-91, 128-168, 185-214; mask_decoder.py:112-149; transformer.py:62-106, 151-182,
218-240).  multimask_output=True, no boxes, no mask inputs, SAM's one decoder configuration (CONFIG below); the image encoder is not
part of this.

What the decoder does per point batch of P prompts, and what is done with it here:
  * layer 0's image-side projections do not depend on the prompt (`keys` is still image_embedding + no_mask_embed there): they are
    tables over the 4096 image rows, built once per image (`image_tables`), and the P-fold repeat of the embedding is never formed;
  * every later pass over the P x 4096 keys is ONE sam6d_gemm_nt(_w16) launch with the weights that read those keys stacked
    (token->image k and v with image->token q: 384 columns; the final attention's k and v with ConvTranspose 1: 512 columns); the
    `image_pe` part of k and q is linear, so pe . W^T + bias is a per-image table added in that GEMM's epilogue;
  * the image->token attention has 7 keys: out_proj is folded into the 7 x 8 value rows (a (P, 56, 256) table) and one kernel goes from
    q to the normalised new keys (sam6d_samdec_image_to_token);
  * the token->image attention splits the 4096 keys over workgroups (sam6d_samdec_token_to_image);
  * LayerNorm2d, GELU, ConvTranspose 2, GELU and the product with hyper_in[1:4] are one kernel (sam6d_samdec_upscale_masks): only
    (P, 3, 256, 256) is written, mask token 0's map is not computed;
  * the P x 7 token rows (self attention over 7, MLP, norms, hypernetworks, IoU head) are sam6d_gemm_nt launches and small torch
    vector ops on the device; nothing is read back to the host.

`eager` is the same function in plain torch ops on any device and dtype, written after the reference: the package's own partner
(CPU path, timing baseline, float64 check), like dinov2.crop_resize_pad and amg.eager_tail.  `TorchOps` runs the restructured
sequence (tables, stacked projections, fold) in plain torch, which is how the restructuring itself is checked in float64 on the host.
"""
import math
import types

import torch
import torch.nn.functional as F

from . import _lib
from .runtime import Linear, _empty, _p, _s, gemm, library_call, linear

CONFIG = dict(dim=256, heads=8, depth=2, mlp=2048, grid=(64, 64), mask_tokens=4)
T = 7  # tokens per prompt: iou, 4 mask tokens, the point, the padding point


def _sd(m):
    return m.state_dict() if hasattr(m, "state_dict") else m


def _depth(decoder_sd):
    return len({k.split(".")[2] for k in decoder_sd if k.startswith("transformer.layers.")})


def check_state_dicts(prompt_sd, decoder_sd, num_heads, grid=(64, 64), boxes=None, masks=None, multimask_output=True):
    """Raises NotImplementedError, naming the value, for anything but the configuration the kernels are built for."""
    def refuse(what, got, want):
        raise NotImplementedError("sam6d_hip.samdec: %s = %s is not implemented (the kernels are built for %s)" % (what, got, want))
    if boxes is not None:
        refuse("box prompts", "given", "point prompts only")
    if masks is not None:
        refuse("mask prompts", "given", "point prompts only")
    if not multimask_output:
        refuse("multimask_output", multimask_output, "True")
    dim = int(decoder_sd["iou_token.weight"].shape[1])
    if dim != CONFIG["dim"]:
        refuse("transformer_dim", dim, CONFIG["dim"])
    if int(num_heads) != CONFIG["heads"]:
        refuse("num_heads", num_heads, CONFIG["heads"])
    if _depth(decoder_sd) != CONFIG["depth"]:
        refuse("transformer depth", _depth(decoder_sd), CONFIG["depth"])
    mlp = int(decoder_sd["transformer.layers.0.mlp.lin1.weight"].shape[0])
    if mlp != CONFIG["mlp"]:
        refuse("mlp_dim", mlp, CONFIG["mlp"])
    nm = int(decoder_sd["mask_tokens.weight"].shape[0])
    if nm != CONFIG["mask_tokens"]:
        refuse("num_mask_tokens", nm, CONFIG["mask_tokens"])
    ci = int(decoder_sd["transformer.layers.0.cross_attn_token_to_image.q_proj.weight"].shape[0])
    if ci != dim // 2:
        refuse("attention_downsample_rate", "%d / %d" % (dim, ci), 2)
    if tuple(int(g) for g in grid) != CONFIG["grid"]:
        refuse("image_embedding_size", tuple(grid), CONFIG["grid"])
    pw = int(prompt_sd["pe_layer.positional_encoding_gaussian_matrix"].shape[1])
    if 2 * pw != dim:
        refuse("prompt embed_dim", 2 * pw, dim)


class SamDecoderWeights:
    """The weights of a prompt encoder and a mask decoder (modules, or their state dicts with num_heads / input_image_size / grid given)
    on `device` in `dtype`, the dense positional encoding, and the stacked / rearranged operands of the restructured sequence, made
    once.  The fp16 halves of the GEMM weights are cut when the library first uses them (Linear.w16)."""

    def __init__(self, prompt_encoder, mask_decoder, device, dtype=torch.float32, num_heads=None, input_image_size=None, grid=None,
                 options=None):
        self.dev, self.dtype, self.options = torch.device(device), dtype, options
        tr = getattr(mask_decoder, "transformer", None)
        self.heads = int(num_heads if num_heads is not None else tr.num_heads)
        self.input_size = tuple(int(v) for v in (input_image_size if input_image_size is not None else prompt_encoder.input_image_size))
        self.grid = tuple(int(v) for v in (grid if grid is not None else prompt_encoder.image_embedding_size))
        for what, get, want in (("transformer MLP activation", lambda: tr.layers[0].mlp.act, "ReLU"),
                                ("output_upscaling activation", lambda: mask_decoder.output_upscaling[2], "GELU")):
            try:  # (a network that keeps the reference's modules says which activations it was built with)
                act = type(get()).__name__
            except (AttributeError, TypeError, IndexError, KeyError):
                continue
            if act != want:
                raise NotImplementedError("sam6d_hip.samdec: %s = %s is not implemented (%s is)" % (what, act, want))
        pe32 = {k: v.detach().to(self.dev) for k, v in _sd(prompt_encoder).items() if not k.startswith("mask_downscaling")}
        self.pe = {k: v.to(dtype) for k, v in pe32.items()}
        self.md = {k: v.detach().to(self.dev, dtype) for k, v in _sd(mask_decoder).items()}
        self.dim = int(self.md["iou_token.weight"].shape[1])
        self.depth = _depth(self.md)
        self.N = self.grid[0] * self.grid[1]
        self.dense_pe = _dense_pe(self.pe["pe_layer.positional_encoding_gaussian_matrix"], self.grid)  # (N, C)
        self._merge()
        self._linears = {}

    def _merge(self):
        md, C, pe = self.md, self.dim, self.dense_pe.double()
        m = {}

        def wb(p):
            return md[p + ".weight"], md[p + ".bias"]

        def pe_table(w, b):
            return (pe @ w.double().t() + b.double()).to(self.dtype)

        for i in range(self.depth):
            p = "transformer.layers.%d." % i
            (wk, bk), (wv, bv), (wq, bq) = (wb(p + "cross_attn_token_to_image.k_proj"), wb(p + "cross_attn_token_to_image.v_proj"),
                                            wb(p + "cross_attn_image_to_token.q_proj"))
            m["big%d" % i] = (torch.cat([wk, wv, wq]).contiguous(),
                              torch.cat([pe_table(wk, bk), bv[None].expand(self.N, -1), pe_table(wq, bq)], dim=1).contiguous())
            (sq, sbq), (sk, sbk) = wb(p + "self_attn.q_proj"), wb(p + "self_attn.k_proj")
            m[p + "self_attn.qk"] = (torch.cat([sq, sk]).contiguous(), torch.cat([sbq, sbk]).contiguous())
        (wk, bk), (wv, bv) = wb("transformer.final_attn_token_to_image.k_proj"), wb("transformer.final_attn_token_to_image.v_proj")
        w1, b1 = wb("output_upscaling.0")  # ConvTranspose2d (in, out, kh, kw): GEMM row (2 kh + kw) * out + o
        w1 = w1.permute(2, 3, 1, 0).reshape(-1, C)
        m["bigf"] = (torch.cat([wk, wv, w1]).contiguous(),
                     torch.cat([pe_table(wk, bk), bv[None].expand(self.N, -1), b1.repeat(4)[None].expand(self.N, -1)], dim=1).contiguous())
        w2, b2 = wb("output_upscaling.3")
        m["up2"] = (w2.permute(2, 3, 1, 0).reshape(-1, w2.shape[0]).contiguous(), b2.repeat(4).contiguous())
        self.merged = m

    def wb(self, name):
        """(weight (N, K), bias or table) of a Linear of the decoder or of a stacked operand."""
        if name in self.merged:
            return self.merged[name]
        return self.md[name + ".weight"], self.md[name + ".bias"]

    def linear(self, name, bias=True):
        """The Linear (weight, bias, fp16 halves on demand) of `name`; stacked image-side operands carry no bias (their table is the
        GEMM's residual)."""
        lin = self._linears.get(name)
        if lin is None:
            w, b = self.wb(name)
            lin = self._linears[name] = Linear(w, b if bias else None)
        return lin

    def require_library(self):
        if self.dtype != torch.float32 or self.dev.type != "cuda":
            raise RuntimeError("sam6d_hip.samdec: the library path needs float32 weights on a HIP device (this build has no CPU path)")
        check_state_dicts(self.pe, self.md, self.heads, self.grid)


# ------------------------------------------------------------------------------------------------- prompt points
def _pe_encoding(coords32, gauss):
    """PositionEmbeddingRandom._pe_encoding (prompt_encoder.py:185-192) of float32 coordinates in [0, 1], in gauss's dtype."""
    coords = 2 * coords32 - 1
    coords = coords @ gauss.to(torch.float32)
    coords = (2 * math.pi * coords).to(gauss.dtype)  # the argument in float32 whatever gauss's dtype: it reaches +-50
    return torch.cat([torch.sin(coords), torch.cos(coords)], dim=-1)


def _dense_pe(gauss, grid):
    """PromptEncoder.get_dense_pe (prompt_encoder.py:62-71, 194-205) as (h w, C) rows, row y w + x."""
    h, w = grid
    ones = torch.ones((h, w), device=gauss.device, dtype=torch.float32)
    y_embed = (ones.cumsum(dim=0) - 0.5) / h
    x_embed = (ones.cumsum(dim=1) - 0.5) / w
    return _pe_encoding(torch.stack([x_embed, y_embed], dim=-1), gauss).reshape(h * w, -1)


def embed_points(points, W):
    """PromptEncoder._embed_points with pad=True and one foreground label per point (prompt_encoder.py:73-91, 207-214): points (P, 2) xy
    in the input frame, in the caller's dtype up to the reference's `coords.to(torch.float)` -> (P, 2, C) [point, padding point]."""
    points = points.to(W.dev)[:, None, :] + 0.5
    pad = torch.zeros((points.shape[0], 1, 2), device=points.device)
    coords = torch.cat([points, pad], dim=1).clone()
    coords[:, :, 0] = coords[:, :, 0] / W.input_size[1]
    coords[:, :, 1] = coords[:, :, 1] / W.input_size[0]
    emb = _pe_encoding(coords.to(torch.float), W.pe["pe_layer.positional_encoding_gaussian_matrix"])
    emb[:, 1, :] = 0.0
    emb[:, 1, :] += W.pe["not_a_point_embed.weight"][0]
    emb[:, 0, :] += W.pe["point_embeddings.1.weight"][0]
    return emb


def _tokens(points, W):
    sparse = embed_points(points, W)
    out = torch.cat([W.md["iou_token.weight"], W.md["mask_tokens.weight"]], dim=0)
    return torch.cat((out.unsqueeze(0).expand(sparse.shape[0], -1, -1), sparse), dim=1)


# ------------------------------------------------------------------------------------------------- eager: the reference's sequence
def _attention(md, p, q, k, v, heads):
    """Attention.forward (transformer.py:218-240)."""
    q = F.linear(q, md[p + "q_proj.weight"], md[p + "q_proj.bias"])
    k = F.linear(k, md[p + "k_proj.weight"], md[p + "k_proj.bias"])
    v = F.linear(v, md[p + "v_proj.weight"], md[p + "v_proj.bias"])

    def sep(x):
        b, n, c = x.shape
        return x.reshape(b, n, heads, c // heads).transpose(1, 2)
    q, k, v = sep(q), sep(k), sep(v)
    attn = q @ k.permute(0, 1, 3, 2)
    attn = torch.softmax(attn / math.sqrt(q.shape[-1]), dim=-1)
    out = (attn @ v).transpose(1, 2)
    out = out.reshape(out.shape[0], out.shape[1], -1)
    return F.linear(out, md[p + "out_proj.weight"], md[p + "out_proj.bias"])


def _ln(md, p, x, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), md[p + ".weight"], md[p + ".bias"], eps)


def _mlp3(md, p, x):
    """MLP with three layers (mask_decoder.py:171-176)."""
    for i in range(3):
        x = F.linear(x, md["%s.layers.%d.weight" % (p, i)], md["%s.layers.%d.bias" % (p, i)])
        if i < 2:
            x = F.relu(x)
    return x


def eager(points, features, W):
    """points (P, 2) xy in the input frame, features (1, C, h, w) -> (low (P, 3, 4h, 4w), iou (P, 3)): prompt encoder and mask decoder
    with multimask_output=True, op for op as the reference runs them, in W's dtype on W's device."""
    md, H = W.md, W.heads
    tokens = _tokens(points, W)
    P = tokens.shape[0]
    src = features.to(W.dev, W.dtype).expand(P, -1, -1, -1) + W.pe["no_mask_embed.weight"].reshape(1, -1, 1, 1)
    b, c, h, w = src.shape
    keys = src.flatten(2).permute(0, 2, 1)
    key_pe = W.dense_pe[None].expand(P, -1, -1)
    queries, query_pe = tokens, tokens
    for i in range(W.depth):
        p = "transformer.layers.%d." % i
        if i == 0:
            queries = _attention(md, p + "self_attn.", queries, queries, queries, H)
        else:
            q = queries + query_pe
            queries = queries + _attention(md, p + "self_attn.", q, q, queries, H)
        queries = _ln(md, p + "norm1", queries)
        q, k = queries + query_pe, keys + key_pe
        queries = _ln(md, p + "norm2", queries + _attention(md, p + "cross_attn_token_to_image.", q, k, keys, H))
        mlp = F.linear(F.relu(F.linear(queries, md[p + "mlp.lin1.weight"], md[p + "mlp.lin1.bias"])), md[p + "mlp.lin2.weight"],
                       md[p + "mlp.lin2.bias"])
        queries = _ln(md, p + "norm3", queries + mlp)
        q, k = queries + query_pe, keys + key_pe
        keys = _ln(md, p + "norm4", keys + _attention(md, p + "cross_attn_image_to_token.", k, q, queries, H))
    q, k = queries + query_pe, keys + key_pe
    queries = _ln(md, "transformer.norm_final_attn", queries + _attention(md, "transformer.final_attn_token_to_image.", q, k, keys, H))
    up = F.conv_transpose2d(keys.transpose(1, 2).reshape(b, c, h, w), md["output_upscaling.0.weight"], md["output_upscaling.0.bias"], stride=2)
    u = up.mean(1, keepdim=True)
    s = (up - u).pow(2).mean(1, keepdim=True)
    up = (up - u) / torch.sqrt(s + 1e-6)
    up = F.gelu(md["output_upscaling.1.weight"][:, None, None] * up + md["output_upscaling.1.bias"][:, None, None])
    up = F.gelu(F.conv_transpose2d(up, md["output_upscaling.3.weight"], md["output_upscaling.3.bias"], stride=2))
    hyper_in = torch.stack([_mlp3(md, "output_hypernetworks_mlps.%d" % m, queries[:, 1 + m, :]) for m in range(4)], dim=1)
    b, c, h, w = up.shape
    masks = (hyper_in @ up.view(b, c, h * w)).view(b, -1, h, w)
    iou = _mlp3(md, "iou_prediction_head", queries[:, 0, :])
    return masks[:, 1:, :, :], iou[:, 1:]


# ------------------------------------------------------------------------------------------------- the restructured sequence
class TorchOps:
    """The steps of `_forward` in plain torch, any device and dtype."""

    def __init__(self, W):
        self.W = W

    def linear(self, x, name, act=0, residual=None):
        w, b = self.W.wb(name)
        y = F.linear(x, w, b)
        if act == 1:
            y = F.relu(y)
        return y if residual is None else residual + y

    def big(self, keys, name):
        w, table = self.W.wb(name)
        return keys @ w.t() + table

    def fold(self, vtok, name):
        W = self.W
        P, d = vtok.shape[0], vtok.shape[2] // W.heads
        wo = W.md[name + ".weight"].view(W.dim, W.heads, d)
        return torch.einsum("pjhd,chd->pjhc", vtok.view(P, T, W.heads, d), wo).reshape(P, T * W.heads, W.dim)

    def t2i(self, q, G, k_off, v_off):
        W = self.W
        P, ci = q.shape[0], q.shape[2]
        d = ci // W.heads
        k = G[:, :, k_off:k_off + ci].reshape(G.shape[0], W.N, W.heads, d)
        v = G[:, :, v_off:v_off + ci].reshape(G.shape[0], W.N, W.heads, d)
        s = torch.einsum("pjhd,pnhd->pjhn", q.view(P, T, W.heads, d), k.expand(P, -1, -1, -1)) / math.sqrt(d)
        return torch.einsum("pjhn,pnhd->pjhd", torch.softmax(s, dim=-1), v.expand(P, -1, -1, -1)).reshape(P, T, ci)

    def i2t(self, G, q_off, ktok, fold, p, keys):
        W = self.W
        P, ci = ktok.shape[0], ktok.shape[2]
        d = ci // W.heads
        q = G[:, :, q_off:q_off + ci].reshape(G.shape[0], W.N, W.heads, d).expand(P, -1, -1, -1)
        s = torch.einsum("pnhd,pjhd->pnjh", q, ktok.view(P, T, W.heads, d)) / math.sqrt(d)
        a = torch.einsum("pnjh,pjhc->pnc", torch.softmax(s, dim=2), fold.view(P, T, W.heads, W.dim))
        x = keys + (a + W.md[p + "cross_attn_image_to_token.out_proj.bias"])
        return _ln(W.md, p + "norm4", x)

    def upscale(self, G, off, hyper):
        W = self.W
        P, C = G.shape[0], W.dim
        gh, gw = W.grid
        x = G[:, :, off:off + C].reshape(P, W.N, 4, C // 4)
        u = x.mean(-1, keepdim=True)
        s = (x - u).pow(2).mean(-1, keepdim=True)
        x = F.gelu(W.md["output_upscaling.1.weight"] * ((x - u) / torch.sqrt(s + 1e-6)) + W.md["output_upscaling.1.bias"])
        w2, b2 = W.wb("up2")
        y = F.gelu(x @ w2.t() + b2).reshape(P, W.N, 4, 4, C // 8)
        m = torch.einsum("pnsuc,pmc->pmnsu", y, hyper)
        # (p, m, ty, tx, a, b, c, d) -> pixel (4 ty + 2 a + c, 4 tx + 2 b + d)
        return m.reshape(P, 3, gh, gw, 2, 2, 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(P, 3, 4 * gh, 4 * gw)


class HipOps:
    """The same steps on the library: sam6d_gemm_nt(_w16) for every projection, the three kernels of csrc/samdec.hip for the rest."""

    def __init__(self, W):
        self.W = W
        self.shape = (W.dim, W.heads, T, W.grid[0], W.grid[1])
        self.ws = None

    def linear(self, x, name, act=0, residual=None):
        lin = self.W.linear(name)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        r2 = None if residual is None else residual.reshape(-1, residual.shape[-1]).contiguous()
        y = linear(x2, lin, act=act, residual=r2)
        return y.view(*x.shape[:-1], y.shape[-1])

    def big(self, keys, name):
        """keys (P, N, C) . stacked weight^T + per-image table, one launch: a batch of P problems that share weight and table."""
        W = self.W
        lin, table = W.linear(name, bias=False), W.wb(name)[1]
        P, N, C, NO = keys.shape[0], W.N, W.dim, lin.w.shape[0]
        keys = keys.contiguous()
        out = _empty((P, N, NO), keys)
        gemm(keys, lin.w, None, out, N, NO, C, C, C, NO, residual=table, ldr=NO, batch=P, sA=N * C, sW=0, sC=N * NO, sR=0,
             w16=lin.w16())
        return out

    def fold(self, vtok, name):
        """(P, 56, 256), row 8 j + h = out_proj.weight[:, 16h:16h+16] . v[j, 16h:16h+16]: one problem per head (K = 16: the exact loop)."""
        W = self.W
        P, ci = vtok.shape[0], vtok.shape[2]
        d, C, H = ci // W.heads, W.dim, W.heads
        vtok = vtok.contiguous()
        out = _empty((P, T * H, C), vtok)
        gemm(vtok, W.md[name + ".weight"], None, out, P * T, C, d, ci, ci, H * C, batch=H, sA=d, sW=d, sC=C)
        return out

    def t2i(self, q, G, k_off, v_off):
        W = self.W
        P = q.shape[0]
        q = q.contiguous()
        ld = G.shape[2]
        need = _lib.load().sam6d_samdec_token_to_image_workspace_bytes(P)
        if self.ws is None or self.ws.numel() * 4 < need:
            self.ws = _empty(((need + 3) // 4,), q)
        out = _empty((P, T, q.shape[2]), q)
        _lib.call("sam6d_samdec_token_to_image", _p(q), _p(G, k_off), _p(G, v_off), ld, 0 if G.shape[0] == 1 else W.N * ld,
                  _p(out), P, *self.shape, self.ws.data_ptr(), self.ws.numel() * 4, _s())
        return out

    def i2t(self, G, q_off, ktok, fold, p, keys):
        W, md = self.W, self.W.md
        P, ld = ktok.shape[0], G.shape[2]
        out = _empty((P, W.N, W.dim), ktok)
        _lib.call("sam6d_samdec_image_to_token", _p(G, q_off), ld, 0 if G.shape[0] == 1 else W.N * ld, _p(ktok.contiguous()),
                  _p(fold), _p(md[p + "cross_attn_image_to_token.out_proj.bias"]), _p(keys),
                  0 if keys.shape[0] == 1 else W.N * W.dim, _p(md[p + "norm4.weight"]), _p(md[p + "norm4.bias"]), 1e-5,
                  _p(out), P, *self.shape, _s())
        return out

    def upscale(self, G, off, hyper):
        W, md = self.W, self.W.md
        P, ld = G.shape[0], G.shape[2]
        w2, b2 = W.wb("up2")
        low = _empty((P, 3, 4 * W.grid[0], 4 * W.grid[1]), G)
        _lib.call("sam6d_samdec_upscale_masks", _p(G, off), ld, W.N * ld, _p(md["output_upscaling.1.weight"]),
                  _p(md["output_upscaling.1.bias"]), 1e-6, _p(w2), _p(b2), _p(hyper.contiguous()), _p(low), P,
                  *self.shape, _s())
        return low


def _self_attention(q, k, v, heads):
    """Attention over the 7 tokens of each prompt as broadcast vector ops: q, k, v (P, T, C) projected -> (P, T, C)."""
    P, n, C = q.shape
    d = C // heads
    q, k, v = q.reshape(P, n, heads, d), k.reshape(P, n, heads, d), v.reshape(P, n, heads, d)
    s = (q.unsqueeze(2) * k.unsqueeze(1)).sum(-1) / math.sqrt(d)          # (P, query, key, head)
    return (torch.softmax(s, dim=2).unsqueeze(-1) * v.unsqueeze(1)).sum(2).reshape(P, n, C)


def _tables(ops, features, W):
    src = features.to(W.dev, W.dtype).flatten(2).permute(0, 2, 1) + W.pe["no_mask_embed.weight"]  # (1, N, C)
    src = src.contiguous()
    return types.SimpleNamespace(src=src, g0=ops.big(src, "big0"))


def _forward(ops, points, tables, W):
    md, C = W.md, W.dim
    ci = C // 2
    tokens = _tokens(points, W)
    queries, keys, G = tokens, tables.src, tables.g0
    for i in range(W.depth):
        p = "transformer.layers.%d." % i
        qk = ops.linear(queries if i == 0 else queries + tokens, p + "self_attn.qk")
        a = _self_attention(qk[..., :C], qk[..., C:], ops.linear(queries, p + "self_attn.v_proj"), W.heads)
        queries = _ln(md, p + "norm1", ops.linear(a, p + "self_attn.out_proj", residual=None if i == 0 else queries))
        if i > 0:
            G = ops.big(keys, "big%d" % i)
        a = ops.t2i(ops.linear(queries + tokens, p + "cross_attn_token_to_image.q_proj"), G, 0, ci)
        queries = _ln(md, p + "norm2", ops.linear(a, p + "cross_attn_token_to_image.out_proj", residual=queries))
        hid = ops.linear(queries, p + "mlp.lin1", act=1)
        queries = _ln(md, p + "norm3", ops.linear(hid, p + "mlp.lin2", residual=queries))
        ktok = ops.linear(queries + tokens, p + "cross_attn_image_to_token.k_proj")
        fold = ops.fold(ops.linear(queries, p + "cross_attn_image_to_token.v_proj"), p + "cross_attn_image_to_token.out_proj")
        keys = ops.i2t(G, 2 * ci, ktok, fold, p, keys)
    G = ops.big(keys, "bigf")
    a = ops.t2i(ops.linear(queries + tokens, "transformer.final_attn_token_to_image.q_proj"), G, 0, ci)
    queries = _ln(md, "transformer.norm_final_attn", ops.linear(a, "transformer.final_attn_token_to_image.out_proj", residual=queries))

    def mlp3(p, x):
        x = ops.linear(ops.linear(x, p + ".layers.0", act=1), p + ".layers.1", act=1)
        return ops.linear(x, p + ".layers.2")
    hyper = torch.stack([mlp3("output_hypernetworks_mlps.%d" % m, queries[:, 1 + m, :]) for m in (1, 2, 3)], dim=1)  # token 0 is iou
    iou = mlp3("iou_prediction_head", queries[:, 0, :])[:, 1:]
    return ops.upscale(G, 2 * ci, hyper), iou


def restructured(points, features, W):
    """`eager`'s result through the restructured sequence in plain torch (TorchOps): the check of the tables, the stacked projections
    and the fold, in any dtype."""
    ops = TorchOps(W)
    return _forward(ops, points, _tables(ops, features, W), W)


_entry = library_call("sam6d_hip.samdec", "SAM mask decoder")


@_entry
def image_tables(features, W):
    """features (1, 256, 64, 64) on the HIP device -> the per-image tables of layer 0 (src = embedding + no_mask_embed, and its k / v /
    q projections with the positional part added), once per set_image."""
    W.require_library()
    if tuple(features.shape) != (1, W.dim) + W.grid:
        raise ValueError("image_tables: features must be (1, %d, %d, %d), got %s" % ((W.dim,) + W.grid + (tuple(features.shape),)))
    return _tables(HipOps(W), features, W)


def predict_low(points, tables, W, options=None):
    """points (P, 2) xy in the model's input frame (a tensor; float64 as amg.apply_coords leaves them, or float32) -> (low (P, 3, 256, 256),
    iou (P, 3)) on W's device.  No host read-back."""
    return _predict_low(tables.src, points, tables, W, options=options)


@_entry
def _predict_low(_src, points, tables, W):
    W.require_library()
    return _forward(HipOps(W), points, tables, W)
