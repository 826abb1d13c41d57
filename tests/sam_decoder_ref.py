"""Float64 restatement of SAM's point-prompt path and mask decoder, written against the reference line by line (test infrastructure
only; nothing here is imported by the package):
    PromptEncoder._embed_points (pad=True), PositionEmbeddingRandom, get_dense_pe    ISM/segment_anything/modeling/prompt_encoder.py
    MaskDecoder.predict_masks / forward, MLP                                         ISM/segment_anything/modeling/mask_decoder.py
    TwoWayTransformer, TwoWayAttentionBlock, Attention                               ISM/segment_anything/modeling/transformer.py
    LayerNorm2d, MLPBlock                                                            ISM/segment_anything/modeling/common.py
State dicts carry the reference's parameter names.  Everything runs in the dtype of the state dict it is given (float64 in the
tests); the prompt path rounds to float32 where the reference does (`coords.to(torch.float)` and the argument of sin / cos).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def to_dtype(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ---- prompt_encoder.py ------------------------------------------------------------------------------------------------------------------
def pe_encoding(coords, gauss):                                  # :185-192
    """coords float32.  The argument of sin / cos is formed in float32 in the reference's order (arguments reach +-50, where one
    float32 rounding is 4e-6 of the result): only sin and cos themselves run in gauss's dtype."""
    assert coords.dtype == torch.float32
    coords = 2 * coords - 1
    coords = coords @ gauss.to(torch.float32)
    coords = (2 * np.pi * coords).to(gauss.dtype)
    return torch.cat([torch.sin(coords), torch.cos(coords)], dim=-1)


def dense_pe(psd, grid):                                         # :62-71, :194-205 -> (1, C, h, w)
    gauss = psd["pe_layer.positional_encoding_gaussian_matrix"]
    h, w = grid
    ones = torch.ones((h, w), dtype=torch.float32, device=gauss.device)
    y_embed = ones.cumsum(dim=0) - 0.5
    x_embed = ones.cumsum(dim=1) - 0.5
    y_embed = y_embed / h
    x_embed = x_embed / w
    pe = pe_encoding(torch.stack([x_embed, y_embed], dim=-1), gauss)
    return pe.permute(2, 0, 1).unsqueeze(0)


def embed_points(psd, points, input_size):                       # :73-91 with labels = 1, pad = True; :207-214
    gauss = psd["pe_layer.positional_encoding_gaussian_matrix"]
    points = points[:, None, :] + 0.5
    padding_point = torch.zeros((points.shape[0], 1, 2), device=points.device)
    points = torch.cat([points, padding_point], dim=1)
    coords = points.clone()
    coords[:, :, 0] = coords[:, :, 0] / input_size[1]
    coords[:, :, 1] = coords[:, :, 1] / input_size[0]
    emb = pe_encoding(coords.to(torch.float), gauss)
    emb[:, 1, :] = 0.0                                            # labels == -1: the padding point
    emb[:, 1, :] += psd["not_a_point_embed.weight"][0]
    emb[:, 0, :] += psd["point_embeddings.1.weight"][0]           # labels == 1
    return emb


def dense_embeddings(psd, bs, grid):                             # :164-166
    return psd["no_mask_embed.weight"].reshape(1, -1, 1, 1).expand(bs, -1, grid[0], grid[1])


# ---- transformer.py ---------------------------------------------------------------------------------------------------------------------
def attention(sd, p, q, k, v, heads):                            # :218-240
    q = F.linear(q, sd[p + ".q_proj.weight"], sd[p + ".q_proj.bias"])
    k = F.linear(k, sd[p + ".k_proj.weight"], sd[p + ".k_proj.bias"])
    v = F.linear(v, sd[p + ".v_proj.weight"], sd[p + ".v_proj.bias"])

    def separate(x):
        b, n, c = x.shape
        return x.reshape(b, n, heads, c // heads).transpose(1, 2)
    q, k, v = separate(q), separate(k), separate(v)
    c_per_head = q.shape[-1]
    attn = q @ k.permute(0, 1, 3, 2)
    attn = attn / math.sqrt(c_per_head)
    attn = torch.softmax(attn, dim=-1)
    out = attn @ v
    b, n_heads, n_tokens, c_per_head = out.shape
    out = out.transpose(1, 2).reshape(b, n_tokens, n_heads * c_per_head)
    return F.linear(out, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def layer_norm(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def two_way_block(sd, p, queries, keys, query_pe, key_pe, heads, skip_first_layer_pe):   # :151-182
    if skip_first_layer_pe:
        queries = attention(sd, p + ".self_attn", queries, queries, queries, heads)
    else:
        q = queries + query_pe
        attn_out = attention(sd, p + ".self_attn", q, q, queries, heads)
        queries = queries + attn_out
    queries = layer_norm(sd, p + ".norm1", queries)
    q = queries + query_pe
    k = keys + key_pe
    attn_out = attention(sd, p + ".cross_attn_token_to_image", q, k, keys, heads)
    queries = queries + attn_out
    queries = layer_norm(sd, p + ".norm2", queries)
    mlp_out = F.linear(F.relu(F.linear(queries, sd[p + ".mlp.lin1.weight"], sd[p + ".mlp.lin1.bias"])), sd[p + ".mlp.lin2.weight"],
                       sd[p + ".mlp.lin2.bias"])
    queries = queries + mlp_out
    queries = layer_norm(sd, p + ".norm3", queries)
    q = queries + query_pe
    k = keys + key_pe
    attn_out = attention(sd, p + ".cross_attn_image_to_token", k, q, queries, heads)
    keys = keys + attn_out
    keys = layer_norm(sd, p + ".norm4", keys)
    return queries, keys


def two_way_transformer(sd, image_embedding, image_pe, point_embedding, heads):          # :62-106
    image_embedding = image_embedding.flatten(2).permute(0, 2, 1)
    image_pe = image_pe.flatten(2).permute(0, 2, 1)
    queries, keys = point_embedding, image_embedding
    depth = len({k.split(".")[2] for k in sd if k.startswith("transformer.layers.")})
    for i in range(depth):
        queries, keys = two_way_block(sd, "transformer.layers.%d" % i, queries, keys, point_embedding, image_pe, heads, i == 0)
    q = queries + point_embedding
    k = keys + image_pe
    attn_out = attention(sd, "transformer.final_attn_token_to_image", q, k, keys, heads)
    queries = queries + attn_out
    queries = layer_norm(sd, "transformer.norm_final_attn", queries)
    return queries, keys


# ---- mask_decoder.py --------------------------------------------------------------------------------------------------------------------
def mlp(sd, p, x, num_layers=3):                                 # :171-176
    for i in range(num_layers):
        x = F.linear(x, sd["%s.layers.%d.weight" % (p, i)], sd["%s.layers.%d.bias" % (p, i)])
        if i < num_layers - 1:
            x = F.relu(x)
    return x


def layer_norm_2d(sd, p, x, eps=1e-6):                           # common.py:38-43
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return sd[p + ".weight"][:, None, None] * x + sd[p + ".bias"][:, None, None]


def predict_masks(sd, image_embeddings, image_pe, sparse, dense, heads):                 # :112-149
    num_mask_tokens = sd["mask_tokens.weight"].shape[0]
    output_tokens = torch.cat([sd["iou_token.weight"], sd["mask_tokens.weight"]], dim=0)
    output_tokens = output_tokens.unsqueeze(0).expand(sparse.size(0), -1, -1)
    tokens = torch.cat((output_tokens, sparse), dim=1)
    src = torch.repeat_interleave(image_embeddings, tokens.shape[0], dim=0)
    src = src + dense
    pos_src = torch.repeat_interleave(image_pe, tokens.shape[0], dim=0)
    b, c, h, w = src.shape
    hs, src = two_way_transformer(sd, src, pos_src, tokens, heads)
    iou_token_out = hs[:, 0, :]
    mask_tokens_out = hs[:, 1:(1 + num_mask_tokens), :]
    src = src.transpose(1, 2).reshape(b, c, h, w)
    up = F.conv_transpose2d(src, sd["output_upscaling.0.weight"], sd["output_upscaling.0.bias"], stride=2)
    up = F.gelu(layer_norm_2d(sd, "output_upscaling.1", up))
    up = F.gelu(F.conv_transpose2d(up, sd["output_upscaling.3.weight"], sd["output_upscaling.3.bias"], stride=2))
    hyper_in = torch.stack([mlp(sd, "output_hypernetworks_mlps.%d" % i, mask_tokens_out[:, i, :]) for i in range(num_mask_tokens)], dim=1)
    b, c, h, w = up.shape
    masks = (hyper_in @ up.view(b, c, h * w)).view(b, -1, h, w)
    iou_pred = mlp(sd, "iou_prediction_head", iou_token_out)
    return masks, iou_pred


def decoder(sd, image_embeddings, image_pe, sparse, dense, heads):                       # :71-110 with multimask_output=True
    masks, iou_pred = predict_masks(sd, image_embeddings, image_pe, sparse, dense, heads)
    return masks[:, 1:, :, :], iou_pred[:, 1:]


def forward(psd, sd, points, features, heads, input_size, grid):
    """points (P, 2) in the input frame, features (1, C, h, w) -> (low (P, 3, 4h, 4w), iou (P, 3)) in sd's dtype."""
    dt = sd["iou_token.weight"].dtype
    sparse = embed_points(psd, points, input_size).to(dt)
    dense = dense_embeddings(psd, sparse.shape[0], grid).to(dt)
    return decoder(sd, features.to(dt), dense_pe(psd, grid).to(dt), sparse, dense, heads)


# ---- seeded weights of a given configuration (the reference's parameter names and shapes) -----------------------------------------------
def state_dict_shapes(dim, mlp_dim, depth=2):
    """(prompt encoder, mask decoder) name -> shape, the reference's names (mask_downscaling, unused by point prompts, left out)."""
    c2, c4, c8 = dim // 2, dim // 4, dim // 8
    ps = {"pe_layer.positional_encoding_gaussian_matrix": (2, c2), "not_a_point_embed.weight": (1, dim), "no_mask_embed.weight": (1, dim)}
    ps.update({"point_embeddings.%d.weight" % i: (1, dim) for i in range(4)})
    ds = {"iou_token.weight": (1, dim), "mask_tokens.weight": (4, dim)}

    def attn(p, inner):
        for n in ("q_proj", "k_proj", "v_proj"):
            ds["%s.%s.weight" % (p, n)] = (inner, dim)
            ds["%s.%s.bias" % (p, n)] = (inner,)
        ds[p + ".out_proj.weight"] = (dim, inner)
        ds[p + ".out_proj.bias"] = (dim,)

    def norm(p, n=dim):
        ds[p + ".weight"] = (n,)
        ds[p + ".bias"] = (n,)
    for i in range(depth):
        p = "transformer.layers.%d" % i
        attn(p + ".self_attn", dim)
        attn(p + ".cross_attn_token_to_image", c2)
        attn(p + ".cross_attn_image_to_token", c2)
        for n in ("norm1", "norm2", "norm3", "norm4"):
            norm(p + "." + n)
        ds[p + ".mlp.lin1.weight"], ds[p + ".mlp.lin1.bias"] = (mlp_dim, dim), (mlp_dim,)
        ds[p + ".mlp.lin2.weight"], ds[p + ".mlp.lin2.bias"] = (dim, mlp_dim), (dim,)
    attn("transformer.final_attn_token_to_image", c2)
    norm("transformer.norm_final_attn")
    ds["output_upscaling.0.weight"], ds["output_upscaling.0.bias"] = (dim, c4, 2, 2), (c4,)
    norm("output_upscaling.1", c4)
    ds["output_upscaling.3.weight"], ds["output_upscaling.3.bias"] = (c4, c8, 2, 2), (c8,)
    for i in range(4):
        for j, (a, b) in enumerate(((dim, dim), (dim, dim), (dim, c8))):
            ds["output_hypernetworks_mlps.%d.layers.%d.weight" % (i, j)] = (b, a)
            ds["output_hypernetworks_mlps.%d.layers.%d.bias" % (i, j)] = (b,)
    for j, (a, b) in enumerate(((dim, dim), (dim, dim), (dim, 4))):
        ds["iou_prediction_head.layers.%d.weight" % j] = (b, a)
        ds["iou_prediction_head.layers.%d.bias" % j] = (b,)
    return ps, ds


def seeded_weights(seed, dim=256, mlp_dim=2048, depth=2):
    """float32 state dicts from a seed: matrices ~ N(0, 1 / fan_in), norm weights 1 + 0.1 N, biases and embeddings 0.1 ... 0.5 N, the
    Gaussian matrix N(0, 1) as PositionEmbeddingRandom draws it.  The order of the draws is the sorted order of the names."""
    g = torch.Generator().manual_seed(seed)
    ps, ds = state_dict_shapes(dim, mlp_dim, depth)
    out = []
    for shapes in (ps, ds):
        sd = {}
        for name in sorted(shapes):
            shape = shapes[name]
            r = torch.randn(shape, generator=g)
            if name.endswith("gaussian_matrix"):
                v = r
            elif "norm" in name or name.startswith("output_upscaling.1"):
                v = 1.0 + 0.1 * r if name.endswith("weight") else 0.1 * r
            elif name.startswith("output_upscaling") and name.endswith("weight"):
                v = r / math.sqrt(shape[0])
            elif len(shape) == 2 and shape[0] > 4 or name.endswith("layers.2.weight"):
                v = r / math.sqrt(shape[1])
            elif name.endswith("bias"):
                v = 0.1 * r
            else:
                v = 0.5 * r  # embeddings and tokens
            sd[name] = v.contiguous()
        out.append(sd)
    return out[0], out[1]


def seeded_features(seed, dim=256, grid=(64, 64)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, dim) + tuple(grid), generator=g)
