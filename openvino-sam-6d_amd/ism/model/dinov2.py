"""Drop-in for ISM/model/dinov2.py::CustomDINOv2 (:115-326), the descriptor model of Instance_Segmentation_Model: constructor
arguments, attribute names and methods are the reference's; it imports neither openvino, pytorch_lightning nor torchvision (CustomDINOv2 is a plain nn.Module).

`self.model` is a plain-PyTorch DinoVisionTransformer with the state-dict keys of the reference's
vision_transformer.vit_*(patch_size=14, img_size=518, init_values=1.0, block_chunks=0), so the released
`dinov2_vitl14_pretrain.pth` loads with strict=True.  It is the CPU path and the fp32 parity partner.  With tensors on a HIP device
and model_name "dinov2_vitl14" the library runs instead (sam6d_hip/dinov2.py: crops, encoder and masked patch descriptors as HIP
kernels); SAM6D_HIP_DINOV2=0 selects eager PyTorch there too.  The other three model names construct and run eager.

Differences from the reference, on purpose:
  * the reference pads the last chunk with zero images and slices the result (:292-302); results do not depend on it, so it is not
    done.  On the library path the chunk size is the library's own slice (sam6d_hip.dinov2.SLICE), `chunk_size` bounds the eager path;
  * process_masks_proposals keeps the in-place `masks.unsqueeze_(1)` on the caller's tensor (:228: the caller's `proposals.masks` is
    (N, 1, H, W) afterwards, which the detector's later steps undo), but squeezes only that dimension of its result: the reference's
    bare `.squeeze_()` (:231) turns the result of a single proposal into (224, 224) and the chunked forward then fails on it; here one
    proposal gives (1, 224, 224);
  * images may live on any device (the reference calls `.numpy()` on them for OpenVINO).  The eager path runs where `self.model`
    lives: with the model left on the CPU, images on a GPU are copied to the host, encoded there and the result copied back, which is
    orders of magnitude slower than either GPU path -- move the model with `.model.to(device)` as the reference's script does (:118);
  * an image that is not (H, W, 3) uint8 takes the eager crop path also on a HIP device; boxes must be integers on both paths
    (ValueError otherwise: the reference's slicing does not take floating-point boxes either; `Detections` converts them to int64).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from utils.bbox_utils import CropResizePad

descriptor_size = {"dinov2_vits14": 384, "dinov2_vitb14": 768, "dinov2_vitl14": 1024, "dinov2_vitg14": 1536}
descriptor_map = {"dinov2_vits14": "vit_small", "dinov2_vitb14": "vit_base", "dinov2_vitl14": "vit_large", "dinov2_vitg14": "vit_giant2"}
# (embed_dim, depth, heads, ffn) of ISM/model/vision_transformer.py:339-389
_ARCH = {"vit_small": (384, 12, 6, "mlp"), "vit_base": (768, 12, 12, "mlp"), "vit_large": (1024, 24, 16, "mlp"),
         "vit_giant2": (1536, 40, 24, "swiglufused")}
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------------------- the eager model (plain PyTorch)
class _PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class _Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * self.scale, qkv[1], qkv[2]
        attn = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


class _LayerScale(nn.Module):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _SwiGLU(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        hidden = (int(hidden * 2 / 3) + 7) // 8 * 8
        self.w12 = nn.Linear(dim, 2 * hidden)
        self.w3 = nn.Linear(hidden, dim)

    def forward(self, x):
        x1, x2 = self.w12(x).chunk(2, dim=-1)
        return self.w3(F.silu(x1) * x2)


class _Block(nn.Module):
    def __init__(self, dim, num_heads, ffn, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, num_heads)
        self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, 4 * dim) if ffn == "mlp" else _SwiGLU(dim, 4 * dim)
        self.ls2 = _LayerScale(dim, init_values)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class DinoVisionTransformer(nn.Module):
    """The DINOv2 backbone as the descriptor path uses it (no masks, no register tokens, no drop path): forward_features returns the
    reference's dictionary (ISM/model/vision_transformer.py:250-266)."""

    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, ffn_layer="mlp", init_values=1.0,
                 interpolate_offset=0.1):
        super().__init__()
        self.embed_dim = self.num_features = embed_dim
        self.n_blocks, self.num_heads, self.patch_size = depth, num_heads, patch_size
        self.num_register_tokens = 0
        self.interpolate_offset = interpolate_offset
        self.patch_embed = _PatchEmbed(img_size, patch_size, 3, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, ffn_layer, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def interpolate_pos_encoding(self, x, w, h):
        from sam6d_hip.dinov2 import interpolate_pos_embed
        if w != h or w % self.patch_size:
            raise NotImplementedError("DinoVisionTransformer: square images of whole patches only, got %d x %d" % (w, h))
        return interpolate_pos_embed(self.pos_embed, w // self.patch_size, self.interpolate_offset).to(x.dtype)

    def prepare_tokens_with_masks(self, x, masks=None):
        if masks is not None:
            raise NotImplementedError("DinoVisionTransformer: mask tokens are not part of the descriptor path")
        _, _, w, h = x.shape
        x = self.patch_embed(x)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        return x + self.interpolate_pos_encoding(x, w, h)

    def forward_features(self, x, masks=None):
        x = self.prepare_tokens_with_masks(x, masks)
        for blk in self.blocks:
            x = blk(x)
        x_norm = self.norm(x)
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_regtokens": x_norm[:, 1:1], "x_norm_patchtokens": x_norm[:, 1:],
                "x_prenorm": x, "masks": masks}

    def forward(self, x, is_training=False, mask=None, **kwargs):
        ret = self.forward_features(x, mask)
        return ret, ret["x_norm_clstoken"]


def _make_dinov2_model(arch_name="vit_large", img_size=518, patch_size=14, init_values=1.0, **kwargs):
    dim, depth, heads, ffn = _ARCH[arch_name]
    return DinoVisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=dim, depth=depth, num_heads=heads, ffn_layer=ffn,
                                 init_values=init_values)


# ----------------------------------------------------------------------------------------- the descriptor model
class CustomDINOv2(nn.Module):
    """A plain nn.Module whether or not pytorch_lightning is installed (the reference derives from pl.LightningModule, :115; the
    detector and the inference script use only `.model`, `.to` and the methods below)."""

    def __init__(self, model_name, token_name, image_size, chunk_size, descriptor_width_size, checkpoint_dir, patch_size=14,
                 validpatch_thresh=0.5):
        super().__init__()
        self.model_name = model_name
        self.model = _make_dinov2_model(arch_name=descriptor_map[model_name], patch_size=patch_size)
        self.checkpoint_dir = checkpoint_dir
        self.validpatch_thresh = validpatch_thresh
        self.token_name = token_name
        self.chunk_size = chunk_size
        self.patch_size = patch_size
        self.proposal_size = image_size
        self.descriptor_width_size = descriptor_width_size
        self.rgb_proposal_processor = CropResizePad(self.proposal_size)
        self.patch_kernel = torch.nn.AvgPool2d(kernel_size=self.patch_size, stride=self.patch_size)
        self._hip_weights = None

    # -- which path ------------------------------------------------------------------------------------------------
    def _use_hip(self, t):
        return (torch.is_tensor(t) and t.is_cuda and self.model_name == "dinov2_vitl14" and self.proposal_size == 224
                and self.patch_size == 14 and os.environ.get("SAM6D_HIP_DINOV2", "1") != "0")

    def _weights(self, dev):
        """The packed weights of self.model for `dev`; packed again when a parameter was replaced or written to."""
        sig = (str(dev),) + tuple((p.data_ptr(), p._version) for p in self.model.parameters())
        if self._hip_weights is None or self._hip_weights[0] != sig:
            from sam6d_hip import dinov2 as _d
            self._hip_weights = (sig, _d.DinoWeights(self.model.state_dict(), dev))
        return self._hip_weights[1]

    def rgb_normalize(self, image_np):
        """T.Compose([T.ToTensor(), T.Normalize(mean, std)]) of the reference (:144-149) without torchvision: (H, W, 3) uint8 ->
        (3, H, W) float32, u8 / 255 then (x - mean) / std."""
        img = torch.from_numpy(np.ascontiguousarray(image_np)) if not torch.is_tensor(image_np) else image_np
        if img.dtype == torch.uint8:
            img = img.permute(2, 0, 1).to(torch.float32).div(255)
        else:
            img = img.permute(2, 0, 1).to(torch.float32)
        mean = torch.as_tensor(_MEAN, dtype=torch.float32, device=img.device)[:, None, None]
        std = torch.as_tensor(_STD, dtype=torch.float32, device=img.device)[:, None, None]
        return (img - mean) / std

    @staticmethod
    def _u8(image_np):
        a = image_np if torch.is_tensor(image_np) else torch.from_numpy(np.ascontiguousarray(image_np))
        return a if a.dtype == torch.uint8 and a.dim() == 3 and a.shape[2] == 3 else None

    # -- dinov2.py:160-173 -------------------------------------------------------------------------------------------
    def process_rgb_proposals(self, image_np, masks, boxes):
        u8 = self._u8(image_np)
        from sam6d_hip import dinov2 as _d
        if self._use_hip(masks) and u8 is not None:
            return _d.crop_proposals(u8.to(masks.device), masks, boxes, mask=False)[0]
        # eager: the normalised image is gathered once per box and the gathered pixels are masked (no N copies of the image)
        m = masks[:, 0] if masks.dim() == 4 else masks
        return _d.crop_resize_pad(self.rgb_normalize(image_np).to(m.device), boxes, self.proposal_size, masks=m.float())

    # -- dinov2.py:221-232 -------------------------------------------------------------------------------------------
    def process_masks_proposals(self, masks, boxes):
        if masks.dim() == 3:
            masks.unsqueeze_(1)  # in place on the caller's tensor, as the reference does
        if self._use_hip(masks):
            from sam6d_hip import dinov2 as _d
            return _d.crop_proposals(None, masks, boxes, rgb=False)[1]
        return self.rgb_proposal_processor(masks.float(), boxes).squeeze_(1)

    def _process_both(self, image_np, proposals):
        u8 = self._u8(image_np)
        if self._use_hip(proposals.masks) and u8 is not None:  # one launch for crops and masks
            from sam6d_hip import dinov2 as _d
            rgbs, m224 = _d.crop_proposals(u8.to(proposals.masks.device), proposals.masks, proposals.boxes)
            if proposals.masks.dim() == 3:
                proposals.masks.unsqueeze_(1)
            return rgbs, m224
        rgbs = self.process_rgb_proposals(image_np, proposals.masks, proposals.boxes)
        return rgbs, self.process_masks_proposals(proposals.masks, proposals.boxes)

    # -- the encoder on a batch --------------------------------------------------------------------------------------
    def _features(self, images):
        """(x_norm_clstoken, x_norm_patchtokens) of images (N, 3, S, S)."""
        if self._use_hip(images):
            from sam6d_hip import dinov2 as _d
            return _d.encode(images.float(), self._weights(images.device))
        dev = next(self.model.parameters()).device
        cls, tok = [], []
        for i0 in range(0, images.shape[0], max(int(self.chunk_size), 1)):
            f = self.model.forward_features(images[i0:i0 + self.chunk_size].to(dev).float())
            cls.append(f["x_norm_clstoken"])
            tok.append(f["x_norm_patchtokens"])
        if not cls:
            d = self.model.embed_dim
            n = (images.shape[-1] // self.patch_size) ** 2
            return images.new_zeros((0, d), dtype=torch.float32), images.new_zeros((0, n, d), dtype=torch.float32)
        return torch.cat(cls).to(images.device), torch.cat(tok).to(images.device)

    def _mask_patches(self, patch_features, masks):
        if patch_features.is_cuda and self._use_hip(patch_features):
            from sam6d_hip import ism as _ism
            return _ism.masked_patch_features(patch_features, masks.to(patch_features.device), self.patch_size, self.validpatch_thresh)
        features_mask = self.patch_kernel(masks.float()).flatten(-2) > self.validpatch_thresh
        return F.normalize(patch_features * features_mask.unsqueeze(-1).to(patch_features.device), dim=-1)

    # -- dinov2.py:175-218 -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compute_features(self, images, token_name):
        if token_name != "x_norm_clstoken":
            raise NotImplementedError
        return self._features(images)[0]

    @torch.no_grad()
    def forward_by_chunk(self, processed_rgbs):
        return self.compute_features(processed_rgbs, token_name="x_norm_clstoken")

    @torch.no_grad()
    def forward_cls_token(self, image_np, proposals):
        return self.forward_by_chunk(self.process_rgb_proposals(image_np, proposals.masks, proposals.boxes))

    # -- dinov2.py:234-270 -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_patch_tokens(self, image_np, proposals):
        processed_rgbs, processed_masks = self._process_both(image_np, proposals)
        return self.forward_by_chunk_v2(processed_rgbs, processed_masks)

    @torch.no_grad()
    def forward_by_chunk_v2(self, processed_rgbs, masks):
        return self.compute_masked_patch_feature(processed_rgbs, masks)

    @torch.no_grad()
    def compute_masked_patch_feature(self, images, masks):
        return self._mask_patches(self._features(images)[1], masks)

    # -- dinov2.py:273-326 -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, image_np, proposals):
        processed_rgbs, processed_masks = self._process_both(image_np, proposals)
        return self.compute_cls_and_patch_features(processed_rgbs, processed_masks)

    @torch.no_grad()
    def compute_cls_and_patch_features(self, images, masks):
        cls_features, patch_features = self._features(images)
        return cls_features, self._mask_patches(patch_features, masks)
