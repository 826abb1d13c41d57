"""Regenerates tests/golden/sam_decoder_small.npz and tests/golden/sam_decoder_full.npz from the reference implementation.

Run by hand where the reference checkout is available (REFERENCE_ROOT, default /root/reference); never imported by a test.  It imports
the reference's segment_anything/modeling/{common,transformer,mask_decoder,prompt_encoder}.py (they import only torch and numpy) under a
package name of their own, so that segment_anything/__init__.py (which pulls the image encoder and torchvision) does not run, and
stores only data: weights, inputs, outputs.

    python tests/gen_sam_decoder_golden.py

PromptEncoder runs in float32 as the reference runs it (it casts the coordinates to float itself); MaskDecoder with its
TwoWayTransformer runs unchanged in .double() on those float32 embeddings.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
MODELING = os.path.join(REF, "SAM-6D", "Instance_Segmentation_Model", "segment_anything", "modeling")
GOLD = os.path.join(ROOT, "tests", "golden")

FULL_SEED, FULL_FEATURE_SEED, FULL_PIXEL_SEED = 20250117, 20250118, 20250119
FULL_POINTS = [[311.25, 407.5], [1023.0, 767.0]]  # input frame of a 480 x 640 image (768 x 1024); the second is its far corner


def load_reference():
    pkg = types.ModuleType("refsam_modeling")
    pkg.__path__ = [MODELING]
    sys.modules["refsam_modeling"] = pkg
    return {n: importlib.import_module("refsam_modeling." + n) for n in ("common", "transformer", "mask_decoder", "prompt_encoder")}


def build(ref, dim, heads, mlp_dim, grid, input_size, mask_in_chans):
    pe = ref["prompt_encoder"].PromptEncoder(embed_dim=dim, image_embedding_size=grid, input_image_size=input_size, mask_in_chans=mask_in_chans)
    md = ref["mask_decoder"].MaskDecoder(
        num_multimask_outputs=3,
        transformer=ref["transformer"].TwoWayTransformer(depth=2, embedding_dim=dim, mlp_dim=mlp_dim, num_heads=heads),
        transformer_dim=dim, iou_head_depth=3, iou_head_hidden_dim=dim)
    return pe.eval(), md.eval()


def run(pe, md, points, features):
    """-> sparse (P, 2, C) f32, dense_pe (1, C, h, w) f32, low (P, 3, 4h, 4w) f64, iou (P, 3) f64."""
    with torch.no_grad():
        labels = torch.ones(points.shape[0], dtype=torch.int)
        sparse, dense = pe(points=(points[:, None, :], labels[:, None]), boxes=None, masks=None)
        dense_pe = pe.get_dense_pe()
        assert sparse.dtype == torch.float32 and dense_pe.dtype == torch.float32
        low, iou = md.double()(image_embeddings=features.double(), image_pe=dense_pe.double(), sparse_prompt_embeddings=sparse.double(),
                               dense_prompt_embeddings=dense.double(), multimask_output=True)
        md.float()
    return sparse, dense_pe, low, iou


def _coarse(t):
    """Random values on a grid of 1 / 256 (exactly representable in float32): the fixture compresses well."""
    return torch.round(t * 256.0) / 256.0


def make_small(ref):
    dim, heads, mlp_dim, grid, input_size = 32, 2, 64, (8, 8), (128, 128)
    torch.manual_seed(20250116)
    pe, md = build(ref, dim, heads, mlp_dim, grid, input_size, 16)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for mod in (pe, md):
            for name, p in list(mod.named_parameters()) + list(mod.named_buffers()):
                if name.endswith("gaussian_matrix"):
                    v = torch.randn(p.shape, generator=g)
                elif "norm" in name or name.startswith("output_upscaling.1"):
                    v = (1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g)
                elif p.dim() >= 2 and p.shape[0] > 4:
                    v = torch.randn(p.shape, generator=g) / (p.shape[1] if p.dim() == 2 else p.shape[0]) ** 0.5
                else:
                    v = 0.3 * torch.randn(p.shape, generator=g)
                p.copy_(_coarse(v))
    points = torch.tensor([[17.0, 90.5], [0.0, 0.0], [127.0, 127.0]], dtype=torch.float64)
    features = _coarse(torch.randn((1, dim) + grid, generator=g))
    sparse, dense_pe, low, iou = run(pe, md, points, features)
    out = {"psd." + k: v.numpy() for k, v in pe.state_dict().items() if not k.startswith("mask_downscaling")}
    out.update({"dsd." + k: v.numpy() for k, v in md.state_dict().items()})
    out.update(points=points.numpy(), features=features.numpy(), sparse=sparse.numpy(), dense_pe=dense_pe.numpy(), low=low.numpy(),
               iou=iou.numpy(), num_heads=np.int64(heads), input_size=np.array(input_size), grid=np.array(grid))
    return out


def make_full(ref):
    from tests import sam_decoder_ref as R
    pe, md = build(ref, 256, 8, 2048, (64, 64), (1024, 1024), 16)
    psd, dsd = R.seeded_weights(FULL_SEED)
    missing = pe.load_state_dict(psd, strict=False)
    assert all(k.startswith("mask_downscaling") for k in missing.missing_keys) and not missing.unexpected_keys
    md.load_state_dict(dsd, strict=True)
    points = torch.tensor(FULL_POINTS, dtype=torch.float64)
    features = R.seeded_features(FULL_FEATURE_SEED)
    sparse, dense_pe, low, iou = run(pe, md, points, features)
    idx = torch.randperm(256 * 256, generator=torch.Generator().manual_seed(FULL_PIXEL_SEED))[:4096].sort()[0]
    return dict(seed=np.int64(FULL_SEED), feature_seed=np.int64(FULL_FEATURE_SEED), points=points.numpy(), pixels=idx.numpy(),
                low_at_pixels=low.flatten(2)[:, :, idx].numpy(), iou=iou.numpy(), sparse=sparse.numpy(),
                dense_pe_at_pixels=dense_pe.flatten(2)[0, :, idx[:64] % 4096].numpy(), pe_tokens=(idx[:64] % 4096).numpy())


def main():
    ref = load_reference()
    for name, data in (("sam_decoder_small.npz", make_small(ref)), ("sam_decoder_full.npz", make_full(ref))):
        path = os.path.join(GOLD, name)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print("%s: %d bytes" % (path, size))
        assert size < 400_000, "fixture too large"


if __name__ == "__main__":
    main()
