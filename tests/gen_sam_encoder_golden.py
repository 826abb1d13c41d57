"""Regenerates tests/golden/sam_encoder_small.npz from the reference implementation.

Run by hand where the reference checkout is available (REFERENCE_ROOT, default /root/reference); never imported by a test.  It imports
the reference's segment_anything/modeling/{common,image_encoder}.py (they import only torch) under a package name of their own, so that
segment_anything/__init__.py does not run, and stores only data: the seeds of the weights and of the input (tests/sam_encoder_ref.py
makes both), the geometry, and the output of the reference's ImageEncoderViT run unchanged in .double().

    python tests/gen_sam_encoder_golden.py

The geometry is small but has every case: width 32, 2 heads, depth 2 with block 1 global, image 320 (a 20 x 20 grid, padded to 28 x 28
for the 14 x 14 windows of block 0, so padded windows occur), neck to 8 channels.  The seeded weights randomise rel_pos_h / _w and
pos_embed, which the reference initialises to zero.
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

SMALL = dict(dim=32, heads=2, depth=2, global_blocks=(1,), grid=20, window=14, patch=16, out=8)
SEED, INPUT_SEED = 20250301, 20250302


def load_reference():
    pkg = types.ModuleType("refsam_modeling")
    pkg.__path__ = [MODELING]
    sys.modules["refsam_modeling"] = pkg
    return {n: importlib.import_module("refsam_modeling." + n) for n in ("common", "image_encoder")}


def main():
    from tests import sam_encoder_ref as R
    ref = load_reference()
    c = SMALL
    enc = ref["image_encoder"].ImageEncoderViT(
        img_size=c["grid"] * c["patch"], patch_size=c["patch"], embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"], mlp_ratio=4.0,
        out_chans=c["out"], qkv_bias=True, norm_layer=lambda n: torch.nn.LayerNorm(n, eps=1e-6), use_abs_pos=True, use_rel_pos=True,
        rel_pos_zero_init=True, window_size=c["window"], global_attn_indexes=c["global_blocks"]).eval()
    sd = R.seeded_weights(SEED, **c)
    enc.load_state_dict(sd, strict=True)
    x = R.seeded_input(INPUT_SEED, c["grid"] * c["patch"])
    with torch.no_grad():
        out = enc.double()(x.double())
    assert out.dtype == torch.float64 and tuple(out.shape) == (1, c["out"], c["grid"], c["grid"])
    data = dict(seed=np.int64(SEED), input_seed=np.int64(INPUT_SEED), out=out.numpy(),
                # two sums that a change of the seeded generators would move
                weight_sum=np.float64(sum(float(v.double().sum()) for v in sd.values())), input_sum=np.float64(float(x.double().sum())),
                **{"cfg_" + k: np.array(v) for k, v in c.items()})
    path = os.path.join(GOLD, "sam_encoder_small.npz")
    np.savez_compressed(path, **data)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1_000_000, "fixture too large"


if __name__ == "__main__":
    main()
