"""Regenerates tests/golden/dinov2_small.npz and tests/golden/crop_resize_pad.npz from the reference implementation.

Run by hand where the reference checkout is available (REFERENCE_ROOT, default /root/reference); never imported by a test.  It
imports the reference's ISM/model/vision_transformer.py and ISM/utils/bbox_utils.py (with empty stand-ins for the packages they
import and this path does not touch: segment_anything, torchvision) and stores only data: weights, inputs, outputs, names.

    python tests/gen_dinov2_golden.py
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
ISM = os.path.join(REF, "SAM-6D", "Instance_Segmentation_Model")
GOLD = os.path.join(ROOT, "tests", "golden")

# The boxes of crop_resize_pad.npz on a 300 x 400 coordinate image (pixel value = its own linear index), xyxy with exclusive ends.
# scale_factor is `224 / tensor`, which torch evaluates as tensor.reciprocal() * 224 in float32 (Tensor.__rtruediv__), not as one
# division.  Long sides whose resized length floor(L * scale_factor) comes out as 223 (found by `sides_223` below): 19, 41, 97, 103,
# 113, 131 ...; for L = 3 and L = 41 the two ways of forming the scale factor differ in the last bit (and for 3 in the resized length).
IMG_H, IMG_W = 300, 400
BOXES = [
    (10, 20, 110, 120, "square 100"),
    (50, 60, 250, 130, "wide 200 x 70"),
    (120, 10, 180, 290, "tall 60 x 280 (larger than 224)"),
    (30, 40, 31, 140, "one pixel thin, tall"),
    (60, 200, 200, 201, "one pixel thin, wide"),
    (0, 0, 90, 50, "touches top and left"),
    (340, 250, 400, 300, "touches bottom and right"),
    (0, 100, 400, 180, "full width (400 > 224)"),
    (100, 0, 170, 300, "full height"),
    (20, 30, 244, 150, "long side exactly 224"),
    (20, 30, 120, 254, "long side exactly 224, tall"),
    (5, 5, 305, 295, "larger than 224 both ways"),
    (200, 100, 219, 112, "long side 19 -> 223"),
    (100, 50, 197, 130, "long side 97 -> 223"),
    (40, 100, 100, 203, "long side 103 -> 223, tall"),
    (150, 150, 263, 263, "square 113 -> 223 x 223: no padding, second resize 223 -> 224"),
    (10, 160, 141, 200, "long side 131 -> 223"),
    (7, 9, 10, 12, "square 3 -> 224 (223 if the scale factor were one division)"),
    (300, 20, 341, 50, "long side 41 -> 223"),
]


def sides_223(limit=400):
    return [L for L in range(1, limit) if math.floor(L * float(224 / torch.tensor(L))) == 223]


def _stub(name):
    m = types.ModuleType(name)
    m.__path__ = []
    sys.modules[name] = m
    return m


def load_reference():
    """The reference's vision_transformer and bbox_utils modules, imported under a package name of their own so that the
    reference's model/__init__.py (which pulls the whole detector) does not run."""
    for name in ("segment_anything", "segment_anything.utils", "segment_anything.utils.transforms", "torchvision",
                 "torchvision.transforms", "torchvision.transforms.functional"):
        if name not in sys.modules:
            _stub(name)
    sys.modules["segment_anything.utils.transforms"].ResizeLongestSide = object
    sys.modules["torchvision.transforms.functional"].resize = None
    sys.modules["torchvision.transforms.functional"].to_pil_image = None
    pkg = _stub("refism_model")
    pkg.__path__ = [os.path.join(ISM, "model")]
    upkg = _stub("refism_utils")
    upkg.__path__ = [os.path.join(ISM, "utils")]
    vt = importlib.import_module("refism_model.vision_transformer")
    bb = importlib.import_module("refism_utils.bbox_utils")
    return vt, bb


def _coarse(t):
    """Random values on a grid of 1 / 256 (exactly representable in float32): the fixture compresses to a quarter of its size."""
    return torch.round(t * 256.0) / 256.0


def make_small(vt):
    torch.manual_seed(20240611)
    m = vt.DinoVisionTransformer(img_size=518, patch_size=14, embed_dim=64, depth=2, num_heads=1, init_values=1.0, block_chunks=0)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("gamma"):
                v = 1.0 + 0.3 * torch.randn(p.shape, generator=g)
            elif name.endswith("weight") and p.dim() >= 2:
                v = torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel())
            elif "norm" in name and name.endswith("weight"):
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            elif name == "pos_embed":
                v = 0.2 * torch.randn(p.shape, generator=g)
            else:
                v = 0.1 * torch.randn(p.shape, generator=g)
            p.copy_(_coarse(v))
    m.eval()
    # two structured (compressible) images: 7 x 7 blocks of random levels plus gradients
    blocks = torch.randint(0, 256, (2, 32, 32, 3), generator=g)
    yy, xx = torch.meshgrid(torch.arange(224), torch.arange(224), indexing="ij")
    img = blocks.repeat_interleave(7, 1).repeat_interleave(7, 2) + (3 * xx + 5 * yy)[None, :, :, None] + torch.tensor([0, 40, 90])
    images = (img % 256).to(torch.uint8)
    x = images.permute(0, 3, 1, 2).to(torch.float32).div(255)
    mean = torch.tensor((0.485, 0.456, 0.406))[:, None, None]
    std = torch.tensor((0.229, 0.224, 0.225))[:, None, None]
    x = (x - mean) / std
    sd32 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        pos32 = m.interpolate_pos_encoding(torch.zeros(1, 257, 64), 224, 224).detach().clone()
        m64 = m.double()
        f = m64.forward_features(x.double())
    out = {"sd." + k: v.numpy() for k, v in sd32.items()}
    out.update(images=images.numpy(), x_norm_clstoken=f["x_norm_clstoken"].numpy(), x_norm_patchtokens=f["x_norm_patchtokens"].numpy(),
               pos_interpolated=pos32.numpy(), num_heads=np.int64(1))
    # names and shapes of the full model the drop-in must reproduce
    big = vt.vit_large(patch_size=14, img_size=518, init_values=1.0, block_chunks=0)
    items = sorted((k, tuple(v.shape)) for k, v in big.state_dict().items())
    out["vitl14_names"] = np.array([k for k, _ in items])
    out["vitl14_shapes"] = np.array([",".join(str(d) for d in s) for _, s in items])
    return out


def make_crops(bb):
    coord = torch.arange(IMG_H * IMG_W, dtype=torch.float32).reshape(1, 1, IMG_H, IMG_W)
    boxes = torch.tensor([b[:4] for b in BOXES], dtype=torch.long)
    got = bb.CropResizePad(224)(coord.expand(len(BOXES), -1, -1, -1), boxes)
    assert tuple(got.shape) == (len(BOXES), 1, 224, 224)
    longs = (boxes[:, 2:] - boxes[:, :2]).max(dim=1)[0]
    resized = [math.floor(int(L) * float(224 / L)) for L in longs]
    assert sum(r == 223 for r in resized) >= 3, resized
    return dict(height=np.int64(IMG_H), width=np.int64(IMG_W), boxes=boxes.numpy(), out=got[:, 0].numpy().astype(np.int32),
                resized_long_side=np.array(resized), notes=np.array([b[4] for b in BOXES]))


def main():
    vt, bb = load_reference()
    print("long sides that resize to 223:", sides_223()[:60])
    for name, data in (("dinov2_small.npz", make_small(vt)), ("crop_resize_pad.npz", make_crops(bb))):
        path = os.path.join(GOLD, name)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print("%s: %d bytes" % (path, size))
        assert size < 1_000_000, "fixture too large"


if __name__ == "__main__":
    main()
