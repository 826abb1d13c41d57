"""Regenerates tests/golden/sam_amg.npz from the reference implementation.

Run by hand where the reference checkout is available (REFERENCE_ROOT, default /root/reference); never imported by a test.  It loads
the reference's segment_anything/modeling/sam.py (for Sam.postprocess_masks), segment_anything/utils/amg.py and
segment_anything/utils/transforms.py by path, with empty stand-ins for the sibling modules and torchvision that this path does not touch,
and stores only data: the parameters of the logits (tests/sam_amg_ref.py builds them exactly), geometry, and the reference's results.

    python tests/gen_sam_amg_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sam_amg_ref as R  # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
SA = os.path.join(REF, "SAM-6D", "Instance_Segmentation_Model", "segment_anything")
GOLD = os.path.join(ROOT, "tests", "golden")

S = 1024
THR, OFFSET = 0.0, 1.0
PRED_IOU_THRESH, STABILITY_THRESH = 0.88, 0.85
EPS_GEN = 1.5e-4     # the band the generator checks the inputs with (the GPU test measures its own, near 1.2e-4)
STRIDE = 16         # the float64 reference logits are kept at every 16th pixel

# (orig_h, orig_w, crop_box xyxy)
CASES = [
    (480, 640, (0, 0, 640, 480)),      # the shipped size: input 768 x 1024
    (640, 480, (0, 0, 480, 640)),      # portrait
    (900, 1200, (0, 0, 1200, 900)),    # long side above the encoder's 1024
    (480, 640, (140, 100, 500, 370)),  # an inner crop box, 270 x 360
]
# cx, cy, kx, ky, a -- see sam_amg_ref.build_logits
MASKS = [
    (128, 100, 30, 40, 300),   # sharp ellipse: kept
    (60, 60, 4, 4, 50),        # soft blob: low stability
    (0, 0, 0, 0, -70),         # empty
    (0, 0, 0, 0, 100),         # full
    (128, 96, 6, 10, 400),     # an ellipse larger than the 256 x 192 window: reaches all four borders, leaves the corners out
    (150, 60, 50, 50, 200),    # sharp, but its predicted IoU is below the filter
]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_modules():
    _stub("segment_anything")
    _stub("segment_anything.modeling")
    _stub("segment_anything.modeling.image_encoder", ImageEncoderViT=object)
    _stub("segment_anything.modeling.mask_decoder", MaskDecoder=object)
    _stub("segment_anything.modeling.prompt_encoder", PromptEncoder=object)
    _stub("torchvision")
    _stub("torchvision.transforms")
    _stub("torchvision.transforms.functional", resize=None, to_pil_image=None)
    sam = _load("segment_anything.modeling.sam", os.path.join(SA, "modeling", "sam.py"))
    _stub("segment_anything.utils")
    amg = _load("segment_anything.utils.amg", os.path.join(SA, "utils", "amg.py"))
    tr = _load("segment_anything.utils.transforms", os.path.join(SA, "utils", "transforms.py"))
    return sam, amg, tr


def main():
    sam, amg, tr = reference_modules()
    fake = types.SimpleNamespace(image_encoder=types.SimpleNamespace(img_size=S))
    out = dict(S=np.int64(S), thr=np.float64(THR), offset=np.float64(OFFSET), pred_iou_thresh=np.float64(PRED_IOU_THRESH),
               stability_thresh=np.float64(STABILITY_THRESH), eps_gen=np.float64(EPS_GEN), stride=np.int64(STRIDE),
               cases=np.array([[h, w, *b] for h, w, b in CASES], dtype=np.int64), params=np.array(MASKS, dtype=np.int32))
    worst = 0.0
    for c, (H, W, box) in enumerate(CASES):
        M = len(MASKS)
        seeds = np.arange(M, dtype=np.int64) + 16 * c
        low = torch.from_numpy(R.build_logits(MASKS, seeds))
        iou = torch.tensor([0.90 + 0.01 * m + 0.001 * c for m in range(M)], dtype=torch.float32)
        iou[5] = 0.5
        x0, y0, x1, y1 = box
        crop = (y1 - y0, x1 - x0)
        inp = tr.ResizeLongestSide.get_preprocess_shape(crop[0], crop[1], S)
        assert tuple(inp) == R.preprocess_shape(crop[0], crop[1], S)
        lg32 = sam.Sam.postprocess_masks(fake, low[None], inp, crop)[0]
        lg64 = sam.Sam.postprocess_masks(fake, low[None].double(), inp, crop)[0].numpy()
        mine = R.postprocess_masks(low.numpy(), inp, crop, S)
        assert np.abs(mine - lg64).max() <= 1e-11, np.abs(mine - lg64).max()
        dev32 = float(np.abs(lg32.double().numpy() - lg64).max())
        worst = max(worst, R.check_cap(lg64, (THR, THR + OFFSET, THR - OFFSET), EPS_GEN))
        assert R.stability_decided(lg64, THR, OFFSET, STABILITY_THRESH, EPS_GEN).all(), "a mask's stability decision is not robust"
        stab = amg.calculate_stability_score(lg32, THR, OFFSET)
        masks = lg32 > THR
        boxes = amg.batched_mask_to_box(masks)
        edge = amg.is_box_near_crop_edge(boxes, list(box), [0, 0, W, H])
        full = amg.uncrop_masks(masks, list(box), H, W)
        rles = amg.mask_to_rle_pytorch(full)
        counts, offsets = [], [0]
        for m, rle in enumerate(rles):
            assert np.array_equal(amg.rle_to_mask(rle), full[m].numpy())
            assert rle["counts"] == R.rle_encode(full[m].numpy())
            counts += rle["counts"]
            offsets.append(len(counts))
        p = "c%d." % c
        out.update({
            p + "seeds": seeds, p + "iou_preds": iou.numpy(), p + "input_size": np.array(inp, dtype=np.int64),
            p + "n_hi": (lg32 > THR + OFFSET).sum((1, 2)).numpy(), p + "n_lo": (lg32 > THR - OFFSET).sum((1, 2)).numpy(),
            p + "area": masks.sum((1, 2)).numpy(), p + "stability": stab.numpy(), p + "boxes": boxes.numpy(),
            p + "keep_iou": (iou > PRED_IOU_THRESH).numpy(), p + "keep_stability": (stab >= STABILITY_THRESH).numpy(),
            p + "keep_edge": (~edge).numpy(), p + "rle_counts": np.array(counts, dtype=np.int32), p + "rle_offsets": np.array(offsets, dtype=np.int64),
            p + "logits64_sample": lg64[:, ::STRIDE, ::STRIDE].copy(), p + "fp32_deviation": np.float64(dev32),
        })
        print("case %d: %dx%d crop %s input %s  fp32 dev %.2e  stab %s  keep iou/stab/edge %s %s %s" % (
            c, H, W, box, tuple(inp), dev32, np.round(stab.numpy(), 3), out[p + "keep_iou"].astype(int), out[p + "keep_stability"].astype(int),
            out[p + "keep_edge"].astype(int)))
    out["worst_band_fraction"] = np.float64(worst)
    # geometry captured from the reference's own helpers
    out["grid4"] = amg.build_point_grid(4)
    out["grid32"] = amg.build_point_grid(32)
    for name, (size, layers) in {"crops_480x640_l1": ((480, 640), 1), "crops_480x640_l2": ((480, 640), 2), "crops_900x1200_l1": ((900, 1200), 1)}.items():
        b, li = amg.generate_crop_boxes(size, layers, 512 / 1500)
        out[name] = np.array([bb + [l] for bb, l in zip(b, li)], dtype=np.int64)
    pts = amg.build_point_grid(8) * np.array([[640, 480]])
    t = tr.ResizeLongestSide(S)
    for name, size in {"coords_480x640": (480, 640), "coords_270x360": (270, 360), "coords_900x1200": (900, 1200), "coords_333x517": (333, 517)}.items():
        out[name] = t.apply_coords(pts, size)
        out[name + "_shape"] = np.array(t.get_preprocess_shape(size[0], size[1], S), dtype=np.int64)
    out["coords_points"] = pts
    path = os.path.join(GOLD, "sam_amg.npz")
    np.savez_compressed(path, **out)
    print("worst band fraction at eps %.0e: %.2e;  %s: %d bytes" % (EPS_GEN, worst, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
