"""Timing of sam6d_hip.refdata on the GPU: 42 templates of 512 x 512 from onboard.render_templates (an
icosphere of 1280 faces from the 42 fixture poses), wall clock between device synchronisations, two warm-up runs, median of the timed
runs with minimum and maximum, the two routes of a comparison ALTERNATED in one process.
  crops  refdata.template_boxes + template_crops (check=True: one read-back; and check=False) against the route a caller has today
         for the same step: rgb and mask to the host, PIL getbbox per mask, the literal torch operations and two eager
         crop_resize_pad calls on the host, the two results uploaded (ISM/run_inference_custom.py:132-155)
  build  refdata.build (one encoder pass) against today's whole route: the above plus compute_features and
         compute_masked_patch_feature of the drop-in CustomDINOv2 on the library (two encoder passes)
and the byte floor of the crop launch: 42 x 4 x 224 x 224 floats written.

    python scratch/refdata_timing.py [--reps 9]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openvino-sam-6d_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(PKG, "ism")]
from sam6d_hip import dinov2, onboard, refdata  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)

DEV = "cuda:0"


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    del res
    return (time.perf_counter() - t0) * 1e3


def alternated(routes, reps):
    """routes: [(name, fn)]; every repetition runs each route once, in turn"""
    for _ in range(2):
        for _, fn in routes:
            wall_ms(fn)
    t = {name: [] for name, _ in routes}
    for _ in range(reps):
        for name, fn in routes:
            t[name].append(wall_ms(fn))
    for name, _ in routes:
        print("%-72s median %9.3f ms  (min %9.3f, max %9.3f)" % (name, statistics.median(t[name]), min(t[name]), max(t[name])), flush=True)


def todays_crops(rgb, mask):
    """ISM/run_inference_custom.py:132-155 from tensors on the device: download, PIL, two eager crops on the host, upload"""
    from PIL import Image
    rgb_h, mask_h = rgb.cpu().numpy(), mask.cpu().numpy()
    boxes, masks, templates = [], [], []
    for t in range(rgb_h.shape[0]):
        m = Image.fromarray(mask_h[t], "L")
        boxes.append(m.getbbox())
        image = torch.from_numpy(rgb_h[t] / 255).float()
        mk = torch.from_numpy(np.array(m) / 255).float()
        templates.append(image * mk[:, :, None])
        masks.append(mk.unsqueeze(-1))
    templates = torch.stack(templates).permute(0, 3, 1, 2)
    masks = torch.stack(masks).permute(0, 3, 1, 2)
    boxes = torch.tensor(np.array(boxes))
    return dinov2.crop_resize_pad(templates, boxes).to(rgb.device), dinov2.crop_resize_pad(masks, boxes).to(rgb.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    poses = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
    v, f = RR.icosphere(3, 50.0)
    out = onboard.render_templates(dict(vertices=v, faces=f), poses)
    rgb, mask = out["rgb"], out["mask"]
    T = rgb.shape[0]
    print("templates: rgb %s, mask %s, %.1f %% of the pixels set" % (tuple(rgb.shape), tuple(mask.shape), 100.0 * float((mask != 0).float().mean())))
    a, b = refdata.template_crops(rgb, mask), todays_crops(rgb, mask)
    print("crops of the two routes equal: rgb %s, mask %s" % (torch.equal(a[0], b[0]), torch.equal(a[1], b[1][:, 0])))
    alternated([("template_boxes", lambda: refdata.template_boxes(mask)),
                ("template_boxes + template_crops, check=False", lambda: refdata.template_crops(rgb, mask, check=False)),
                ("template_boxes + template_crops, check=True (one read-back)", lambda: refdata.template_crops(rgb, mask)),
                ("today: download, PIL getbbox, two eager crop_resize_pad, upload", lambda: todays_crops(rgb, mask))], args.reps)
    written = T * 4 * 224 * 224 * 4
    print("crop launch writes %d bytes: %.1f us at 6.3 TB/s (the achievable HBM rate)" % (written, written / 6.3e12 * 1e6))

    from model.dinov2 import CustomDINOv2
    d = CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused").eval()
    W = dinov2.DinoWeights(d.model.state_dict(), DEV)
    d.model.to(DEV)
    obj_poses, points = np.tile(np.eye(4), (T, 1, 1)), np.zeros((2048, 3), np.float32)

    def today():
        templates, masks = todays_crops(rgb, mask)
        return (d.compute_features(templates, token_name="x_norm_clstoken").unsqueeze(0),
                d.compute_masked_patch_feature(templates, masks[:, 0]).unsqueeze(0))

    alternated([("refdata.build (one encoder pass)", lambda: refdata.build(rgb, mask, W, obj_poses, points)),
                ("today: host crops + compute_features + compute_masked_patch_feature", today)], args.reps)


if __name__ == "__main__":
    main()
