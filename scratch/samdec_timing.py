"""Timing of SAM's prompt encoder + mask decoder on the GPU: the library path (sam6d_hip.samdec.predict_low) against the package's eager
fp32 partner (samdec.eager: the reference's sequence of torch ops), alternated in one process, device events, median of repeated runs
after warm-up.  Seeded full-width weights (tests/sam_decoder_ref.seeded_weights), the image encoder stubbed out.  Cases: predict_low at
P = 64 and P = 1, and generate_masks with 1024 points on a 480 x 640 image (decoder on the library / eager, the tail on the library in
both).

    python scratch/samdec_timing.py [--reps 15] [--mode 1] [--once]     (--once: one library pass at P = 64, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "openvino-sam-6d_amd", "ism")]
from sam6d_hip import amg, samdec  # noqa: E402
from sam6d_hip.pem import Options  # noqa: E402
from tests.sam_decoder_stub import StubSamNetwork, encode_image  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def compare(name, lib, eager, reps):
    for _ in range(3):
        timed(lib), timed(eager)
    t = {"library": [], "eager": []}
    for _ in range(reps):  # alternated: both paths see the same clocks
        t["library"].append(timed(lib))
        t["eager"].append(timed(eager))
    for k in ("eager", "library"):
        ms = [x[0] for x in t[k]]
        print("%-46s %-8s median %8.3f ms  (min %8.3f, max %8.3f, %d runs)  peak %8.1f MiB" % (name, k, statistics.median(ms), min(ms), max(ms),
                                                                                              len(ms), max(x[1] for x in t[k])))
    print("%-46s ratio eager / library: %.2f" % (name, statistics.median([x[0] for x in t["eager"]]) / statistics.median([x[0] for x in t["library"]])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--mode", type=int, default=1)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    sam = StubSamNetwork("cuda:0", seed=20250117)
    W = sam.eager_weights()
    opt = Options(matmul_mode=args.mode)
    grid = amg.point_grid(32) * np.array([[640, 480]])
    pts = torch.as_tensor(amg.apply_coords(grid, (480, 640), 1024), device=sam.device)
    tables = samdec.image_tables(sam.features, W, options=opt)
    if args.once:
        samdec.predict_low(pts[:64], tables, W, options=opt)
        torch.cuda.synchronize()
        samdec.predict_low(pts[:64], tables, W, options=opt)
        torch.cuda.synchronize()
        return
    with torch.no_grad():
        for P in (64, 1):
            compare("predict_low, P = %d, matmul mode %d" % (P, args.mode), lambda: samdec.predict_low(pts[:P], tables, W, options=opt),
                    lambda: samdec.eager(pts[:P], sam.features, W), args.reps)
        compare("image_tables (once per set_image)", lambda: samdec.image_tables(sam.features, W, options=opt), lambda: None, args.reps)
        mod = importlib.import_module("model.sam")
        image = np.zeros((480, 640, 3), dtype=np.uint8)
        gens = {on: mod.CustomSamAutomaticMaskGenerator(sam, pred_iou_thresh=0.0, stability_score_thresh=0.6, encode_image=encode_image,
                                                        hip_decoder=on) for on in (True, False)}
        prev = os.environ.get("SAM6D_MATMUL_MODE")
        os.environ["SAM6D_MATMUL_MODE"] = str(args.mode)
        compare("generate_masks, 1024 points, 480 x 640", lambda: gens[True].generate_masks(image), lambda: gens[False].generate_masks(image),
                args.reps)
        if prev is None:
            del os.environ["SAM6D_MATMUL_MODE"]


if __name__ == "__main__":
    main()
