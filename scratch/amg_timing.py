"""Timing of SAM's mask-generator tail on the GPU: the library path (sam6d_hip.amg) against eager_tail in PyTorch fp32, alternated in
one process, device events, median of repeated runs after warm-up.  The network is stubbed out (tests/sam_amg_stub.py), so the numbers
are the tail's alone.  Two cases: one 64-point batch (192 masks) and the whole tail of a 1024-point 480 x 640 image.

    python scratch/amg_timing.py [--reps 15] [--once]      (--once: a single library pass, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "openvino-sam-6d_amd", "ism")]
from sam6d_hip import amg  # noqa: E402
from tests.sam_amg_stub import StubSam  # noqa: E402

BOX, ORIG, S = [0, 0, 640, 480], (480, 640), 1024
SETTINGS = dict(mask_threshold=0.0, stability_score_offset=1.0, pred_iou_thresh=0.88, stability_score_thresh=0.85)


def batches(sam, n_batches):
    grid = amg.point_grid(32) * np.array([[640, 480]])
    out = []
    for b in range(n_batches):
        pts = grid[64 * b:64 * b + 64]
        coords = torch.as_tensor(amg.apply_coords(pts, ORIG, S), device=sam.device)
        low, iou = sam.mask_decoder(None, None, coords[:, None, :], None, True)
        out.append((low.contiguous(), iou.contiguous(), torch.as_tensor(pts).to(sam.device)))
    return out


def run_hip(bs):
    st = amg.CropState(BOX, ORIG, S, 64 * len(bs), bs[0][0].device, **SETTINGS)
    for low, iou, pts in bs:
        amg.process_batch(low, iou, st, pts)
    return amg.finish_crop(st, BOX, ORIG, 0.7)


def run_eager(bs):
    return amg.eager_tail(bs, BOX, ORIG, S, box_nms_thresh=0.7, **SETTINGS)


def timed(fn, bs):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn(bs)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (torch.cuda.max_memory_allocated() - base) / 2 ** 20, res["masks"].shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    sam = StubSam("cuda:0")
    if args.once:
        bs = batches(sam, 16)
        run_hip(bs)
        torch.cuda.synchronize()
        return
    for name, nb in (("one 64-point batch (192 masks)", 1), ("1024 points, 480 x 640 (16 batches, 3072 masks)", 16)):
        bs = batches(sam, nb)
        live = sum(int((iou > 0.88).sum()) for _, iou, _ in bs)
        for _ in range(3):
            timed(run_hip, bs), timed(run_eager, bs)
        t = {"hip": [], "eager": []}
        for _ in range(args.reps):  # alternated: both paths see the same clocks
            t["hip"].append(timed(run_hip, bs))
            t["eager"].append(timed(run_eager, bs))
        for k in ("eager", "hip"):
            ms = [x[0] for x in t[k]]
            print("%-50s %-6s median %8.3f ms  (min %8.3f, max %8.3f, %d runs)  peak %8.1f MiB  survivors %d  live %d" % (
                name, k, statistics.median(ms), min(ms), max(ms), len(ms), max(x[1] for x in t[k]), t[k][0][2], live))
        print("%-50s ratio eager / hip: %.1f" % (name, statistics.median([x[0] for x in t["eager"]]) / statistics.median([x[0] for x in t["hip"]])))


if __name__ == "__main__":
    main()
