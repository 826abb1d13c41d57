"""Timing of SAM's min_mask_region_area clean-up on the GPU: the library path (sam6d_hip.amg.remove_small_regions and
postprocess_small_regions) against the host route the reference takes (download, connected components per mask twice on the host,
upload, boxes, NMS), alternated in one process, wall clock between device synchronisations, median of repeated runs after warm-up.
The host labeller is cv2 where it imports (the reference's own), else scipy.ndimage.label, else the numpy restatement of the tests; the
output says which.  Cases: 100 and 300 blob masks at 480 x 640 with min_area 100, and 100 coin-flip masks (the most runs and unions).

    python scratch/small_regions_timing.py [--reps 9] [--host-reps 3] [--once]   (--once: one library pass, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "openvino-sam-6d_amd", "ism")]
from sam6d_hip import amg  # noqa: E402
from tests import small_regions_ref as R  # noqa: E402

H, W, MIN_AREA, NMS_THRESH = 480, 640, 100, 0.7


def host_labeller():
    """-> (name, f(mask bool (H, W)) -> (labels int (H, W) with 0 off the mask, sizes per label with sizes[0] unused))."""
    try:
        import cv2

        def f(m):
            _, regions, stats, _ = cv2.connectedComponentsWithStats(m.astype(np.uint8), 8)
            return regions, stats[:, -1]
        return "cv2", f
    except ImportError:
        pass
    try:
        from scipy import ndimage

        def f(m):
            lab, n = ndimage.label(m, structure=R.NEIGHBOURS_8)
            return lab, np.bincount(lab.ravel(), minlength=n + 1)
        return "scipy", f
    except ImportError:
        pass

    def f(m):
        labels, _, first, size = R.components(m)
        return np.searchsorted(first + 1, labels, side="right") * (labels > 0), np.concatenate([[0], size])
    return "numpy restatement", f


def host_route(data, label):
    """The drop-in's host route (ism/model/sam.py postprocess_small_regions) with `label` in cv2's place."""
    def clean(mask, holes):
        work = holes ^ mask
        regions, sizes = label(work)
        sizes = sizes[1:]
        small = np.nonzero(sizes < MIN_AREA)[0] + 1
        if len(small) == 0:
            return mask, False
        fill = np.concatenate([[0], small])
        if not holes:
            fill = np.setdiff1d(np.arange(len(sizes) + 1), fill)
            if len(fill) == 0:
                fill = np.array([int(np.argmax(sizes)) + 1])
        return np.isin(regions, fill), True

    dev = data["masks"].device
    new_masks, scores = [], []
    for mask in data["masks"].bool().cpu().numpy():
        mask, c1 = clean(mask, True)
        mask, c2 = clean(mask, False)
        new_masks.append(torch.as_tensor(mask))
        scores.append(float(not (c1 or c2)))
    masks = torch.stack(new_masks).to(dev)
    boxes = amg.mask_boxes(masks)
    scores = torch.as_tensor(scores, device=dev)
    keep = amg.nms_torch(boxes.float(), scores, NMS_THRESH)
    out_boxes = data["boxes"].clone()
    out_boxes[scores == 0.0] = boxes[scores == 0.0]
    return {"masks": masks[keep], "boxes": out_boxes[keep]}


def blob_masks(n, base=16):
    """n blob masks from `base` generated ones, shifted cyclically so that no two are equal."""
    b = [R.blobs(H, W, 100 + i, k=15) for i in range(base)]
    return np.stack([np.roll(b[i % base], (7 * (i // base), 13 * (i // base)), axis=(0, 1)) for i in range(n)])


def coin_masks(n, base=8):
    b = [R.coin(H, W, 200 + i) for i in range(base)]
    return np.stack([np.roll(b[i % base], (5 * (i // base), 3 * (i // base)), axis=(0, 1)) for i in range(n)])


def timed(fn, arg):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    res = fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20, res


def line(case, name, runs):
    ms = [r[0] for r in runs]
    print("%-34s %-28s median %10.3f ms  (min %10.3f, max %10.3f, %2d runs)  peak %8.1f MiB" % (
        case, name, statistics.median(ms), min(ms), max(ms), len(ms), max(r[1] for r in runs)), flush=True)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lname, label = host_labeller()
    print("host labeller: %s" % lname, flush=True)
    cases = [("100 blob masks 480x640", blob_masks(100)), ("300 blob masks 480x640", blob_masks(300)), ("100 coin-flip masks 480x640", coin_masks(100))]
    if args.once:
        m = torch.from_numpy(cases[0][1]).to(dev)
        amg.remove_small_regions(m, MIN_AREA)
        torch.cuda.synchronize()
        return
    for case, masks in cases:
        m = torch.from_numpy(masks).to(dev)
        data = {"masks": m, "boxes": amg.mask_boxes(m)}
        clean = lambda x: amg.remove_small_regions(x["masks"], MIN_AREA)            # noqa: E731
        post = lambda x: amg.postprocess_small_regions(x, MIN_AREA, NMS_THRESH)     # noqa: E731
        host = lambda x: host_route(x, label)                                       # noqa: E731
        for _ in range(2):
            timed(clean, data), timed(post, data)
        timed(host, data)
        t = {"clean": [], "post": [], "host": []}
        for r in range(args.reps):  # alternated: every path sees the same clocks
            t["clean"].append(timed(clean, data))
            t["post"].append(timed(post, data))
            if r < args.host_reps:
                t["host"].append(timed(host, data))
        a, b = t["post"][0][2], t["host"][0][2]
        same = torch.equal(a["masks"], b["masks"]) and torch.equal(a["boxes"], b["boxes"])
        changed = int(t["clean"][0][2][1].sum())
        th = line(case, "host route (%s)" % lname, t["host"])
        line(case, "remove_small_regions", t["clean"])
        tp = line(case, "postprocess_small_regions", t["post"])
        print("%-34s changed %d of %d, survivors %d, library == host route: %s, host / library: %.1f" % (
            case, changed, len(masks), a["masks"].shape[0], same, th / tp), flush=True)


if __name__ == "__main__":
    main()
