"""Timing of SAM's image front on the GPU: the one-launch library path (sam6d_hip.samfront.preprocess, both layouts) against the
package's eager route on the same GPU (samfront.eager for the x layout; eager + sam6d_sam_patch_rows for the rows layout), alternated
in one process, device events, median of repeated runs after warm-up.  Where PIL imports, also the reference's host route, wall clock
with a device synchronise: PIL resize on the CPU, upload, torch normalise + pad on the device, sam6d_sam_patch_rows.

    python scratch/samfront_timing.py [--reps 15] [--sizes 480x640 1080x1920]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd")]
from sam6d_hip import _lib, amg, samfront  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def patch_rows(x):
    A = torch.empty((x.shape[0] * 4096, 768), device=x.device)
    _lib.call("sam6d_sam_patch_rows", x.data_ptr(), A.data_ptr(), x.shape[0], torch.cuda.current_stream().cuda_stream)
    return A


def report(name, paths, reps, clock=timed):
    for _ in range(2):
        for fn in paths.values():
            clock(fn)
    t = {k: [] for k in paths}
    for _ in range(reps):  # alternated: the paths see the same clocks
        for k, fn in paths.items():
            t[k].append(clock(fn))
    for k, ms in t.items():
        print("%-22s %-34s median %8.3f ms  (min %8.3f, max %8.3f, %d runs)" % (name, k, statistics.median(ms), min(ms), max(ms), len(ms)))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", nargs="+", default=["480x640", "1080x1920"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    try:
        from PIL import Image
    except ImportError:
        Image = None
        print("PIL does not import here: the reference's host route is not timed")
    mean_d, std_d = torch.tensor(MEAN, device=dev).view(-1, 1, 1), torch.tensor(STD, device=dev).view(-1, 1, 1)
    for size in args.sizes:
        h, w = (int(v) for v in size.split("x"))
        img = np.random.RandomState(1).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        d = torch.from_numpy(img).to(dev)
        assert torch.equal(samfront.preprocess(d, MEAN, STD, layout="rows"), patch_rows(samfront.eager(d, MEAN, STD)))
        report(size, {"library, x layout": lambda: samfront.preprocess(d, MEAN, STD, layout="x"),
                      "library, rows layout": lambda: samfront.preprocess(d, MEAN, STD, layout="rows"),
                      "eager, x layout": lambda: samfront.eager(d, MEAN, STD),
                      "eager + patch rows": lambda: patch_rows(samfront.eager(d, MEAN, STD))}, args.reps)
        report(size + " (wall, with upload)", {"library, rows layout": lambda: samfront.preprocess(torch.from_numpy(img).to(dev), MEAN, STD, layout="rows")},
               args.reps, wall)
        if Image is not None:
            oh, ow = amg.preprocess_shape(h, w, 1024)

            def host_route():
                r = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
                x = torch.as_tensor(r, device=dev).permute(2, 0, 1).contiguous()[None]
                x = torch.nn.functional.pad((x - mean_d) / std_d, (0, 1024 - ow, 0, 1024 - oh))
                return patch_rows(x)
            assert torch.equal(host_route(), samfront.preprocess(d, MEAN, STD, layout="rows"))
            report(size + " (wall, with upload)", {"PIL + upload + torch + patch rows": host_route}, args.reps, wall)


if __name__ == "__main__":
    main()
