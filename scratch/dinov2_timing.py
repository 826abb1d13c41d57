"""Eager PyTorch vs the library's proposal descriptors (CustomDINOv2.forward: crops + DINOv2 ViT-L/14 + masked patch descriptors),
alternated within one process: device events, warm-up of both paths, the median and max - min of 2 x --reps runs per shape.
N = 1, 42 and 200 proposals on a 480 x 640 image, random weights; one JSON line per shape.

    python scratch/dinov2_timing.py [--reps 20] [--only n200]      (--only n200: one library pass at N = 200, for a rocprofv3 run)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "openvino-sam-6d_amd"),
                os.path.join(os.path.dirname(HERE), "openvino-sam-6d_amd", "ism")]

import torch  # noqa: E402


class Det:
    pass


def _time(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = importlib.import_module("model.dinov2").CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, p in d.model.named_parameters():
            if n.endswith("gamma"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5 if p.dim() >= 2 else 0.05))
    d.model = d.model.to(dev).eval()
    H, W = 480, 640
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).numpy()

    def case(N):
        x1 = torch.randint(0, W - 220, (N,), generator=g)
        y1 = torch.randint(0, H - 220, (N,), generator=g)
        bw, bh = torch.randint(20, 220, (N,), generator=g), torch.randint(20, 220, (N,), generator=g)
        boxes = torch.stack([x1, y1, x1 + bw, y1 + bh], 1).to(dev)
        masks = torch.zeros(N, H, W)
        for i, (a_, b_, c_, e_) in enumerate(boxes.tolist()):
            masks[i, b_:e_, a_:c_] = 1.0
        masks = masks.to(dev)

        def run():
            p = Det()
            p.masks, p.boxes = masks.clone(), boxes
            return d.forward(img, p)
        return run

    def switch(on):
        os.environ["SAM6D_HIP_DINOV2"] = "1" if on else "0"

    with torch.no_grad():
        if a.only == "n200":
            switch(True)
            f = case(200)
            print(json.dumps(dict(shape="N=200", hip_ms=round(statistics.median(_time(f, max(a.reps, 1), warm=1)), 3))), flush=True)
            return
        for N in (1, 42, 200):
            f = case(N)
            res = {"eager": [], "hip": []}
            for _ in range(2):
                for on in (False, True):
                    switch(on)
                    res["hip" if on else "eager"] += _time(f, a.reps)
            e, h = statistics.median(res["eager"]), statistics.median(res["hip"])
            print(json.dumps(dict(shape="N=%d" % N, runs=len(res["hip"]), eager_ms=round(e, 3), eager_spread_ms=round(max(res["eager"]) - min(res["eager"]), 3),
                                  hip_ms=round(h, 3), hip_spread_ms=round(max(res["hip"]) - min(res["hip"]), 3), speedup=round(e / h, 2))), flush=True)


if __name__ == "__main__":
    main()
