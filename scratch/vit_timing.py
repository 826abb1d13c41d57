"""Eager PyTorch vs the library's ViT image features (sam6d_hip.vit), alternated within one process: device events, warm-up, the
median of --reps runs per shape.  Shapes: B = 1 and B = 32 proposals (224 x 224, 2048 chosen pixels each) through
ViTEncoder.get_img_feats, and T = 42 templates x 5000 chosen pixels through the list form of get_obj_feats (eager: 42 batch-1 passes;
library: one stacked batch).  Random weights; one JSON line per shape.

    python scratch/vit_timing.py [--reps 20] [--only b32]        (--only b32: the B = 32 library path alone, for a rocprofv3 pass)
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "openvino-sam-6d_amd"),
                os.path.join(os.path.dirname(HERE), "openvino-sam-6d_amd", "pem")]

import torch  # noqa: E402

from sam6d_hip import synth  # noqa: E402


def _time(fn, reps, warm=3):
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
    import importlib
    fe = importlib.import_module("feature_extraction").ViTEncoder(synth.default_model_cfg().feature_extraction, 2048)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for n, p in fe.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5 if p.dim() >= 2 else 0.05))
    fe = fe.to(dev).eval()

    def switch(on):
        os.environ["SAM6D_HIP_VIT"] = "1" if on else "0"

    def img_case(B):
        rgb = torch.randn(B, 3, 224, 224, generator=g).to(dev)
        ch = torch.randint(0, 224 * 224, (B, 2048), generator=g).to(dev)
        return lambda: fe.get_img_feats(rgb, ch)

    def tem_case(T=42, N=5000):
        rgbs = [torch.randn(1, 3, 224, 224, generator=g).to(dev) for _ in range(T)]
        pts = [torch.rand(1, N, 3, generator=g).to(dev) for _ in range(T)]
        chs = [torch.randint(0, 224 * 224, (1, N), generator=g).to(dev) for _ in range(T)]
        return lambda: fe.get_obj_feats(rgbs, pts, chs)

    with torch.no_grad():
        if a.only == "b32":
            switch(True)
            f = img_case(32)
            print(json.dumps(dict(shape="B=32", hip_ms=round(statistics.median(_time(f, a.reps)), 4))), flush=True)
            return
        for name, f in (("B=1", img_case(1)), ("B=32", img_case(32)), ("T=42x5000", tem_case())):
            res = {"eager": [], "hip": []}
            for _ in range(2):  # alternate the two paths twice: median of 2 x reps runs each
                for on in (False, True):
                    switch(on)
                    res["hip" if on else "eager"] += _time(f, a.reps)
            e, h = statistics.median(res["eager"]), statistics.median(res["hip"])
            print(json.dumps(dict(shape=name, eager_ms=round(e, 4), hip_ms=round(h, 4), speedup=round(e / h, 2))), flush=True)


if __name__ == "__main__":
    main()
