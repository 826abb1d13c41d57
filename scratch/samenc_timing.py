"""Timing of SAM's ViT-H image encoder on the GPU: the library path (sam6d_hip.samenc.encode) against the package's eager fp32 partner
(samenc.eager: the reference's sequence of torch ops, what `sam.image_encoder` runs), alternated in one process, device events, median of
repeated runs after warm-up, plus peak allocation.  Seeded full ViT-H (depth 32, blocks 7 / 15 / 23 / 31 global;
tests/sam_encoder_ref.seeded_weights), one 1024 x 1024 image.

    python scratch/samenc_timing.py [--reps 15] [--modes 1 0] [--depth 32] [--whole-tiles 1 0] [--once]
    (--whole-tiles: with and without the block GEMMs' whole-tile request, act + 32; --once: two library passes in mode 1 with the
    first --whole-tiles value and nothing else, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd")]
from sam6d_hip import samenc  # noqa: E402
from sam6d_hip.pem import Options  # noqa: E402
from tests import sam_encoder_ref as R  # noqa: E402


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
    for _ in range(2):
        timed(lib), timed(eager)
    t = {"library": [], "eager": []}
    for _ in range(reps):  # alternated: both paths see the same clocks
        t["library"].append(timed(lib))
        t["eager"].append(timed(eager))
    for k in ("eager", "library"):
        ms = [x[0] for x in t[k]]
        print("%-40s %-8s median %9.3f ms  (min %9.3f, max %9.3f, %d runs)  peak %8.1f MiB" % (name, k, statistics.median(ms), min(ms), max(ms),
                                                                                               len(ms), max(x[1] for x in t[k])))
    print("%-40s ratio eager / library: %.2f" % (name, statistics.median([x[0] for x in t["eager"]]) / statistics.median([x[0] for x in t["library"]])))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 0])
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--whole-tiles", type=int, nargs="+", default=[1])
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    glob = tuple(i for i in range(args.depth) if i % 8 == 7)
    sd = R.seeded_weights(20250401, depth=args.depth, global_blocks=glob)
    W = samenc.SamEncoderWeights(sd, dev)
    del sd
    x = R.seeded_input(20250402, 1024).to(dev)
    samenc.ENC = samenc.ENC._replace(whole_tiles=bool(args.whole_tiles[0]))
    if args.once:
        for _ in range(2):
            samenc.encode(x, W, options=Options(matmul_mode=1))
            torch.cuda.synchronize()
        return
    with torch.no_grad():
        for whole in args.whole_tiles:
            samenc.ENC = samenc.ENC._replace(whole_tiles=bool(whole))
            for mode in args.modes:
                opt = Options(matmul_mode=mode)
                compare("encode, depth %d, mode %d, whole tiles %d" % (args.depth, mode, whole), lambda: samenc.encode(x, W, options=opt),
                        lambda: samenc.eager(x, W), args.reps)


if __name__ == "__main__":
    main()
