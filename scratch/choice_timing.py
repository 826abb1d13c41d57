"""Timing of the point choices of sam6d_hip.inputs.test_data / inputs.templates on the GPU: the default
host route (one np.random.choice per detection, a read-back in front of it and an upload of the indices behind it) against
rng=DeviceChoice (inputs.draw_choice, one launch).  Both paths alternated in one process, wall clock between device synchronisations,
two warm-up runs, median of the timed runs with minimum and maximum.  test_data end to end with N = 200 proposals (and N = 1) on
480 x 640, disc masks of radius about 30, 80 and 150 pixels, ns = 2048; templates with T = 42 renders of 480 x 640, ns = 5000; then
draw_choice on its own over the same counts, and one row of 1 166 400 candidates.

    python scratch/choice_timing.py [--reps 9]
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
from sam6d_hip import inputs  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    del res
    return (time.perf_counter() - t0) * 1e3


def alternate(paths, reps):
    for _ in range(2):
        for fn in paths.values():
            wall_ms(fn)
    t = {k: [] for k in paths}
    for _ in range(reps):  # alternated: every path sees the same clocks
        for k, fn in paths.items():
            t[k].append(wall_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def report(name, res, host="host np.random", device="DeviceChoice"):
    for k, (med, lo, hi) in res.items():
        print("%-44s %-16s median %9.3f ms  (min %9.3f, max %9.3f, spread %8.3f)" % (name, k, med, lo, hi, hi - lo))
    if host in res and device in res:
        gain, spread = res[host][0] - res[device][0], res[host][2] - res[host][1]
        print("%-44s host - device = %.3f ms, host spread %.3f ms: device faster by more than the spread: %s" % ("", gain, spread, gain > spread))


def discs(g, N, r, h=H, w=W):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    cy = torch.from_numpy(g.integers(r, max(h - r, r + 1), N))
    cx = torch.from_numpy(g.integers(r, max(w - r, r + 1), N))
    rr = torch.from_numpy(g.integers(max(r - 3, 1), r + 4, N))
    return (yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2 < rr[:, None, None] ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    g = np.random.default_rng(0)
    img = torch.from_numpy(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)
    xx = np.arange(W)[None]
    depth = torch.from_numpy((0.6 + 0.0004 * xx + 0.02 * g.random((H, W))).astype(np.float32)).to(DEV)
    model = ((g.random((1024, 3)) - 0.5) * 0.7).astype(np.float32)  # radius ~0.5 m: the radius filter keeps every point of a disc
    cfg = dict(img_size=224, n_sample_observed_point=2048, n_sample_template_point=5000, rgb_mask_flag=True)
    host_rng, dev_rng = np.random.RandomState(1), inputs.DeviceChoice(1)
    counts = {}

    for N in (200, 1):
        for r in (30, 80, 150):
            masks = discs(g, N, r).to(torch.uint8).to(DEV)
            scores = g.random(N)
            geom = inputs.proposal_geometry(masks, depth, K, np.max(np.linalg.norm(model, axis=1)))
            n_keep = geom["n_keep"]
            counts[(N, r)] = n_keep.clone()
            paths = {"host np.random": lambda: inputs.test_data(img, depth, K, masks, scores, model, cfg, rng=host_rng),
                     "DeviceChoice": lambda: inputs.test_data(img, depth, K, masks, scores, model, cfg, rng=dev_rng)}
            kept = len(paths["DeviceChoice"]()[1])
            report("test_data N = %d, r ~ %d px (n_keep mean %d, kept %d)" % (N, r, int(n_keep.float().mean()), kept), alternate(paths, args.reps))
            del masks, geom
            torch.cuda.empty_cache()

    T = 42
    tm = (discs(g, T, 113).to(torch.uint8) * 255).to(DEV)
    ti = torch.from_numpy(g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)).to(DEV)
    txyz = torch.from_numpy(((g.random((T, H, W, 3)) - 0.5) * 200.0).astype(np.float32)).to(DEV)
    n_valid = inputs.template_geometry(tm, txyz)["n_valid"]
    paths = {"host np.random": lambda: inputs.templates(ti, tm, txyz, cfg, rng=host_rng),
             "DeviceChoice": lambda: inputs.templates(ti, tm, txyz, cfg, rng=dev_rng)}
    report("templates T = 42 (n_valid mean %d), ns = 5000" % int(n_valid.float().mean()), alternate(paths, args.reps))

    # the launch on its own, against the bare host loop over the same counts
    def host_loop(n, ns):
        return np.stack([inputs._draw(host_rng, int(v), ns) for v in n])

    for (N, r), n in counts.items():
        nh = n.cpu().numpy()
        report("draw alone N = %d, r ~ %d px, ns = 2048" % (N, r),
               alternate({"host np.random": lambda: host_loop(nh, 2048), "DeviceChoice": lambda: inputs.draw_choice(n, 2048, 1)}, args.reps))
    nh = n_valid.cpu().numpy()
    report("draw alone T = 42, ns = 5000", alternate({"host np.random": lambda: host_loop(nh, 5000),
                                                      "DeviceChoice": lambda: inputs.draw_choice(n_valid, 5000, 1)}, args.reps))
    one = torch.tensor([1166400], dtype=torch.int32, device=DEV)
    report("draw alone, one row of 1 166 400, ns = 5000", alternate({"host np.random": lambda: host_loop([1166400], 5000),
                                                                     "DeviceChoice": lambda: inputs.draw_choice(one, 5000, 1)}, args.reps))


if __name__ == "__main__":
    main()
