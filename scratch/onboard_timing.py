"""Timing of sam6d_hip.onboard on the GPU: render_views of 42 views at 512 x 512 and sample_surface of
2048 points, wall clock between device synchronisations, two warm-up runs, median of the timed runs with minimum and maximum.
Meshes: icospheres of 20 480 and 81 920 faces (the two subdivision levels around the 45 666 faces of a typical scanned model), of
327 680 faces (triangles below one pixel: the thread path's extreme) and one triangle that covers every image (the wave path's
extreme), each with the path threshold at its default and forced each way where that is not hopeless.

    python scratch/onboard_timing.py [--reps 9]
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
from sam6d_hip import onboard  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)

DEV = "cuda:0"


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    del res
    return (time.perf_counter() - t0) * 1e3


def timed(name, fn, reps):
    for _ in range(2):
        wall_ms(fn)
    t = [wall_ms(fn) for _ in range(reps)]
    print("%-64s median %9.3f ms  (min %9.3f, max %9.3f)" % (name, statistics.median(t), min(t), max(t)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    poses = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
    view, light = onboard.view_matrices(poses, 0.5 / 50.0)
    view, light = torch.from_numpy(view).to(DEV), torch.from_numpy(light).to(DEV)
    intr = onboard.intrinsics_from_fov(512, 0.691111)
    for level in (5, 6, 7):
        v, f = RR.icosphere(level, 50.0)
        v, f = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        for wave_area, label in ((0, "default"), (1 << 30, "threads only"), (1, "waves only")):
            if level == 7 and wave_area == 1:
                continue
            timed("render 42 x 512^2, F = %d, %s" % (f.shape[0], label),
                  lambda: onboard.render_views(v, f, None, None, view, light, intr, (512, 512), wave_area=wave_area), args.reps)
        timed("sample_surface 2048 points, F = %d" % f.shape[0], lambda: onboard.sample_surface(v, f, 2048), args.reps)
    wall = torch.tensor([[-400.0, -300.0, 0.0], [400.0, -300.0, 0.0], [0.0, 500.0, 0.0]], device=DEV)
    one = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    eye = torch.tensor([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 100.0]]], device=DEV).repeat(42, 1, 1)
    out = onboard.render_views(wall, one, None, None, eye, light, intr, (512, 512))
    print("whole-image triangle: covered %.1f %% of the pixels" % (100.0 * float((out["mask"] == 255).float().mean())))
    timed("render 42 x 512^2, one whole-image triangle, default (wave)", lambda: onboard.render_views(wall, one, None, None, eye, light, intr, (512, 512)),
          args.reps)
    timed("render 42 x 512^2, one whole-image triangle, thread", lambda: onboard.render_views(wall, one, None, None, eye, light, intr, (512, 512),
                                                                                             wave_area=1 << 30), args.reps)


if __name__ == "__main__":
    main()
