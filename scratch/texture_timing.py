"""Timing of the textured template render on the GPU, in one process: 42 views at 512 x 512 of one dense
mesh (an icosphere of 81 920 faces with a spherical texture map) through sam6d_render_views with vertex colours and through
sam6d_render_views_textured with a 1024 x 1024 and a 4096 x 4096 texture, and the single whole-image triangle through both entries.
The C entries are called directly on buffers allocated once, so a figure is the entry's two memsets and two launches and nothing of
the Python layer; HIP events around each call, three warm-up rounds, the routes alternated within every round, median of the timed
rounds with minimum and maximum.

    python scratch/texture_timing.py [--reps 30]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd")]
from sam6d_hip import _lib, onboard  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)

DEV = "cuda:0"
T, H, W = 42, 512, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    g = np.random.default_rng(0)
    poses = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
    view, light = onboard.view_matrices(poses, 0.5 / 50.0)
    intr = [float(x) for x in onboard.intrinsics_from_fov(512, 0.691111)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    view, light, lut, texel = dev(view), dev(light), dev(onboard.srgb_table()), dev(onboard.texel_table())
    out = dict(mask=torch.empty((T, H, W), dtype=torch.uint8, device=DEV), face=torch.empty((T, H, W), dtype=torch.int32, device=DEV),
               depth=torch.empty((T, H, W), device=DEV), xyz=torch.empty((T, H, W, 3), device=DEV),
               rgb=torch.empty((T, H, W, 3), dtype=torch.uint8, device=DEV), n_dropped=torch.empty((T,), dtype=torch.int32, device=DEV))
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=DEV)
    tail = [out[k].data_ptr() for k in ("mask", "face", "depth", "xyz", "rgb", "n_dropped")] + [ws.data_ptr(), need]
    textures = {side: dev(np.concatenate([g.integers(0, 256, (side, side, 3), dtype=np.uint8), np.zeros((side, side, 1), np.uint8)], axis=2))
                for side in (1024, 4096)}

    def scene(v, f, mview):
        n = v / np.linalg.norm(v, axis=1, keepdims=True)
        vt = np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 2], -1, 1)) / np.pi], axis=1).astype(np.float32)
        return dict(v=dev(v), f=dev(f), c=dev(g.integers(0, 256, (len(v), 3), dtype=np.uint8)), uv=dev(vt[f]), view=mview, V=len(v), F=len(f))

    def plain(s):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.call("sam6d_render_views", s["v"].data_ptr(), s["V"], s["f"].data_ptr(), s["F"], None, s["c"].data_ptr(), s["view"].data_ptr(),
                  light.data_ptr(), T, *intr, H, W, onboard.NEAR, 0.05, 0, lut.data_ptr(), 0, *tail, stream)

    def textured(s, side):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.call("sam6d_render_views_textured", s["v"].data_ptr(), s["V"], s["f"].data_ptr(), s["F"], None, s["view"].data_ptr(), light.data_ptr(),
                  T, *intr, H, W, onboard.NEAR, 0.05, lut.data_ptr(), 0, s["uv"].data_ptr(), textures[side].data_ptr(), side, side,
                  texel.data_ptr(), *tail, stream)

    v, f = RR.icosphere(6, 50.0)
    dense = scene(v, f, view)
    wall = np.array([[-400.0, -300.0, 0.0], [400.0, -300.0, 0.0], [0.0, 500.0, 0.0]], np.float32)
    eye = torch.tensor([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 100.0]]], device=DEV).repeat(T, 1, 1).contiguous()
    single = scene(wall, np.array([[0, 1, 2]], np.int32), eye)
    single["uv"] = dev(np.array([[[0, 0], [4, 0], [2, 4]]], np.float32))
    for name, s in (("dense mesh, F = %d" % dense["F"], dense), ("one whole-image triangle", single)):
        routes = [("vertex colours", lambda: plain(s)), ("texture 1024 x 1024", lambda: textured(s, 1024)),
                  ("texture 4096 x 4096", lambda: textured(s, 4096))]
        times = {r: [] for r, _ in routes}
        for rep in range(3 + args.reps):
            for r, fn in (routes if rep % 2 == 0 else routes[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[r].append(a.elapsed_time(b))
        covered = 100.0 * float((out["mask"] == 255).float().mean())
        for r, _ in routes:
            t = times[r]
            print("%-28s %-22s median %8.3f ms  (min %8.3f, max %8.3f, %d runs; %.1f %% of the pixels covered)"
                  % (name, r, statistics.median(t), min(t), max(t), len(t), covered), flush=True)


if __name__ == "__main__":
    main()
