"""Timing of sam6d_hip.visualize on the GPU: one overlay_masks and one draw_detections call at the
workload's own shape (1080 x 1920, 200 instances x 512 points, boxes of a few hundred pixels), the worst shape the limits allow that
is still sane (200 boxes spanning the screen), and the round trip the device route saves (download of the image and the poses, the
numpy painter of tests/overlay_ref.py restricted to each primitive's neighbourhood).  Wall clock between device synchronisations,
two warm-up runs, median of the timed runs with minimum and maximum; beside each the launch's write floor: the canvas plus the key
buffer (memset and atomics' lines) over the 6.29 TB/s a float4 copy reaches on this part.

    python scratch/overlay_timing.py [--reps 9]
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
from sam6d_hip import inputs, visualize as V  # noqa: E402
from tests import overlay_ref as OR  # noqa: E402

DEV = "cuda:0"
H, W, N, P = 1080, 1920, 200, 512
HBM = 6.29e12  # bytes / s


def wall_ms(fn, sync=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    if sync:
        torch.cuda.synchronize()
    del res
    return (time.perf_counter() - t0) * 1e3


def timed(name, fn, reps, floor_bytes=None, warm=2):
    for _ in range(warm):
        wall_ms(fn)
    t = [wall_ms(fn) for _ in range(reps)]
    floor = "" if floor_bytes is None else "  write floor %.4f ms (%.1f MB)" % (floor_bytes / HBM * 1e3, floor_bytes / 1e6)
    print("%-72s median %9.3f ms  (min %9.3f, max %9.3f)%s" % (name, statistics.median(t), min(t), max(t), floor), flush=True)


def poses(rng, n, z_lo, z_hi, spread):
    R, t = [], []
    for _ in range(n):
        Q, _r = np.linalg.qr(rng.randn(3, 3))
        R.append(Q * np.sign(np.linalg.det(Q)))
        z = rng.uniform(z_lo, z_hi)
        t.append([rng.uniform(-spread, spread) * z, rng.uniform(-spread, spread) * z * H / W, z])
    return np.asarray(R, np.float32), np.asarray(t, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    model = (rng.uniform(-1, 1, size=(2048, 3)) * (0.12, 0.09, 0.06)).astype(np.float32)
    K = np.broadcast_to(np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]], np.float32), (N, 3, 3)).copy()
    box = V.box_corners(model).astype(np.float32)
    pts = model[rng.choice(len(model), P)]
    colors = V.palette(N)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    rgb_d, K_d, box_d, pts_d, model_d = d(rgb), d(K), d(box), d(pts), d(model)
    canvas_bytes, key_bytes = H * 2 * W * 3, H * W * 4

    # ---- mask overlay
    yy, xx = np.mgrid[0:H, 0:W]
    for M in (1, 200):
        c = rng.uniform(0.1, 0.9, size=(M, 2)) * (H, W)
        masks = np.stack([(yy - c[m, 0]) ** 2 + (xx - c[m, 1]) ** 2 <= 150 ** 2 for m in range(M)]).astype(np.uint8)
        masks_d = d(masks)
        cols = V.palette(M)
        timed("overlay_masks 1080 x 1920, M = %d (discs of radius 150)" % M, lambda: V.overlay_masks(rgb_d, masks_d, colors=cols), args.reps,
              canvas_bytes)
        timed("  without edges", lambda: V.overlay_masks(rgb_d, masks_d, colors=cols, edge=False), args.reps, canvas_bytes)
        if M == 1:
            lut = np.stack([V.blend_table(cols[0])])
            timed("  saved round trip: masks + image download, numpy restatement", lambda: OR.overlay_masks(rgb_d.cpu().numpy(), masks_d.cpu().numpy(), lut),
                  3, warm=1)
        del masks_d

    # ---- pose overlay
    for label, z_lo, z_hi, spread in (("boxes of a few hundred pixels", 0.6, 1.2, 0.45), ("boxes spanning the screen", 0.13, 0.16, 0.1)):
        R, t = poses(rng, N, z_lo, z_hi, spread)
        R_d, t_d = d(R), d(t)
        canvas, skipped = V.draw_primitives(rgb_d, R_d, t_d, K_d, box_d, pts_d, colors)
        cu = np.stack([np.stack(OR.project(R[i], t[i], K[i], box)[:2], 1) for i in range(N)])
        ext = (cu.max(axis=1) - cu.min(axis=1)).mean(axis=0)
        painted = float((canvas[:, W:] != rgb_d).any(dim=2).float().mean())
        print("%s: mean box extent %d x %d pixels, %.1f %% of the picture painted, %d primitives skipped"
              % (label, ext[0], ext[1], 100 * painted, int(skipped.sum())), flush=True)
        timed("draw_primitives 1080 x 1920, N = 200, P = 512, %s" % label, lambda: V.draw_primitives(rgb_d, R_d, t_d, K_d, box_d, pts_d, colors),
              args.reps, canvas_bytes + 2 * key_bytes)
        timed("  draw_detections (host corner + np.random.choice + upload included)",
              lambda: V.draw_detections(rgb_d, R_d, t_d, model, K_d, colors=colors), args.reps, canvas_bytes + 2 * key_bytes)
        timed("  draw_detections, model points on the device, DeviceChoice",
              lambda: V.draw_detections(rgb_d, R_d, t_d, model_d, K_d, colors=colors, rng=inputs.DeviceChoice(1)),
              args.reps, canvas_bytes + 2 * key_bytes)
        timed("  P = 0 (boxes only)", lambda: V.draw_primitives(rgb_d, R_d, t_d, K_d, box_d, pts_d[:0], colors), args.reps, canvas_bytes + 2 * key_bytes)
        timed("  N = 0 (memset + resolve)", lambda: V.draw_primitives(rgb_d, R_d[:0], t_d[:0], K_d[:0], box_d, pts_d, (255, 0, 0)), args.reps,
              canvas_bytes + 2 * key_bytes)

        n_host = N if z_lo > 0.5 else 10  # the numpy painter needs ~0.1 s per screen-spanning edge: ten instances of those

        def host_route():
            img, Rh, th, Kh = rgb_d.cpu().numpy(), R_d[:n_host].cpu().numpy(), t_d[:n_host].cpu().numpy(), K_d[:n_host].cpu().numpy()
            return OR.draw_detections(img, Rh, th, Kh, box, pts, colors[:n_host], window=True)

        t0 = time.perf_counter()
        want, _ = host_route()
        print("  saved round trip: image + poses download, numpy painter (windowed), %d instances, one run: %9.1f ms"
              % (n_host, (time.perf_counter() - t0) * 1e3), flush=True)
        got, _ = V.draw_primitives(rgb_d, R_d[:n_host], t_d[:n_host], K_d[:n_host], box_d, pts_d, colors[:n_host])
        print("  device canvas == numpy painter (%d instances): %s" % (n_host, bool(np.array_equal(got.cpu().numpy(), want))), flush=True)


if __name__ == "__main__":
    main()
