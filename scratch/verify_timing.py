"""Timing of sam6d_hip.verify on the GPU: 200 poses checked against a 1080 x 1920 depth image, for a dense
mesh (the 81 920-face icosphere of scratch/onboard_timing.py, 50 mm radius under metre poses) and for two triangles that fill the
image.  Two routes, alternated in one process, HIP events around each, two warm-up rounds, median of the timed rounds with minimum
and maximum, and the peak allocation of each route:

  windowed   verify.render_compare (with and without masks), and its stages alone on preallocated buffers: sam6d_pose_windows, the
             prefix sums with their 8-byte read-back, sam6d_pose_verify with the map, without the map, and with masks
  full size  the only route before: onboard.render_views of the same poses at full size in slices that fit (32 bytes per pixel and
             view, plus the z-buffer), followed by the same classification, counts and composite in torch ops

The kernels inside sam6d_pose_verify (raster, classify, mask area, resolve) are one call from outside; a kernel trace of this script
(--trace-once: one windowed round and nothing else) gives their shares.

    python scratch/verify_timing.py [--reps 9] [--poses 200] [--slice 16] [--mesh dense|quad|both] [--trace-once]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd")]
from sam6d_hip import _lib, onboard, verify  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)

DEV = "cuda:0"
H, W = 1080, 1920
K = (1066.778, 1067.487, 960.0, 540.0)
TOL = 0.01


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    del res
    return a.elapsed_time(b)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    del res
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def alternate(routes, reps):
    """routes: [(name, fn)]; every round runs each once, in order"""
    times = {name: [] for name, _ in routes}
    for r in range(reps + 2):
        for name, fn in routes:
            t = event_ms(fn)
            if r >= 2:
                times[name].append(t)
    for name, fn in routes:
        t = times[name]
        print("  %-58s median %9.3f ms  (min %9.3f, max %9.3f)  peak %8.1f MiB" % (name, statistics.median(t), min(t), max(t), peak_mib(fn)),
              flush=True)


def poses(n, z_lo, z_hi, seed=0):
    """n poses whose centres project inside the image, depths in [z_lo, z_hi] metres, random rotations"""
    g = np.random.default_rng(seed)
    z = g.uniform(z_lo, z_hi, n)
    u, v = g.uniform(100, W - 100, n), g.uniform(100, H - 100, n)
    t = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    R = np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], 1),
                  np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], 1),
                  np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], 1)], 1)
    return torch.from_numpy(R.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.float32)).to(DEV)


def full_size_route(v, f, view, depth, masks, step):
    """render_views at full size in slices of `step` views, then the classification of csrc/verify.hip in torch ops"""
    N = view.shape[0]
    light = torch.zeros((N, 3), device=DEV)
    counts = torch.zeros((N, 8), dtype=torch.int32, device=DEV)
    best = torch.full((H, W), float("inf"), device=DEV)
    ids = torch.full((H, W), -1, dtype=torch.int32, device=DEV)
    known = depth > 0
    for s in range(0, N, step):
        out = onboard.render_views(v, f, None, None, view[s:s + step], light[s:s + step], K, (H, W))
        hit, r = out["mask"] == 255, out["depth"]
        e = depth - r
        behind, occluded = hit & known & (e > TOL), hit & known & (e < -TOL)
        c = counts[s:s + step]
        c[:, 0] = hit.sum((1, 2))
        c[:, 2] = occluded.sum((1, 2))
        c[:, 3] = behind.sum((1, 2))
        c[:, 4] = (hit & ~known).sum((1, 2))
        c[:, 1] = c[:, 0] - c[:, 2] - c[:, 3] - c[:, 4]
        c[:, 7] = out["n_dropped"]
        if masks is not None:
            m = masks[s:s + step] != 0
            c[:, 5] = m.sum((1, 2))
            c[:, 6] = (hit & m).sum((1, 2))
        near, arg = torch.where(hit, r, torch.full_like(r, float("inf"))).min(dim=0)
        take = near < best
        best = torch.where(take, near, best)
        ids = torch.where(take, (arg + s).to(torch.int32), ids)
    return counts, ids, torch.where(ids >= 0, best, torch.zeros_like(best))


def run_mesh(name, v, f, R, t, scale, args):
    N = R.shape[0]
    view = verify.pose_views(R, t, scale)
    plane = torch.full((H, W), 1.5, device=DEV)
    first = verify.render_compare((v, f), R, t, K, plane, tol=TOL, scale=scale)
    depth = torch.where(first.ids >= 0, first.depth, plane)  # what a sensor would see of these poses before a wall
    depth[:, :40] = 0.0                                      # and a strip without a reading
    masks = torch.zeros((N, H, W), dtype=torch.uint8, device=DEV)
    box = first.boxes.cpu().numpy()
    for n in range(N):  # the windows as masks: the proposals' role
        if box[n, 2] >= box[n, 0]:
            masks[n, box[n, 1]:box[n, 3] + 1, box[n, 0]:box[n, 2] + 1] = 1
    area = (first.boxes[:, 2] - first.boxes[:, 0] + 1).clamp(min=0).long() * (first.boxes[:, 3] - first.boxes[:, 1] + 1).clamp(min=0).long()
    total = int(area.sum())
    print("%s: V = %d, F = %d, N = %d, windows hold %d words (%.1f MiB of z-buffer, %.2f %% of N H W), n_render %d"
          % (name, v.shape[0], f.shape[0], N, total, total * 8 / 2.0 ** 20, 100.0 * total / (N * H * W), int(first.counts[:, 0].sum())), flush=True)
    # ---- the stages alone, on preallocated buffers
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    b = torch.empty((N, 4), dtype=torch.int32, device=DEV)
    dropped = torch.empty((N,), dtype=torch.int32, device=DEV)
    offset = torch.zeros((N + 1,), dtype=torch.int64, device=DEV)
    offset[1:] = torch.cumsum(area, 0)
    need = lib.sam6d_pose_verify_workspace_bytes(total, H, W)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=DEV)
    counts = torch.empty((N, 8), dtype=torch.int32, device=DEV)
    ids, dout = torch.empty((H, W), dtype=torch.int32, device=DEV), torch.empty((H, W), device=DEV)

    def windows():
        _lib.call("sam6d_pose_windows", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], view.data_ptr(), N, *K, H, W, 1e-3, b.data_ptr(),
                  dropped.data_ptr(), stream)

    def prefix():
        bw, bh = (b[:, 2] - b[:, 0] + 1).clamp_(min=0).long(), (b[:, 3] - b[:, 1] + 1).clamp_(min=0).long()
        off = torch.zeros((N + 1,), dtype=torch.int64, device=DEV)
        torch.cumsum(bw * bh, dim=0, out=off[1:])
        return int(off[N])

    def check(m, want_map):
        _lib.call("sam6d_pose_verify", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], view.data_ptr(), N, *K, H, W, 1e-3, 0, b.data_ptr(),
                  offset.data_ptr(), total, depth.data_ptr(), m.data_ptr() if m is not None else None, TOL, counts.data_ptr(),
                  ids.data_ptr() if want_map else None, dout.data_ptr() if want_map else None, ws.data_ptr(), need, stream)

    if args.trace_once:
        windows()
        check(masks, True)
        torch.cuda.synchronize()
        return
    windows()
    alternate([("render_compare, no masks", lambda: verify.render_compare((v, f), R, t, K, depth, tol=TOL, scale=scale)),
               ("full size + torch ops, no masks (slices of %d)" % args.slice, lambda: full_size_route(v, f, view, depth, None, args.slice)),
               ("render_compare, masks", lambda: verify.render_compare((v, f), R, t, K, depth, masks=masks, tol=TOL, scale=scale)),
               ("full size + torch ops, masks (slices of %d)" % args.slice, lambda: full_size_route(v, f, view, depth, masks, args.slice))], args.reps)
    alternate([("  sam6d_pose_windows alone", windows), ("  box areas, prefix sums, 8-byte read-back", prefix),
               ("  sam6d_pose_verify alone, map, no masks", lambda: check(None, True)),
               ("  sam6d_pose_verify alone, no map, no masks", lambda: check(None, False)),
               ("  sam6d_pose_verify alone, map, masks", lambda: check(masks, True))], args.reps)
    # the two routes agree (the full-size route's arg-min on a tie is torch's, so ids are compared where the depth is not tied)
    got = verify.render_compare((v, f), R, t, K, depth, masks=masks, tol=TOL, scale=scale)
    c, i, d = full_size_route(v, f, view, depth, masks, args.slice)
    print("  counts equal: %s, depth equal: %s, ids differ on %d pixels" % (bool(torch.equal(got.counts, c)), bool(torch.equal(got.depth, d)),
                                                                              int((got.ids != i).sum())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--slice", type=int, default=16)
    ap.add_argument("--mesh", default="both")
    ap.add_argument("--trace-once", action="store_true")
    args = ap.parse_args()
    print("%s, %d poses on %d x %d, median of %d after 2 warm-ups, routes alternated" % (torch.cuda.get_device_name(0), args.poses, H, W, args.reps))
    if args.mesh in ("dense", "both"):
        v, f = RR.icosphere(6, 50.0)  # millimetres
        R, t = poses(args.poses, 0.6, 1.2)
        run_mesh("dense", torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), R, t, 0.001, args)
    if args.mesh in ("quad", "both"):
        v = torch.tensor([[-4.0, -3.0, 0.0], [4.0, -3.0, 0.0], [-4.0, 3.0, 0.0], [4.0, 3.0, 0.0]], device=DEV)  # metres: fills the image at 1 m
        f = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32, device=DEV)
        n = args.poses
        R = torch.eye(3, device=DEV).repeat(n, 1, 1)
        t = torch.stack([torch.zeros(n), torch.zeros(n), torch.linspace(0.8, 1.2, n)], dim=1).to(DEV)
        run_mesh("quad", v, f, R, t, 1.0, args)


if __name__ == "__main__":
    main()
