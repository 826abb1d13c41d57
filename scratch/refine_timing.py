"""Timing of sam6d_hip.refine on the GPU: 200 poses refined against a 1080 x 1920 depth image in 5
iterations, for a dense mesh (the 81 920-face icosphere of scratch/verify_timing.py, 50 mm radius under metre poses) and for two
triangles that fill the image.  The routes are alternated in one process, HIP events around each, two warm-up rounds, median of the
timed rounds with minimum and maximum, and the peak allocation of each route (scratch/verify_timing.py's harness):

  refine_poses          5 iterations, with and without masks: windows, prefix sums and the read-back once, then 5 steps
  5 x render_compare    the nearest existing cost: windows, raster and classify of the same poses five times, no refinement
  one step alone        sam6d_pose_refine_step on preallocated buffers (memsets, view, raster, accumulate, solve)

The observed depth is the render of the true poses before a wall; the starts are the true poses turned by one degree and moved by
3 mm.  The two-triangle case is a plane: its normal equations are singular and every pose ends with status 2 -- the work is done all
the same, which is what is timed.  A kernel trace of this script (--trace-once: one step and nothing else) gives the kernels' shares.

    python scratch/refine_timing.py [--reps 9] [--poses 200] [--mesh dense|quad|both] [--trace-once]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "scratch")]
import verify_timing as VT  # noqa: E402  (the harness, the poses, the camera)
from sam6d_hip import _lib, refine, verify  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)
from tests import verify_ref as VR  # noqa: E402  (Rodrigues)

DEV, H, W, K = VT.DEV, VT.H, VT.W, VT.K
ITERS, GATE = 5, 0.02


def run_mesh(name, v, f, R, t, scale, shift, args):
    N = R.shape[0]
    plane = torch.full((H, W), 1.5, device=DEV)
    first = verify.render_compare((v, f), R, t, K, plane, tol=0.01, scale=scale)
    depth = torch.where(first.ids >= 0, first.depth, plane)
    depth[:, :40] = 0.0
    turn = torch.from_numpy(VR.rotation((3.0, -1.0, 2.0), np.deg2rad(1.0)).astype(np.float32)).to(DEV)
    R0, t0 = turn @ R, t + torch.tensor(shift, device=DEV)
    masks = torch.zeros((N, H, W), dtype=torch.uint8, device=DEV)
    box = first.boxes.cpu().numpy()
    for n in range(N):
        if box[n, 2] >= box[n, 0]:
            masks[n, box[n, 1]:box[n, 3] + 1, box[n, 0]:box[n, 2] + 1] = 1
    res = refine.refine_poses((v, f), R0, t0, K, depth, iters=ITERS, gate=GATE, scale=scale)
    area = (res.boxes[:, 2] - res.boxes[:, 0] + 1).clamp(min=0).long() * (res.boxes[:, 3] - res.boxes[:, 1] + 1).clamp(min=0).long()
    total = int(area.sum())
    before, after = (t0 - t).norm(dim=1), (res.t - t).norm(dim=1)
    print("%s: V = %d, F = %d, N = %d, windows hold %d words (%.1f MiB of z-buffer), pairs %d, status counts %s, median |t - t_true| %.2e -> %.2e"
          % (name, v.shape[0], f.shape[0], N, total, total * 8 / 2.0 ** 20, int(res.n_pairs.sum()), torch.bincount(res.status, minlength=5).tolist(),
             float(before.median()), float(after.median())), flush=True)
    # ---- one step alone, on preallocated buffers
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    offset = torch.zeros((N + 1,), dtype=torch.int64, device=DEV)
    offset[1:] = torch.cumsum(area, 0)
    need = lib.sam6d_pose_refine_workspace_bytes(total, N)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=DEV)
    state0 = torch.cat([R0.reshape(N, 9), t0], dim=1).double()
    state = state0.clone()
    acc = torch.empty((N, 32), dtype=torch.int64, device=DEV)
    stats = torch.empty((N, 4), dtype=torch.int32, device=DEV)
    iu = refine.inv_unit(float(refine.mesh_radius2(v)), scale)

    def step(m):
        state.copy_(state0)
        _lib.call("sam6d_pose_refine_step", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], scale, N, *K, H, W, 1e-3, 0, res.boxes.data_ptr(),
                  offset.data_ptr(), total, depth.data_ptr(), m.data_ptr() if m is not None else None, GATE, iu, 1e-6, 32, float("inf"),
                  state.data_ptr(), acc.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, stream)

    if args.trace_once:
        step(None)
        torch.cuda.synchronize()
        return

    def compare5(m):
        for _ in range(ITERS):
            out = verify.render_compare((v, f), R0, t0, K, depth, masks=m, tol=0.01, scale=scale)
        return out

    VT.alternate([("refine_poses, %d iterations, no masks" % ITERS, lambda: refine.refine_poses((v, f), R0, t0, K, depth, iters=ITERS, gate=GATE, scale=scale)),
                  ("%d x render_compare, no masks" % ITERS, lambda: compare5(None)),
                  ("refine_poses, %d iterations, masks" % ITERS,
                   lambda: refine.refine_poses((v, f), R0, t0, K, depth, masks=masks, iters=ITERS, gate=GATE, scale=scale)),
                  ("%d x render_compare, masks" % ITERS, lambda: compare5(masks))], args.reps)
    VT.alternate([("  sam6d_pose_refine_step alone, no masks", lambda: step(None)), ("  sam6d_pose_refine_step alone, masks", lambda: step(masks))],
                 args.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--mesh", default="both")
    ap.add_argument("--trace-once", action="store_true")
    args = ap.parse_args()
    print("%s, %d poses on %d x %d, %d iterations, median of %d after 2 warm-ups, routes alternated"
          % (torch.cuda.get_device_name(0), args.poses, H, W, ITERS, args.reps))
    if args.mesh in ("dense", "both"):
        v, f = RR.icosphere(6, 50.0)  # millimetres
        v = v * np.array([1.0, 0.8, 0.6], np.float32)  # an ellipsoid: a sphere's depth does not fix its rotation
        R, t = VT.poses(args.poses, 0.6, 1.2)
        run_mesh("dense", torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), R, t, 0.001, (0.003, -0.002, 0.003), args)
    if args.mesh in ("quad", "both"):
        v = torch.tensor([[-4.0, -3.0, 0.0], [4.0, -3.0, 0.0], [-4.0, 3.0, 0.0], [4.0, 3.0, 0.0]], device=DEV)  # metres: fills the image at 1 m
        f = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32, device=DEV)
        n = args.poses
        R = torch.eye(3, device=DEV).repeat(n, 1, 1)
        t = torch.stack([torch.zeros(n), torch.zeros(n), torch.linspace(0.8, 1.2, n)], dim=1).to(DEV)
        run_mesh("quad", v, f, R, t, 1.0, (0.0, 0.0, 0.003), args)


if __name__ == "__main__":
    main()
