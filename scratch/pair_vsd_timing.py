"""Timing of sam6d_hip.posematch.pair_vsd on the GPU, in the protocol of scratch/verify_timing.py (its
event_ms, alternate and poses are imported; estimates and the tolerances are scratch/poseerr_timing.py's): HIP events around each
route, two warm-up rounds, the routes alternated in one process, median of the timed rounds with minimum and maximum, and the peak
allocation.

  pair_vsd      the A x B matrix of VSD counts for config4's proposal count (A = B = 200 poses), ten tolerances, 1080 x 1920: one
                render per pose, the pairs by the overlap of their windows
  old route     what existed before: the A B pairs expanded on the device and fed to poseerr.vsd 512 pairs a call (79 calls, two
                renders per pair).  The two matrices are compared bit for bit.

over the dense mesh (the 81 920-face icosphere, 50 mm radius under metre poses) and a coarse one (the 642-vertex, 1280-face
icosphere; the 512 vertices of scratch/posematch_timing.py are points without faces, and VSD renders), once with the poses spread
over the image as config4's instances are and once with all of them on one spot, where every window overlaps every other: the worst
case for the pair pass.

The kernels inside sam6d_pose_pair_vsd (raster, view pass, pair pass) are one call from outside; a kernel trace of this script
(--trace-once: three pair_vsd rounds per scene and nothing else; the third is the warm one) gives their shares.

    python scratch/pair_vsd_timing.py [--reps 9] [--poses 200] [--mesh dense|coarse|both] [--scene spread|spot|both] [--trace-once]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "scratch")]
from sam6d_hip import poseerr, posematch, verify  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)
from poseerr_timing import DELTA, DIAMETER, SCALE, TAUS, estimates  # noqa: E402
from verify_timing import DEV, H, K, W, alternate, poses  # noqa: E402


def old_route(mesh, Ra, ta, Rb, tb, depth):
    """the A B pairs in row-major order through poseerr.vsd, 512 a call -> counts (A, B, 4+T)"""
    A, B = Ra.shape[0], Rb.shape[0]
    Re, te, Rg, tg = Ra.repeat_interleave(B, dim=0), ta.repeat_interleave(B, dim=0), Rb.repeat(A, 1, 1), tb.repeat(A, 1)
    parts = [poseerr.vsd(mesh, Re[k:k + 512], te[k:k + 512], Rg[k:k + 512], tg[k:k + 512], K, depth, DELTA, TAUS, diameter=DIAMETER, scale=SCALE)[1]
             for k in range(0, A * B, 512)]
    return torch.cat(parts).reshape(A, B, -1)


def scene(name, n):
    """ground truths b and estimates a near them; `spot`: every pose within a few millimetres of one place"""
    Rb, tb = poses(n, 0.6, 1.2)
    if name == "spot":
        g = torch.Generator(device="cpu").manual_seed(2)
        tb = (torch.tensor([0.05, -0.03, 0.8]) + 0.004 * torch.randn((n, 3), generator=g)).to(DEV)
    Ra, ta = estimates(Rb, tb)
    return Ra, ta, Rb, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--mesh", default="both")
    ap.add_argument("--scene", default="both")
    ap.add_argument("--trace-once", action="store_true")
    args = ap.parse_args()
    n = args.poses
    print("%s, A = B = %d poses, T = %d, %d x %d, median of %d after 2 warm-ups, routes alternated"
          % (torch.cuda.get_device_name(0), n, len(TAUS), H, W, args.reps))
    for mesh_name, level in (("dense", 6), ("coarse", 3)):
        if args.mesh not in (mesh_name, "both"):
            continue
        vn, fn = RR.icosphere(level, 50.0)  # millimetres
        mesh = (torch.from_numpy(vn).to(DEV), torch.from_numpy(fn).to(DEV))
        for scene_name in ("spread", "spot"):
            if args.scene not in (scene_name, "both"):
                continue
            Ra, ta, Rb, tb = scene(scene_name, n)
            plane = torch.full((H, W), 1.5, device=DEV)
            first = verify.render_compare(mesh, Rb, tb, K, plane, tol=0.01, scale=SCALE)
            depth = torch.where(first.ids >= 0, first.depth, plane)  # what a sensor would see of the ground truths before a wall
            depth[:, :40] = 0.0                                      # and a strip without a reading
            new = lambda: posematch.pair_vsd(mesh, Ra, ta, Rb, tb, K, depth, DELTA, TAUS, diameter=DIAMETER, scale=SCALE)  # noqa: E731
            got = new()
            if args.trace_once:
                new(), new()
                torch.cuda.synchronize()
                continue
            met = int((got.counts[:, :, 1] > 0).sum())
            print("%s mesh (V = %d, F = %d), %s: the %d renders cover %d pixels, %d of %d pairs meet in a pixel, %d old-route calls"
                  % (mesh_name, len(vn), len(fn), scene_name, 2 * n, int(got.n_render_a.sum() + got.n_render_b.sum()), met, n * n,
                     (n * n + 511) // 512), flush=True)
            alternate([("pair_vsd", new), ("poseerr.vsd, expanded pairs, 512 a call", lambda: old_route(mesh, Ra, ta, Rb, tb, depth))], args.reps)
            print("  bit for bit against the old route: %s; mean vsd over the matrix at tau = 0.05 .. 0.5: %s"
                  % (bool(torch.equal(new().counts, old_route(mesh, Ra, ta, Rb, tb, depth))),
                     [round(float(x), 3) for x in got.vsd.mean(dim=(0, 1))]), flush=True)


if __name__ == "__main__":
    main()
