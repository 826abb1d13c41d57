"""Timing of sam6d_hip.poseerr on the GPU, in the protocol of scratch/verify_timing.py (its event_ms,
alternate and poses are imported): 200 pose pairs on 1080 x 1920 with the dense mesh (the 81 920-face icosphere, 50 mm radius under
metre poses).  Each entry runs beside the same function written in plain torch ops on the same device, the routes alternated in one
process, HIP events around each, two warm-up rounds, median of the timed rounds with minimum and maximum, and the peak allocation:

  pose_errors   MSSD, MSPD and ADD over the mesh's 40 962 vertices with S = 1, 2 and the limit of 1024 symmetries; the torch route
                forms G in float64, then e, g, the distances, the maxima and minima with matmul / amax / min, poses in slices that fit
  vsd           two renders per pair into the pair's window and the counts; the torch route renders both poses at full size
                (onboard.render_views, in slices that fit) and forms the masks and counts with elementwise ops and sums

    python scratch/poseerr_timing.py [--reps 9] [--poses 200] [--slice 16] [--only points|vsd]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "scratch")]
from sam6d_hip import onboard, poseerr, verify  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)
from verify_timing import DEV, H, K, W, alternate, poses  # noqa: E402

SCALE = 0.001       # a millimetre model under metre poses
DIAMETER = 0.1      # metres
DELTA = 0.015
TAUS = [0.05 * k for k in range(1, 11)]  # BOP's ten tolerances


def estimates(R, t, seed=1):
    """the ground truths turned by about two degrees and moved by about five millimetres"""
    g = np.random.default_rng(seed)
    n = R.shape[0]
    w = torch.from_numpy((g.normal(size=(n, 3)) * 0.02).astype(np.float32)).to(DEV)
    Kx = torch.zeros((n, 3, 3), device=DEV)
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    dR = torch.linalg.matrix_exp(Kx)
    return (dR @ R).contiguous(), (t + torch.from_numpy((g.normal(size=(n, 3)) * 0.005).astype(np.float32)).to(DEV)).contiguous()


def torch_point_errors(pts, est, gt, syms, step):
    """pose_errors in plain torch ops: -> mssd, mspd, add, mssd_sym, mspd_sym"""
    fx, fy, cx, cy = K
    N, S = est.shape[0], syms.shape[0]
    G = torch.cat([gt[:, None, :, :3].double() @ syms[None, :, :, :3].double(),
                   gt[:, None, :, :3].double() @ syms[None, :, :, 3:].double() + gt[:, None, :, 3:].double()], dim=3).float()  # (N,S,3,4)
    out = [[] for _ in range(5)]
    for s in range(0, N, step):
        e = pts @ est[s:s + step, :, :3].transpose(1, 2) + est[s:s + step, None, :, 3]                        # (n,V,3)
        g = torch.einsum("nsij,vj->nsvi", G[s:s + step, :, :, :3], pts) + G[s:s + step, :, None, :, 3]        # (n,S,V,3)
        d2 = ((e[:, None] - g) ** 2).sum(-1)
        m2, s2 = d2.amax(2).min(1)
        ue, ve = fx * e[..., 0] / e[..., 2] + cx, fy * e[..., 1] / e[..., 2] + cy
        ug, vg = fx * g[..., 0] / g[..., 2] + cx, fy * g[..., 1] / g[..., 2] + cy
        p2 = (ue[:, None] - ug) ** 2 + (ve[:, None] - vg) ** 2
        front = (e[:, None, :, 2] > 0) & (g[..., 2] > 0)
        mp, sp = torch.where(front, p2, torch.zeros_like(p2)).amax(2).min(1)
        for k, v in enumerate((m2.sqrt(), mp.sqrt(), d2[:, 0].sqrt().mean(1), s2, sp)):
            out[k].append(v)
    return [torch.cat(o) for o in out]


def torch_vsd(v, f, view_e, view_g, depth, step):
    """vsd in plain torch ops on full-size renders: -> counts (N, 4 + T) i32"""
    fx, fy, cx, cy = K
    N = view_e.shape[0]
    light = torch.zeros((step, 3), device=DEV)
    ax = (torch.arange(W, device=DEV, dtype=torch.float32) - cx) / fx
    ay = (torch.arange(H, device=DEV, dtype=torch.float32) - cy) / fy
    c = torch.sqrt(ax[None, :] ** 2 + ay[:, None] ** 2 + 1.0)
    reading, Do = depth > 0, depth * c
    taus = torch.tensor(TAUS, device=DEV)
    rows = []
    for s in range(0, N, step):
        n = min(step, N - s)
        oe = onboard.render_views(v, f, None, None, view_e[s:s + n], light[:n], K, (H, W))
        og = onboard.render_views(v, f, None, None, view_g[s:s + n], light[:n], K, (H, W))
        has_e, has_g, De, Dg = oe["mask"] == 255, og["mask"] == 255, oe["depth"] * c, og["depth"] * c
        vg = has_g & (~reading | (Dg - Do <= DELTA))
        ve = has_e & (~reading | (De - Do <= DELTA) | vg)
        inter = ve & vg
        err = (Dg - De).abs() * (1.0 / DIAMETER)
        cost = (inter[:, None] & (err[:, None] >= taus[None, :, None, None])).sum((2, 3))
        rows.append(torch.cat([torch.stack([(ve | vg).sum((1, 2)), inter.sum((1, 2)), ve.sum((1, 2)), vg.sum((1, 2))], dim=1), cost], dim=1))
    return torch.cat(rows).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--slice", type=int, default=16)
    ap.add_argument("--only", default="both")
    args = ap.parse_args()
    print("%s, %d pose pairs on %d x %d, median of %d after 2 warm-ups, routes alternated" % (torch.cuda.get_device_name(0), args.poses, H, W, args.reps))
    vn, fn = RR.icosphere(6, 50.0)  # millimetres
    v, f = torch.from_numpy(vn).to(DEV), torch.from_numpy(fn).to(DEV)
    R, t = poses(args.poses, 0.6, 1.2)
    Re, te = estimates(R, t)
    est, gt = verify.pose_views(Re, te, SCALE), verify.pose_views(R, t, SCALE)
    if args.only in ("points", "both"):
        ring = dict(axis=[0, 0, 1], offset=[0, 0, 0])
        flip = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
        for name, syms, step in (("S = 1", poseerr.symmetry_transforms(), 50), ("S = 2", poseerr.symmetry_transforms(discrete=[flip]), 50),
                                 ("S = 1024", poseerr.symmetry_transforms(discrete=[flip], continuous=[ring], max_step=np.pi / 512), 1)):
            sy = torch.from_numpy(syms).to(DEV)
            print("pose_errors, V = %d, N = %d, %s: %.3g point transforms" % (v.shape[0], args.poses, name, float(v.shape[0]) * args.poses * len(syms)),
                  flush=True)
            alternate([("pose_errors", lambda: poseerr.pose_errors(v, Re, te, R, t, K, syms=sy, scale=SCALE, unit=DIAMETER)),
                       ("torch ops (slices of %d poses)" % step, lambda: torch_point_errors(v, est, gt, sy, step))], args.reps)
            got, ref = poseerr.pose_errors(v, Re, te, R, t, K, syms=sy, scale=SCALE, unit=DIAMETER), torch_point_errors(v, est, gt, sy, step)
            print("  largest difference: mssd %.3g m, mspd %.3g px, add %.3g m; indices differ on %d + %d poses; n_skipped %d"
                  % (float((got.mssd - ref[0]).abs().max()), float((got.mspd - ref[1]).abs().max()), float((got.add - ref[2]).abs().max()),
                     int((got.mssd_sym != ref[3]).sum()), int((got.mspd_sym != ref[4]).sum()), int(got.n_skipped.sum())), flush=True)
    if args.only in ("vsd", "both"):
        plane = torch.full((H, W), 1.5, device=DEV)
        first = verify.render_compare((v, f), R, t, K, plane, tol=0.01, scale=SCALE)
        depth = torch.where(first.ids >= 0, first.depth, plane)  # what a sensor would see of the ground truths before a wall
        depth[:, :40] = 0.0                                      # and a strip without a reading
        print("vsd, F = %d, N = %d, T = %d" % (f.shape[0], args.poses, len(TAUS)), flush=True)
        run = lambda: poseerr.vsd((v, f), Re, te, R, t, K, depth, DELTA, TAUS, diameter=DIAMETER, scale=SCALE)  # noqa: E731
        alternate([("vsd", run), ("full size + torch ops (slices of %d pairs)" % args.slice, lambda: torch_vsd(v, f, est, gt, depth, args.slice))],
                  args.reps)
        (err, counts), ref = run(), torch_vsd(v, f, est, gt, depth, args.slice)
        print("  counts equal: %s (largest difference %d); mean vsd at tau = 0.05 .. 0.5: %s"
              % (bool(torch.equal(counts, ref)), int((counts - ref).abs().max()), [round(float(x), 3) for x in err.mean(0)]), flush=True)


if __name__ == "__main__":
    main()
