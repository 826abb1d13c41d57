"""Timing of sam6d_hip.posematch on the GPU, in the protocol of scratch/verify_timing.py (its event_ms,
alternate and poses are imported; estimates and torch_point_errors are scratch/poseerr_timing.py's): HIP events around each route, two
warm-up rounds, the routes alternated in one process, median of the timed rounds with minimum and maximum, and the peak allocation.

  pair_errors   the A x B error matrix of config4's proposal count (A = B = 200 poses) over the dense mesh (the 81 920-face
                icosphere, 40 962 vertices, 50 mm radius under metre poses) with S = 1 and S = 64 symmetries, and over V = 512 of its
                vertices; with K (MSSD, MSPD, ADD) and without (MSSD, ADD).  Beside it the route that existed before: the A B pairs
                expanded on the device and fed to poseerr.pose_errors 1024 pairs a call (the yardstick), and the same pair list
                through plain torch ops in slices that fit.  The matrices of the first two routes are compared bit for bit.
  match_poses   1024 estimates against 1024 targets, 1 and 64 thresholds
  pose_nms      1024 poses, a matrix in which about half of them are kept

    python scratch/posematch_timing.py [--reps 9] [--poses 200] [--only pairs|match]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "scratch")]
from sam6d_hip import poseerr, posematch, verify  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)
from poseerr_timing import DIAMETER, SCALE, estimates, torch_point_errors  # noqa: E402
from verify_timing import DEV, K, alternate, poses  # noqa: E402

FIELDS = ("mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")


def expanded(Ra, ta, Rb, tb):
    """the A B pairs in row-major order, on the device"""
    A, B = Ra.shape[0], Rb.shape[0]
    return (Ra.repeat_interleave(B, dim=0), ta.repeat_interleave(B, dim=0), Rb.repeat(A, 1, 1), tb.repeat(A, 1))


def chunked_pose_errors(v, Ra, ta, Rb, tb, sy):
    """the route that existed: pose_errors on the expanded pair list, 1024 pairs a call -> dict of (A,B) tensors"""
    A, B = Ra.shape[0], Rb.shape[0]
    Re, te, Rg, tg = expanded(Ra, ta, Rb, tb)
    parts = [poseerr.pose_errors(v, Re[k:k + 1024], te[k:k + 1024], Rg[k:k + 1024], tg[k:k + 1024], K, syms=sy, scale=SCALE, unit=DIAMETER)
             for k in range(0, A * B, 1024)]
    return {f: torch.cat([getattr(p, f) for p in parts]).reshape(A, B) for f in FIELDS}


def chunked_torch(v, Ra, ta, Rb, tb, sy, step):
    Re, te, Rg, tg = expanded(Ra, ta, Rb, tb)
    return torch_point_errors(v, verify.pose_views(Re, te, SCALE), verify.pose_views(Rg, tg, SCALE), sy, step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--only", default="both")
    args = ap.parse_args()
    n = args.poses
    print("%s, A = B = %d poses, median of %d after 2 warm-ups, routes alternated" % (torch.cuda.get_device_name(0), n, args.reps))
    if args.only in ("pairs", "both"):
        vn, _ = RR.icosphere(6, 50.0)  # millimetres
        dense = torch.from_numpy(vn).to(DEV)
        pick = np.random.default_rng(0).choice(len(vn), 512, replace=False)
        small = torch.from_numpy(np.ascontiguousarray(vn[np.sort(pick)])).to(DEV)
        Rb, tb = poses(n, 0.6, 1.2)
        Ra, ta = estimates(Rb, tb)
        ring = dict(axis=[0, 0, 1], offset=[0, 0, 0])
        flip = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
        s1, s64 = poseerr.symmetry_transforms(), poseerr.symmetry_transforms(discrete=[flip], continuous=[ring], max_step=np.pi / 32)
        assert len(s64) == 64
        for v, syms, step in ((dense, s1, 200), (dense, s64, 16), (small, s1, 2000), (small, s64, 400)):
            sy = torch.from_numpy(syms).to(DEV)
            V, S = v.shape[0], len(syms)
            print("pair_errors, V = %d, A = B = %d, S = %d: %.3g point transforms, %d pose_errors calls on the old route"
                  % (V, n, S, float(V) * n * n * S, (n * n + 1023) // 1024), flush=True)
            new = lambda: posematch.pair_errors(v, Ra, ta, Rb, tb, K=K, syms=sy, scale=SCALE, unit=DIAMETER)  # noqa: E731
            alternate([("pair_errors (MSSD, MSPD, ADD)", new),
                       ("pair_errors without K (MSSD, ADD)", lambda: posematch.pair_errors(v, Ra, ta, Rb, tb, syms=sy, scale=SCALE, unit=DIAMETER)),
                       ("pose_errors, expanded pairs, 1024 a call", lambda: chunked_pose_errors(v, Ra, ta, Rb, tb, sy)),
                       ("torch ops, expanded pairs (slices of %d)" % step, lambda: chunked_torch(v, Ra, ta, Rb, tb, sy, step))], args.reps)
            got, old = new(), chunked_pose_errors(v, Ra, ta, Rb, tb, sy)
            bare = posematch.pair_errors(v, Ra, ta, Rb, tb, syms=sy, scale=SCALE, unit=DIAMETER)
            print("  bit for bit against the old route: %s; without K: %s" % (all(torch.equal(getattr(got, f), old[f]) for f in FIELDS),
                  all(torch.equal(getattr(bare, f), old[f]) for f in ("mssd", "mssd_sym", "add_sum"))), flush=True)
    if args.only in ("match", "both"):
        g = torch.Generator(device="cpu").manual_seed(0)
        N = 1024
        err = torch.rand((N, N), generator=g).to(DEV)
        scores = torch.rand((N,), generator=g).to(DEV)
        for T in (1, 64):
            thr = torch.linspace(0.001, 0.05, T).to(DEV) if T > 1 else torch.tensor([0.01], device=DEV)
            print("match_poses, A = B = %d, T = %d" % (N, T), flush=True)
            alternate([("match_poses", lambda: posematch.match_poses(err, scores, thr))], args.reps)
            print("  matched: %s" % posematch.match_poses(err, scores, thr).n_matched.tolist()[::max(1, T // 8)], flush=True)
        print("pose_nms, N = %d" % N, flush=True)
        alternate([("pose_nms", lambda: posematch.pose_nms(err, scores, 2.0 / N))], args.reps)
        print("  kept: %d" % int(posematch.pose_nms(err, scores, 2.0 / N).count), flush=True)


if __name__ == "__main__":
    main()
