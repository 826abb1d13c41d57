"""Timing of sam6d_hip.posematch.pair_adi on the GPU, in the protocol of scratch/verify_timing.py (its
event_ms, alternate and poses are imported; estimates is scratch/poseerr_timing.py's): HIP events around each route, two warm-up
rounds, the routes alternated in one process, median of the timed rounds with minimum and maximum, and the peak allocation.

  models   the dense mesh (the 81 920-face icosphere, 40 962 vertices, 50 mm radius under metre poses) and 2048 of its vertices
           chosen by ops.furthest_point_sampling
  poses    n x n of one object: `spread` over the 1080 x 1920 view (a tenth of them near-duplicates of others, the rest other
           instances), n = 25 (config4's share per object) and n = 200; and 200 x 200 `one spot`: one translation, random rotations
  routes   pair_adi with a cap of 0.1 diameters, pair_adi without a cap, and the route that existed before: the pairs expanded on
           the device and fed to poseerr.adi 1024 a call.  The computed entries of the first two are compared bit for bit with the
           third, and the fraction of pairs the cap skipped is printed.

    python scratch/pair_adi_timing.py [--reps 9] [--only dense|fps] [--sizes 25,200]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openvino-sam-6d_amd"), os.path.join(ROOT, "scratch")]
from sam6d_hip import ops, poseerr, posematch  # noqa: E402
from tests import raster_ref as RR  # noqa: E402  (the icosphere)
from poseerr_timing import DIAMETER, SCALE, estimates  # noqa: E402
from verify_timing import DEV, alternate, poses  # noqa: E402

CAP = 0.1 * DIAMETER


def expanded_adi(v, R, t):
    """the route that existed: poseerr.adi on the expanded pair list, 1024 pairs a call -> adi_sum, adi (n,n)"""
    n = R.shape[0]
    Re, te, Rg, tg = R.repeat_interleave(n, dim=0), t.repeat_interleave(n, dim=0), R.repeat(n, 1, 1), t.repeat(n, 1)
    parts = [poseerr.adi(v, Re[k:k + 1024], te[k:k + 1024], Rg[k:k + 1024], tg[k:k + 1024], scale=SCALE, unit=DIAMETER) for k in range(0, n * n, 1024)]
    print(".", end="", file=sys.stderr, flush=True)  # a sign of life: a round of the dense 200 x 200 case takes many seconds
    return torch.cat([p.adi_sum for p in parts]).reshape(n, n), torch.cat([p.adi for p in parts]).reshape(n, n)


def spread(n):
    """n poses over the view, the last n // 10 of them near-duplicates of the first"""
    R, t = poses(n, 0.6, 1.2)
    k = n // 10
    if k:
        Rd, td = estimates(R[:k], t[:k])
        R, t = torch.cat([R[:n - k], Rd]).contiguous(), torch.cat([t[:n - k], td]).contiguous()
    return R, t


def one_spot(n):
    R, t = poses(n, 0.6, 1.2)
    return R, t[:1].repeat(n, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="both")
    ap.add_argument("--sizes", default="25,200")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    print("%s, median of %d after 2 warm-ups, routes alternated, cap = 0.1 diameters" % (torch.cuda.get_device_name(0), args.reps))
    vn, _ = RR.icosphere(6, 50.0)  # millimetres
    dense = torch.from_numpy(vn).to(DEV)
    pick = ops.furthest_point_sampling(dense[None], 2048)[0].long()
    models = [("dense", dense), ("fps", dense[pick].contiguous())]
    for name, v in models:
        if args.only not in (name, "both"):
            continue
        cases = [("spread", n, spread(n)) for n in sizes] + ([("one spot", 200, one_spot(200))] if 200 in sizes else [])
        for where, n, (R, t) in cases:
            print("pair_adi, %s, V = %d, %d x %d poses, %s" % (name, v.shape[0], n, n, where), flush=True)
            capped = lambda: posematch.pair_adi(v, R, t, R, t, scale=SCALE, unit=DIAMETER, cap=CAP)  # noqa: E731
            plain = lambda: posematch.pair_adi(v, R, t, R, t, scale=SCALE, unit=DIAMETER)  # noqa: E731
            alternate([("pair_adi, cap", capped), ("pair_adi, no cap", plain), ("adi, expanded pairs, 1024 a call", lambda: expanded_adi(v, R, t))],
                      args.reps)
            got, bare, (old_sum, old_adi) = capped(), plain(), expanded_adi(v, R, t)
            keep = ~got.skipped
            same = (torch.equal(bare.adi_sum, old_sum) and torch.equal(bare.adi.view(torch.int32), old_adi.view(torch.int32))
                    and torch.equal(got.adi_sum[keep], old_sum[keep]) and torch.equal(got.adi[keep].view(torch.int32), old_adi[keep].view(torch.int32)))
            below = int((old_adi < CAP).sum())
            print("  skipped %.4f of the pairs; %d of %d pairs are below the cap, none of them skipped: %s; bit for bit against the old route: %s"
                  % (float(got.skipped.float().mean()), below, n * n, not bool((got.skipped & (old_adi < CAP)).any()), same), flush=True)


if __name__ == "__main__":
    main()
