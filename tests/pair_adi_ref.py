"""Numpy restatement of all-pairs ADI with its cap (csrc/pairadi.hip, sam6d_hip.posematch.pair_adi / nms_poses_adi), code of its own,
plain loops over the pairs.  The full table, the boxes, the lower bound and the terms are tests/nearest_ref.py's, the point transform
and the float32 `adi` tests/poseerr_ref.py's, the NMS tests/posematch_ref.py's -- imported, not copied: each recipe has one
restatement.  The definition is the published one (ADI: Hinterstoisser et al. 2012, Hodan et al. 2016), over the vertices; nothing
here is bop_toolkit's code or checked against it.

    adi_sum[i][j]    nearest_ref's full V x V table for E = a[i], G = b[j]
    lb_i             min over ALL tiles t of b[j] of nearest_ref.lower_bound(e_i, lo_t, hi_t), from +inf (fmin)
    lower_sum[i][j]  sum_i nearest_ref.terms(lb_i)
    cap_sum          floor(float64(cap) * float64(float32(inv_unit)) * 2^30 * V), at most 2^63 - 1
    skipped          lower_sum > cap_sum: adi = +inf, adi_sum = -1
    NMS              posematch_ref.nms on the matrix capped at thresh * (1 + 2^-20)

The poses are (N,3,4) float32 view matrices (scale 1).  `order` is the order of the points the search runs in: lower_sum belongs to
its tiles, adi_sum does not depend on it.  morton_order restates sam6d_hip.poseerr.morton_order in numpy float32.
"""
import functools

import numpy as np

from tests import nearest_ref as NR
from tests import posematch_ref as MR
from tests import poseerr_ref as PR
from tests import verify_ref as VR

F32, F64 = np.float32, np.float64
INT64_MAX = (1 << 63) - 1
NMS_MARGIN = 2.0 ** -20
UNIT = 2.0
INV_UNIT = F32(1.0 / UNIT)


# ------------------------------------------------------------------------------------------------------------ the recipes
def _spread10(q):
    q = (q | (q << 16)) & 0x30000FF
    q = (q | (q << 8)) & 0x300F00F
    q = (q | (q << 4)) & 0x30C30C3
    return (q | (q << 2)) & 0x9249249


def morton_order(points):
    """sam6d_hip.poseerr.morton_order: 10 bits per axis over the bounding box (one step, the longest side's), a stable argsort"""
    x = np.nan_to_num(np.asarray(points, F32), nan=0.0, posinf=0.0, neginf=0.0).astype(F32)
    lo = x.min(axis=0)
    span = np.maximum((x.max(axis=0) - lo).max(), F32(1e-30)).astype(F32)
    q = np.clip((x - lo) / span * F32(1023.0), F32(0.0), F32(1023.0)).astype(np.int64)
    return np.argsort(_spread10(q[:, 0]) | (_spread10(q[:, 1]) << 1) | (_spread10(q[:, 2]) << 2), kind="stable")


def _under(poses, points):
    with np.errstate(all="ignore"):
        return [PR.transform(M, points) for M in np.asarray(poses, F32).reshape(-1, 3, 4)]


def pair_adi_sum(points, a, b, inv_unit=1.0):
    """-> (A,B) int64 by the full table of every pair"""
    points = np.asarray(points, F32)
    ea, gb = _under(a, points), _under(b, points)
    out = np.zeros((len(ea), len(gb)), np.int64)
    for i, e in enumerate(ea):
        for j, g in enumerate(gb):
            out[i, j] = NR.terms(NR.nearest_d2(e, g), inv_unit).sum()
    return out


def point_lower_bounds(e, g):
    """e, g (V,3) float32 -> lb (V) float32: the minimum over all tiles of g of the tile's lower bound, from +inf"""
    lo, hi = NR.boxes(g)
    lb = np.full(len(e), NR.INF, F32)
    for t in range(len(lo)):
        lb = np.fmin(lb, NR.lower_bound(e, lo[t], hi[t]))
    return lb


def pair_lower_sum(points, a, b, inv_unit=1.0, order=None):
    """-> (A,B) int64; the tiles are those of points[order]"""
    points = np.asarray(points, F32)
    if order is not None:
        points = points[np.asarray(order)]
    ea, gb = _under(a, points), _under(b, points)
    out = np.zeros((len(ea), len(gb)), np.int64)
    for i, e in enumerate(ea):
        for j, g in enumerate(gb):
            out[i, j] = NR.terms(point_lower_bounds(e, g), inv_unit).sum()
    return out


def cap_sum(cap, inv_unit, V):
    with np.errstate(all="ignore"):
        x = ((F64(cap) * F64(F32(inv_unit))) * F64(PR.ADD_SCALE)) * F64(V)
    return INT64_MAX if x >= 2.0 ** 63 else int(np.floor(x))


def capped(full_sum, lower_sum, cap, inv_unit, V):
    """the outputs of pair_adi from the uncapped table and lower_sum -> dict adi_sum, lower_sum, skipped, adi"""
    full_sum = np.asarray(full_sum, np.int64)
    if cap is None:
        skipped, lower_sum = np.zeros(full_sum.shape, bool), None
    else:
        skipped = np.asarray(lower_sum, np.int64) > cap_sum(cap, inv_unit, V)
    adi_sum = np.where(skipped, np.int64(-1), full_sum)
    adi = np.where(skipped, F32(np.inf), NR.adi_of(full_sum, inv_unit, V)).astype(F32)
    return dict(adi_sum=adi_sum, lower_sum=lower_sum, skipped=skipped, adi=adi)


def pair_adi(points, a, b, inv_unit=1.0, cap=None, order=None):
    """sam6d_hip.posematch.pair_adi -> dict adi_sum, lower_sum (None without a cap), skipped, adi"""
    V = len(points)
    lower = None if cap is None else pair_lower_sum(points, a, b, inv_unit, order)
    return capped(pair_adi_sum(points, a, b, inv_unit), lower, cap, inv_unit, V)


def nms_cap(thresh):
    return float(thresh) * (1.0 + NMS_MARGIN)


def nms_adi(points, poses, scores, thresh, inv_unit=1.0, order=None):
    """sam6d_hip.posematch.nms_poses_adi -> (keep_idx, count, suppressed_by), the capped adi matrix"""
    adi = pair_adi(points, poses, poses, inv_unit, nms_cap(thresh), order)["adi"]
    return MR.nms(adi, scores, thresh), adi


# ------------------------------------------------------------------------------------------------------------ shared scenes
HALF_TURN = np.diag([-1.0, -1.0, 1.0])
KINDS_A = ("mid", "half", "nan", "far", "identical", "near")
KINDS_B = ("identical", "far", "near", "nan", "mid", "half")
CAPS = (0.03, 1.0)   # in the unit of t: below and above the lower bound of a pose half a diameter away (`mid`)


def symmetric_points(V, seed=0, extent=(1.0, 0.5, 0.25)):
    """V points in a cuboid with the half extents `extent`, the set mapped onto itself by a half turn about z: pairs (x, y, z),
    (-x, -y, z), and for an odd V one point on the axis.  In random order"""
    g = np.random.default_rng(seed)
    half = g.uniform(-1.0, 1.0, (V // 2, 3)).astype(F32) * F32(extent)
    pts = np.concatenate([half, half * F32([-1.0, -1.0, 1.0])] + ([F32([[0.0, 0.0, 0.125]])] if V % 2 else []))
    return np.ascontiguousarray(pts[g.permutation(V)], F32)


def _variant(base, kind, g):
    R, t = base[:, :3].astype(F64), base[:, 3].astype(F64)
    if kind == "near":     # a few mrad and 1 % of the radius
        R, t = VR.rotation(g.normal(size=3), 0.003) @ R, t + g.normal(size=3) * 0.006
    elif kind == "half":   # the same pose for a set with the half-turn symmetry
        R = R @ HALF_TURN
    elif kind == "far":    # several diameters
        t = t + np.array([7.0, -5.0, 9.0])
    elif kind == "mid":    # half a diameter
        t = t + np.array([0.9, 0.5, -0.4])
    M = np.concatenate([R, t[:, None]], axis=1).astype(F32)
    if kind == "nan":
        M[0, 3] = np.nan
    return M


def pose_sets(A, B, seed=0):
    """a (A,3,4), b (B,3,4) float32 about one base pose: a mix of the kinds above, dealt in the order of KINDS_A and KINDS_B"""
    g = np.random.default_rng(1000 + seed)
    base = VR.pose((0.2, -0.1, 6.0), axis=g.normal(size=3), angle=1.1)
    a = np.stack([_variant(base, KINDS_A[i % len(KINDS_A)], g) for i in range(A)])
    b = np.stack([_variant(base, KINDS_B[j % len(KINDS_B)], g) for j in range(B)])
    return a, b


@functools.lru_cache(maxsize=None)
def scene(V, A, B):
    """the inputs the host and the GPU test share, and the uncapped table -> points, a, b, adi_sum (A,B); leave them unchanged"""
    pts = symmetric_points(V, seed=V)
    a, b = pose_sets(A, B, seed=V)
    return pts, a, b, pair_adi_sum(pts, a, b, INV_UNIT)


@functools.lru_cache(maxsize=None)
def scene_lower(V, A, B, sort):
    """lower_sum (A,B) of scene(V, A, B) for the points as given or in morton_order"""
    pts, a, b, _ = scene(V, A, B)
    return pair_lower_sum(pts, a, b, INV_UNIT, morton_order(pts) if sort else None)


def nms_scene():
    """V = 257, eight poses: every kind above, two of them twice; the scores put a duplicate first -> points, poses (8,3,4), scores"""
    pts = symmetric_points(257, seed=3)
    a, b = pose_sets(6, 2, seed=3)
    return pts, np.concatenate([a, b]), F32([0.5, 0.9, 0.1, 0.8, 0.7, 0.6, 0.95, 0.3])


def cuboid_case():
    """The use case: a cuboid point set with no symmetry annotation, two poses half a turn about its axis apart and one distinct pose
    -> points (512,3), poses (3,3,4), scores (3), thresh (a tenth of the diameter, in the unit of t)"""
    pts = symmetric_points(512, seed=77)
    g = np.random.default_rng(78)
    base = VR.pose((0.0, 0.1, 5.0), axis=g.normal(size=3), angle=0.8)
    poses = np.stack([base, _variant(base, "half", g), _variant(base, "mid", g)])
    return pts, poses, F32([0.9, 0.8, 0.7]), 0.1 * float(NR.diameter(pts))
