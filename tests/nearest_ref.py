"""Numpy restatement of ADI and the model diameter (csrc/nearest.hip, sam6d_hip.poseerr.adi / model_diameter), code of its own: the
recipe at the top of nearest.hip by brute force over the full V x V table, float32 operation by operation in the order written there
(every float array is float32, so numpy rounds each operation once, as the device does without fused multiply-adds), float64 where
the recipe names it, integers elsewhere.  The definitions are the published ones (ADI: Hinterstoisser et al. 2012, Hodan et al. 2016;
the diameter: the largest distance between two vertices, as bop_toolkit computes it); nothing here is bop_toolkit's code or checked
against it.

    e_i = E x_i, g_j = G x_j (poseerr_ref.transform);  d2_ij = (dx dx + dy dy) + dz dz
    ADI       m_i = min_j d2_ij from +inf, a NaN never wins;  adi_sum = sum_i rint(min(float64(sqrt(m_i)) * inv_unit * 2^30, 2^42))
    diameter  sqrt(max_ij of the words poseerr_ref.bits gives d2_ij = |x_i - x_j|^2)

THE SKIP RULE is restated too (boxes, lower_bound, upper_bound, adi_walk, diameter_walk), so that the tests can show that it never
changes a result and that it fires: tiles of 256 consecutive points, per tile the box lo, hi of its actual float32 points (NaN
ignored, an empty box lo = +inf, hi = -inf);
    gap_k = e_k - hi_k where e_k > hi_k, lo_k - e_k where e_k < lo_k, else 0;   lb = (gap_x gap_x + gap_y gap_y) + gap_z gap_z
    u_k = fmax(|x_k - lo_k|, |x_k - hi_k|);                                      ub = (u_x u_x + u_y u_y) + u_z u_z
a workgroup (1024 points) walks a tile unless every one of its points has lb > m (ADI), or has ub <= L and finite coordinates (the
diameter; L the seeds' maximum).  Rounding to nearest is monotone, so lb <= d2_ij <= ub hold in float32 as they stand.

THE BOUNDS of the float64 comparison (tests/test_nearest_host.py).  poseerr_ref.mssd_bound(B) bounds the error of ONE distance
sqrt(d2) between two transformed points whose rows have operand magnitude at most B; it holds for every d_ij of the table, and
neither min_j nor max_ij enlarges a bound that holds for every element (|min a - min b| <= max |a_j - b_j|).  So
    |sqrt(m_i) - exact_i| <= mssd_bound(B),   |diameter - exact| <= mssd_bound(B) with B = max |x_c| (no transform: the bound is generous)
and ADI adds what ADD adds (poseerr_ref.add_bound): 2^-31 / inv_unit per term for the rint, u adi for the float32 the module returns.
"""
import numpy as np

from tests import poseerr_ref as PR

F32, F64 = np.float32, np.float64
TILE = 256
CHUNK = 1024
INF = F32(np.inf)


def adi_bound(B, inv_unit, adi):
    return PR.add_bound(B, inv_unit, adi)


def diameter_bound(B):
    return PR.mssd_bound(B)


# ------------------------------------------------------------------------------------------------------------ the recipes
def d2_table(a, b):
    """a (A,3), b (B,3) float32 -> (A,B) float32"""
    with np.errstate(all="ignore"):
        d = np.asarray(a, F32)[:, None, :] - np.asarray(b, F32)[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_d2(e, g, rows=512):
    """m_i = min_j d2_ij from +inf, NaN ignored: (V) float32"""
    return np.concatenate([np.fmin.reduce(d2_table(e[i:i + rows], g), axis=1, initial=INF) for i in range(0, len(e), rows)])


def terms(m, inv_unit):
    with np.errstate(all="ignore"):
        w = (np.sqrt(np.asarray(m, F32)).astype(F64) * F64(F32(inv_unit))) * PR.ADD_SCALE
        return np.rint(np.where(w <= PR.TERM_MAX, w, PR.TERM_MAX)).astype(np.int64)


def adi_sum(points, est, gt, inv_unit=1.0):
    """sam6d_pose_adi -> adi_sum (N) int64, by the full table"""
    points = np.asarray(points, F32)
    with np.errstate(all="ignore"):
        return np.array([terms(nearest_d2(PR.transform(E, points), PR.transform(G, points)), inv_unit).sum()
                         for E, G in zip(np.asarray(est, F32), np.asarray(gt, F32))], np.int64)


def adi_of(adi_sum, inv_unit, V):
    """what sam6d_hip.poseerr.adi returns as `adi`"""
    return PR.add_of(adi_sum, inv_unit, V)


def diameter_bits(points, rows=512):
    points = np.asarray(points, F32)
    return max(int(PR.bits(d2_table(points[i:i + rows], points)).max()) for i in range(0, len(points), rows))


def diameter(points):
    """sam6d_points_diameter -> float32, by the full table"""
    with np.errstate(all="ignore"):
        return np.sqrt(np.array([diameter_bits(points)], np.uint32).view(F32))[0]


# ------------------------------------------------------------------------------------------------------------ the skip rule
def boxes(p):
    """p (V,3) float32 -> lo, hi (T,3) float32 of the tiles of 256 consecutive points"""
    p = np.asarray(p, F32)
    T = (len(p) + TILE - 1) // TILE
    lo = np.stack([np.fmin.reduce(p[t * TILE:(t + 1) * TILE], axis=0, initial=INF) for t in range(T)])
    hi = np.stack([np.fmax.reduce(p[t * TILE:(t + 1) * TILE], axis=0, initial=-INF) for t in range(T)])
    return lo.astype(F32), hi.astype(F32)


def lower_bound(e, lo, hi):
    """e (...,3), lo, hi (3) float32 -> lb (...) float32"""
    e = np.asarray(e, F32)
    with np.errstate(all="ignore"):
        gap = np.where(e > hi, e - hi, np.where(e < lo, lo - e, F32(0))).astype(F32)
        return (gap[..., 0] * gap[..., 0] + gap[..., 1] * gap[..., 1]) + gap[..., 2] * gap[..., 2]


def upper_bound(x, lo, hi):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        u = np.fmax(np.abs(x - lo), np.abs(x - hi)).astype(F32)
        return (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]


def adi_walk(points, E, G, prune=True):
    """One pose as nn_adi_kernel walks it: -> m (V) float32, walked (chunks, T) bool.  Chunk c takes tile (4 c + s) mod T at step s."""
    points = np.asarray(points, F32)
    with np.errstate(all="ignore"):
        e, g = PR.transform(np.asarray(E, F32), points), PR.transform(np.asarray(G, F32), points)
        lo, hi = boxes(g)
        T, C = len(lo), (len(points) + CHUNK - 1) // CHUNK
        m, walked = np.full(len(points), INF, F32), np.zeros((C, T), bool)
        for c in range(C):
            rows = slice(c * CHUNK, (c + 1) * CHUNK)
            for s in range(T):
                t = (c * (CHUNK // TILE) + s) % T
                if prune and (lower_bound(e[rows], lo[t], hi[t]) > m[rows]).all():
                    continue
                walked[c, t] = True
                m[rows] = np.fmin(m[rows], np.fmin.reduce(d2_table(e[rows], g[t * TILE:(t + 1) * TILE]), axis=1, initial=INF))
    return m, walked


def seed_bits(points, seeds):
    points = np.asarray(points, F32)
    ok = [s for s in seeds if 0 <= s < len(points)]
    return int(PR.bits(d2_table(points, points[ok])).max()) if ok else 0


def diameter_walk(points, seeds, prune=True):
    """The seed launch and nn_diameter_kernel's walk over the tile pairs (a, b), b >= the first tile of a's chunk: -> the maximum's
    word, walked (chunks, T) bool"""
    points = np.asarray(points, F32)
    with np.errstate(all="ignore"):
        seed = seed_bits(points, seeds)
        L = np.array([seed], np.uint32).view(F32)[0]
        lo, hi = boxes(points)
        T, C = len(lo), (len(points) + CHUNK - 1) // CHUNK
        best, walked = 0, np.zeros((C, T), bool)
        fin = np.isfinite(points).all(axis=1)
        for c in range(C):
            rows = slice(c * CHUNK, (c + 1) * CHUNK)
            for t in range(c * (CHUNK // TILE), T):
                if prune and ((upper_bound(points[rows], lo[t], hi[t]) <= L) & fin[rows]).all():
                    continue
                walked[c, t] = True
                best = max(best, int(PR.bits(d2_table(points[rows], points[t * TILE:(t + 1) * TILE])).max()))
    return max(seed, best), walked


def axis_seeds(points):
    """the seeds sam6d_hip.poseerr passes: the arg-min and arg-max vertex of each axis"""
    points = np.asarray(points, F32)
    return [int(i) for i in points.argmin(axis=0)] + [int(i) for i in points.argmax(axis=0)]


# ------------------------------------------------------------------------------------------------------------ shared scenes
def two_clusters(seed=0):
    """V = 2050 points in two balls of radius 1 whose centres are 50 radii apart: indices 0 .. 1023 the first ball, 1024 .. 2049 the
    second, each ordered along x, so that a chunk of 1024 points is one ball and a tile of 256 a slab of it; N = 3 ground truths and
    estimates 0.02 rad and 0.02 radii away.  -> points (2050,3), est, gt (3,3,4) float32"""
    from tests import verify_ref as VR
    g = np.random.default_rng(seed)

    def ball(n, centre):
        p = g.normal(size=(n, 3))
        p = p / np.linalg.norm(p, axis=1, keepdims=True) * g.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)
        return p[np.argsort(p[:, 0])] + centre
    pts = np.concatenate([ball(1024, (0.0, 0.0, 0.0)), ball(1026, (50.0, 0.0, 0.0))]).astype(F32)
    gt = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(80, 90)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(3)])
    est = []
    for M in gt:
        dR = VR.pose((0.0, 0.0, 0.0), axis=g.normal(size=3), angle=0.02)[:, :3].astype(F64)
        est.append(np.concatenate([dR @ M[:, :3].astype(F64), (M[:, 3].astype(F64) + g.normal(size=3) * 0.02)[:, None]], axis=1))
    return pts, np.stack(est).astype(F32), gt.astype(F32)
