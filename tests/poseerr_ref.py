"""Numpy restatement of the pose errors (csrc/poseerr.hip, sam6d_hip.poseerr), code of its own: the recipe at the top of poseerr.hip,
float32 operation by operation in the order written there (every float array is float32 and every constant wrapped in np.float32, so
numpy rounds each operation once, as the device does without fused multiply-adds), float64 where the recipe names it, integers
elsewhere.  VSD builds its two z-buffers per pair from tests/verify_ref.py's window_zbuffer.  The definitions are the published ones
(Hodan et al., BOP Challenge 2020; ADD: Hinterstoisser et al. 2012); nothing here is bop_toolkit's code or checked against it.

    G      = fl32(gt[n] o syms[s]), the float64 sums left to right
    e, g   = ((M_r0 x0 + M_r1 x1) + M_r2 x2) + M_r3;  d2 = (dx dx + dy dy) + dz dz;  u = fx * (x / z) + cx;  p2 = du du + dv dv
    maxima of bit patterns (> 0: the bits, 0: 0, else 0x7fc00000); a point with e_z > 0 or g_z > 0 false is left out of the p2 maximum
    mssd   = sqrt(min_s max_x d2), the lowest s on a tie;  add_sum = sum_x rint(min(float64(sqrt(d2 at s = 0)) * inv_unit * 2^30, 2^42))
    vsd    D = z * sqrt((ax ax + ay ay) + 1), ax = (float(x) - cx) / fx;  visib_gt = has_g & (~reading | (D_g - D_o <= delta));
           visib_est = has_e & (~reading | (D_e - D_o <= delta) | visib_gt);  cost_k = inter & (|D_g - D_e| * inv_norm >= tau_k)

THE BOUNDS of the float64 comparison (tests/test_poseerr_host.py) follow from the unit roundoff u = 2^-24 and the operand magnitudes;
first-order terms are written out and the sum is doubled for the higher orders, which are below u times it.
  A row of M x has three products and three sums: its error is at most 4 u B with B >= sum_c |M_rc| |x_c| + |M_r3|.  G is rounded
  once from float64 (u B more for g), so a component of d = e - g is off by at most 4 u B + 5 u B + u |d_c| <= 11 u B (|d_c| <= 2 B)
  and |d| by sqrt(3) 11 u B.  d2 has three products and two sums, the square root halves the relative error and adds u: 3 u |d|
  <= 3 u 2 sqrt(3) B.  max and min do not enlarge a bound that holds for every element.  So
      |mssd - exact| <= (11 + 6) sqrt(3) u B < 30 u B, doubled: 60 u B.
  ADD: the same per point, plus 2^-31 / inv_unit per term for the rint, plus u add for the float32 the module returns.
  A pixel coordinate u = fx * (x / z) + cx with z >= zmin and |x / z| <= Q: x and z are off by at most 5 u B each (the larger, g's), the
  quotient by 5 u B (1 + Q) / zmin + u Q, the product and the sum add u (fx Q) + u (fx Q + |cx|).  With P = fx Q + |cx| a coordinate
  is off by at most fx 5 u B (1 + Q) / zmin + 3 u P, a difference of two by twice that plus u 2 P, the distance by sqrt(2) of it plus
  3 u 2 sqrt(2) P:
      |mspd - exact| <= sqrt(2) (10 u fx B (1 + Q) / zmin + 8 u P) + 6 sqrt(2) u P < 15 u fx B (1 + Q) / zmin + 20 u P, doubled.
"""
import numpy as np

from tests import raster_ref as RR
from tests import verify_ref as VR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
NAN_BITS = np.uint32(0x7FC00000)
ADD_SCALE = 2.0 ** 30
TERM_MAX = 2.0 ** 42
VSD_COLUMNS = ("n_union", "n_inter", "n_visib_est", "n_visib_gt")


def mssd_bound(B):
    return 60.0 * U * B


def add_bound(B, inv_unit, add):
    return mssd_bound(B) + 2.0 ** -31 / inv_unit + 2.0 * U * add


def mspd_bound(B, zmin, Q, f, c):
    return 2.0 * (15.0 * U * f * B * (1.0 + Q) / zmin + 20.0 * U * (f * Q + abs(c)))


# ------------------------------------------------------------------------------------------------------------ point errors
def sym_gt(gt, syms):
    """(N,3,4), (S,3,4) float32 -> G (N,S,3,4) float32"""
    g, s = np.asarray(gt, F32).astype(F64)[:, None], np.asarray(syms, F32).astype(F64)[None]
    out = np.empty((g.shape[0], s.shape[1], 3, 4), F64)
    for r in range(3):
        for c in range(4):
            a = g[..., r, 0] * s[..., 0, c]
            a = a + g[..., r, 1] * s[..., 1, c]
            a = a + g[..., r, 2] * s[..., 2, c]
            if c == 3:
                a = a + g[..., r, 3]
            out[..., r, c] = a
    return out.astype(F32)


def transform(M, x):
    """M (...,3,4), x (V,3) float32 -> (...,V,3) float32"""
    M = np.asarray(M, F32)[..., None, :, :]
    x0, x1, x2 = (np.asarray(x, F32)[:, k] for k in range(3))
    return np.stack([((M[..., r, 0] * x0 + M[..., r, 1] * x1) + M[..., r, 2] * x2) + M[..., r, 3] for r in range(3)], axis=-1)


def project(p, intr):
    fx, fy, cx, cy = (F32(v) for v in intr)
    with np.errstate(all="ignore"):
        return fx * (p[..., 0] / p[..., 2]) + cx, fy * (p[..., 1] / p[..., 2]) + cy


def bits(v):
    """the word a value offers to a maximum"""
    v = np.ascontiguousarray(v, F32)
    with np.errstate(all="ignore"):
        return np.where(v > 0, v.view(np.uint32), np.where(v == 0, np.uint32(0), NAN_BITS)).astype(np.uint32)


def point_errors(points, est, gt, syms, intr, inv_unit=1.0):
    """sam6d_pose_point_errors -> dict of mssd, mspd (N) float32, mssd_sym, mspd_sym, n_skipped (N) int32, add_sum (N) int64"""
    points, est = np.asarray(points, F32), np.asarray(est, F32)
    with np.errstate(all="ignore"):
        e = transform(est, points)[:, None]            # (N,1,V,3)
        g = transform(sym_gt(gt, syms), points)        # (N,S,V,3)
        d = e - g
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ue, ve = project(e, intr)
        ug, vg = project(g, intr)
        du, dv = ue - ug, ve - vg
        p2 = du * du + dv * dv
        skip = ~((e[..., 2] > 0) & (g[..., 2] > 0))
        m2 = bits(d2).max(axis=2)                                                  # (N,S)
        mp = np.where(skip, np.uint32(0), bits(p2)).max(axis=2)
        w = (np.sqrt(d2[:, 0]).astype(F64) * F64(F32(inv_unit))) * ADD_SCALE
        w = np.where(w <= TERM_MAX, w, TERM_MAX)
        s2, sp = m2.argmin(axis=1), mp.argmin(axis=1)                              # the first minimum: the lowest s
        rows = np.arange(len(est))
        return dict(mssd=np.sqrt(m2[rows, s2].view(F32)), mspd=np.sqrt(mp[rows, sp].view(F32)), mssd_sym=s2.astype(np.int32),
                    mspd_sym=sp.astype(np.int32), n_skipped=skip[:, 0].sum(axis=1).astype(np.int32),
                    add_sum=np.rint(w).astype(np.int64).sum(axis=1))


def add_of(add_sum, inv_unit, V):
    """what sam6d_hip.poseerr returns as `add`"""
    return (np.asarray(add_sum, np.int64).astype(F64) / ADD_SCALE / float(F32(inv_unit)) / V).astype(F32)


# ------------------------------------------------------------------------------------------------------------ VSD
def union_box(a, b):
    ea, eb = a[2] < a[0] or a[3] < a[1], b[2] < b[0] or b[3] < b[1]
    if ea and eb:
        return [0, 0, -1, -1]
    if ea or eb:
        return [int(v) for v in (b if ea else a)]
    return [min(int(a[0]), int(b[0])), min(int(a[1]), int(b[1])), max(int(a[2]), int(b[2])), max(int(a[3]), int(b[3]))]


def pair_boxes(vert, faces, view, intr, size, near=1e-3):
    """view (2N,3,4): estimates then ground truths -> the (N,4) int32 union of each pair's windows"""
    box = VR.windows(vert, faces, view, intr, size, near)[0]
    N = len(box) // 2
    return np.array([union_box(box[n], box[N + n]) for n in range(N)], np.int32).reshape(N, 4)


def vsd_pixels(zb_e, zb_g, obs, x0, y0, intr, delta, taus, inv_norm):
    """the masks of one window: union, inter, visib_est, visib_gt, and the (T,) + shape cost masks"""
    fx, fy, cx, cy = (F32(v) for v in intr)
    bh, bw = zb_e.shape
    has_e, has_g = zb_e != VR.EMPTY, zb_g != VR.EMPTY
    with np.errstate(all="ignore"):
        ax = (np.arange(x0, x0 + bw).astype(F32) - cx) / fx
        ay = (np.arange(y0, y0 + bh).astype(F32) - cy) / fy
        c = np.sqrt((ax[None, :] * ax[None, :] + ay[:, None] * ay[:, None]) + F32(1))
        De, Dg, Do = VR.key_depth(zb_e) * c, VR.key_depth(zb_g) * c, np.asarray(obs, F32) * c
        reading = np.asarray(obs, F32) > 0
        vg = has_g & (~reading | (Dg - Do <= F32(delta)))
        ve = has_e & (~reading | (De - Do <= F32(delta)) | vg)
        inter = ve & vg
        err = np.abs(Dg - De) * F32(inv_norm)
        cost = np.stack([inter & (err >= F32(t)) for t in taus])
    return ve | vg, inter, ve, vg, cost


def vsd_counts(vert, faces, view, intr, size, near, depth_obs, delta, taus, inv_norm=1.0, box=None):
    """sam6d_pose_vsd with the windows sam6d_hip.poseerr.vsd gives it (box: other (N,4) pair windows)
    -> counts (N, 4+T) int32"""
    view = np.asarray(view, F32).reshape(-1, 3, 4)
    N, T = len(view) // 2, len(taus)
    box = pair_boxes(vert, faces, view, intr, size, near) if box is None else np.asarray(box)
    counts = np.zeros((N, 4 + T), np.int32)
    if VR.areas(box, size).sum() == 0:
        return counts
    depth_obs = np.asarray(depth_obs, F32)
    setups = VR._setups(vert, faces, view, intr, size, near)
    for n in range(N):
        x0, y0, bw, bh = VR.clamp_box(box[n], size)
        if bw == 0:
            continue
        win = (x0, y0, bw, bh)
        uni, inter, ve, vg, cost = vsd_pixels(VR.window_zbuffer(setups[n], win), VR.window_zbuffer(setups[N + n], win),
                                              depth_obs[y0:y0 + bh, x0:x0 + bw], x0, y0, intr, delta, taus, inv_norm)
        counts[n, :4] = [uni.sum(), inter.sum(), ve.sum(), vg.sum()]
        counts[n, 4:] = cost.sum(axis=(1, 2))
    return counts


def vsd_of(counts):
    """what sam6d_hip.poseerr returns as `vsd`: (cost_k + n_union - n_inter) / n_union in float32, 1 where n_union is 0"""
    c = np.asarray(counts)
    num = (c[:, 4:] + (c[:, 0:1] - c[:, 1:2])).astype(F32)
    with np.errstate(all="ignore"):
        return np.where(c[:, 0:1] > 0, num / c[:, 0:1].astype(F32), F32(1)).astype(F32)


def views(R, t):
    return np.concatenate([np.asarray(R, F32), np.asarray(t, F32)[:, :, None]], axis=2)
