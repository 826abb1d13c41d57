"""Numpy restatement of the all-pairs VSD (csrc/vsdpairs.hip, sam6d_hip.posematch.pair_vsd), code of its own: every view is rendered
ONCE, into its own window (tests/verify_ref.py's window_zbuffer), D, has and own are formed per view, and a pair's counts come from the
per-view totals and a walk over the rectangle the two windows share.  float32 operation by operation in the order of the recipe at the
top of vsdpairs.hip, integers elsewhere; plain loops over the pairs, no attempt at speed.

    per view   has = a key is there;  c = sqrt((ax ax + ay ay) + 1), ax = (float(x) - cx) / fx;  D = r * c, D_o = o * c
               own = has & (~reading | (D - D_o <= delta)), reading = o > 0;  view_counts = #has, #own
    per pair   X = the intersection of the windows of a[i] and b[j];  E = #own of a[i], G = #own of b[j]
               n_inter = #X{has_e & own_g};  n_visib_est = E + #X{has_e & ~own_e & own_g};  n_visib_gt = G
               n_union = n_visib_est + G - n_inter;  cost_k = #X{has_e & own_g & (|D_g - D_e| * inv_norm >= tau_k)}

The independent route to the same integers is tests/poseerr_ref.py's vsd_counts on the expanded pairs (union windows, two renders per
pair): tests/test_vsdpairs_host.py compares the two.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests import raster_ref as RR
from tests import refine_ref as RF
from tests import verify_ref as VR

F32 = np.float32
NEAR = 1e-3
DELTA = 2.0 ** -6  # with depths in [2, 4) every z - DELTA is a float32


def view_images(vert, faces, view, intr, size, near, depth_obs, delta):
    """per view: win = (x0, y0, bw, bh) its own window, and has, own (bh, bw) bool, D (bh, bw) float32 over it"""
    fx, fy, cx, cy = (F32(v) for v in intr)
    depth_obs = np.asarray(depth_obs, F32)
    box = VR.windows(vert, faces, view, intr, size, near)[0]
    out = []
    for s, b in zip(VR._setups(vert, faces, view, intr, size, near), box):
        x0, y0, bw, bh = win = VR.clamp_box(b, size)
        zb = VR.window_zbuffer(s, win)
        has = zb != VR.EMPTY
        o = depth_obs[y0:y0 + bh, x0:x0 + bw]
        with np.errstate(all="ignore"):
            ax = (np.arange(x0, x0 + bw).astype(F32) - cx) / fx
            ay = (np.arange(y0, y0 + bh).astype(F32) - cy) / fy
            c = np.sqrt((ax[None, :] * ax[None, :] + ay[:, None] * ay[:, None]) + F32(1))
            D, Do = VR.key_depth(zb) * c, o * c
            own = has & (~(o > 0) | (D - Do <= F32(delta)))
        out.append(SimpleNamespace(win=win, has=has, own=own, D=D.astype(F32)))
    return box, out


def intersection(win_a, win_b):
    """(x0, y0, w, h) of the rectangle two windows share; w = h = 0 when they do not meet (an empty window meets nothing)"""
    ax, ay, aw, ah = win_a
    bx, by, bw, bh = win_b
    x0, y0 = max(ax, bx), max(ay, by)
    w, h = min(ax + aw, bx + bw) - x0, min(ay + ah, by + bh) - y0
    return (x0, y0, w, h) if aw > 0 and bw > 0 and w > 0 and h > 0 else (x0, y0, 0, 0)


def _cut(img, win, X):
    x0, y0, w, h = X
    return img[y0 - win[1]:y0 - win[1] + h, x0 - win[0]:x0 - win[0] + w]


def pair_vsd(vert, faces, view_a, view_b, intr, size, near, depth_obs, delta, taus, inv_norm=1.0):
    """sam6d_pose_pair_vsd with the windows sam6d_hip.posematch.pair_vsd gives it
    -> counts (A, B, 4+T) int32, view_counts (A+B, 2) int32, box (A+B, 4) int32, X (A, B, 4) int32 the shared rectangles"""
    view_a, view_b = np.asarray(view_a, F32).reshape(-1, 3, 4), np.asarray(view_b, F32).reshape(-1, 3, 4)
    A, B, T = len(view_a), len(view_b), len(taus)
    box, img = view_images(vert, faces, np.concatenate([view_a, view_b]), intr, size, near, depth_obs, delta)
    counts, view_counts = np.zeros((A, B, 4 + T), np.int32), np.zeros((A + B, 2), np.int32)
    X = np.zeros((A, B, 4), np.int32)
    for i in range(A):
        for j in range(B):
            X[i, j] = intersection(img[i].win, img[A + j].win)
    if VR.areas(box, size).sum() == 0:  # total == 0: no pass runs
        return counts, view_counts, box, X
    for n, v in enumerate(img):
        view_counts[n] = [v.has.sum(), v.own.sum()]
    for i in range(A):
        e = img[i]
        for j in range(B):
            g = img[A + j]
            E, G = int(view_counts[i, 1]), int(view_counts[A + j, 1])
            n_inter = n_extra = 0
            cost = [0] * T
            if X[i, j, 2] > 0:
                has_e, own_e, D_e = (_cut(a, e.win, X[i, j]) for a in (e.has, e.own, e.D))
                own_g, D_g = (_cut(a, g.win, X[i, j]) for a in (g.own, g.D))
                inter = has_e & own_g
                with np.errstate(all="ignore"):
                    err = np.abs(D_g - D_e) * F32(inv_norm)
                    cost = [int((inter & (err >= F32(t))).sum()) for t in taus]
                n_inter, n_extra = int(inter.sum()), int((inter & ~own_e).sum())
            visib_est = E + n_extra
            counts[i, j] = [visib_est + G - n_inter, n_inter, visib_est, G] + cost
    return counts, view_counts, box, X


def expand(view_a, view_b):
    """the A B pairs of the matrix, row-major, as the (2 A B, 3, 4) views poseerr_ref.vsd_counts and poseerr.vsd take"""
    view_a, view_b = np.asarray(view_a, F32).reshape(-1, 3, 4), np.asarray(view_b, F32).reshape(-1, 3, 4)
    A, B = len(view_a), len(view_b)
    return np.concatenate([np.repeat(view_a, B, axis=0), np.tile(view_b, (A, 1, 1))])


def vsd_of(counts):
    """what sam6d_hip.posematch.pair_vsd returns as `vsd`: (cost_k + n_union - n_inter) / n_union in float32, 1 where n_union is 0"""
    c = np.asarray(counts)
    num = (c[..., 4:] + (c[..., 0:1] - c[..., 1:2])).astype(F32)
    with np.errstate(all="ignore"):
        return np.where(c[..., 0:1] > 0, num / c[..., 0:1].astype(F32), F32(1)).astype(F32)


# ---------------------------------------------------------------------------------------------- scenes for the tests
# Scene builders and, cached once for the host and the device tests, what the restatement gives for them (want).  Everything is
# seeded; the cached arrays are shared and must not be written to.
INSIDE, BORDER, THROUGH, OFF, BEHIND = range(5)  # VR.five_poses


def render(view, mesh=None, intr=VR.INTR, size=VR.SIZE):
    """the nearest rendered depth of the views, 0 where nothing is"""
    v, f = mesh or RR.icosphere(2)
    box = VR.windows(v, f, view, intr, size)[0]
    return VR.pose_verify(v, f, view, intr, size, NEAR, box, np.zeros(size, F32), None, 0.0)[2]


def _scene(mesh, a, b, obs, intr=VR.INTR, delta=DELTA, taus=(0.05,), diameter=None):
    return SimpleNamespace(mesh=mesh, a=np.asarray(a, F32), b=np.asarray(b, F32), obs=np.asarray(obs, F32), intr=intr, size=obs.shape,
                           delta=delta, taus=list(taus), diameter=diameter, inv_norm=1.0 if diameter is None else F32(1.0 / diameter))


def want(s):
    """the restatement on a scene -> counts, view_counts, box, X"""
    return pair_vsd(s.mesh[0], s.mesh[1], s.a, s.b, s.intr, s.size, NEAR, s.obs, s.delta, s.taus, s.inv_norm)


def occluded(obs):
    """test_vsd_mixed_pairs' depth image from a render: a plane in front of the left part, a strip without readings, a negative value
    and a NaN"""
    obs = obs.copy()
    obs[:, :30] = np.where(obs[:, :30] > 0, F32(2.5), obs[:, :30])
    obs[40:, :] = 0
    obs[20, 33], obs[21, 34] = -1.0, np.nan
    return obs


@functools.lru_cache(maxsize=None)
def mixed(T=4):
    """9 x 8 poses of the icosphere at VR.SIZE: five_poses on both sides (empty windows, a pose through the camera plane), an estimate a
    little behind a ground truth (it is seen only through the ground truth's visibility), and random poses"""
    g = np.random.default_rng(22)
    five = list(VR.five_poses())

    def rand():
        return VR.pose((g.uniform(-1.2, 1.2), g.uniform(-0.8, 0.8), g.uniform(3.5, 5.0)), axis=g.normal(size=3), angle=g.uniform(0.0, 3.0))

    b = np.stack(five + [rand() for _ in range(3)])
    a = np.stack(five + [VR.pose(b[5][:, 3].astype(np.float64) + (0.05, 0.0, 0.15))] + [rand() for _ in range(3)])
    return _scene(RR.icosphere(2), a, b, occluded(render(b)), taus=[0.02 * (k + 1) for k in range(T)], diameter=2.0)


@functools.lru_cache(maxsize=None)
def mixed_want(T=4):
    return want(mixed(T))


@functools.lru_cache(maxsize=None)
def crowd_poses(n):
    """pose_crowd_ref's scene as test_vsd_crowd_of_tiny_windows draws it: mesh a at 45 x 61, windows of a few words, some empty, n
    ground truths and an estimate near each, the ground truths' render with random holes as the depth image"""
    g = np.random.default_rng(3)
    mesh = RF.mesh_a()
    size, intr = (45, 61), (60.0, 60.0, 30.0, 22.0)
    fx, fy, cx, cy = intr
    gt, est = [], []
    for _ in range(n):
        z, px, py = g.uniform(15.0, 60.0), g.uniform(-8.0, size[1] + 8.0), g.uniform(-8.0, size[0] + 8.0)
        axis, angle = g.normal(size=3), g.uniform(0.0, 3.0)
        t = np.array([(px - cx) / fx * z, (py - cy) / fy * z, z])
        gt.append(VR.pose(t, axis=axis, angle=angle))
        est.append(VR.pose(t + g.normal(size=3) * [0.3, 0.3, 1.0], axis=axis, angle=angle + 0.2))
    gt, est = np.stack(gt), np.stack(est)
    depth = render(gt, mesh, intr, size)
    obs = np.where(depth > 0, depth, np.where(g.random(size) < 0.5, F32(60.0), F32(0))).astype(F32)
    obs[g.random(size) < 0.05] = 0
    return mesh, est, gt, obs, intr


def crowd(A, B, n=64):
    """estimates 0 .. A-1 against ground truths 0 .. B-1 of crowd_poses(n)"""
    mesh, est, gt, obs, intr = crowd_poses(n)
    return _scene(mesh, est[:A], gt[:B], obs, intr=intr, delta=0.5, taus=[0.25, 1.0, 4.0])


@functools.lru_cache(maxsize=None)
def crowd_want(A, B, n=64):
    return want(crowd(A, B, n))


def _shifted(base, axis, px, step, count):
    """`base` moved along camera x or y in steps of `step` pixels at its depth -> (count,3,4)"""
    out = np.repeat(base[None], count, axis=0).copy()
    out[:, axis, 3] += (np.arange(count) * step * base[2, 3] / px).astype(F32)
    return out


def shift_to(mesh, base, axis, offset, intr=VR.INTR, size=VR.SIZE):
    """`base` moved along camera x (axis 0) or y (axis 1) until its window starts `offset` pixels after base's: the window's first
    pixel is a staircase of the translation, walked here in half-pixel steps"""
    cand = _shifted(base, axis, intr[axis], 0.5, 2 * offset + 8)
    box = VR.windows(mesh[0], mesh[1], cand, intr, size)[0]
    hit = np.nonzero(box[:, axis] == box[0, axis] + offset)[0]
    assert len(hit), (axis, offset, box[:, axis])
    return cand[hit[0]]


@functools.lru_cache(maxsize=None)
def window_edges():
    """the sphere at VR.SIZE.  a = a sphere 6 units away at the image centre, and one 5 units away that the border does not cut;
    b = the first a moved along x until the windows share exactly one pixel column, and until they abut without sharing; the same two
    along y; a sphere 12 units away nested inside a[0]'s window; five_poses' sphere that the border cuts"""
    mesh = RR.icosphere(2)
    base = VR.pose((-0.9, -0.8, 6.0))
    x0, y0, x1, y1 = VR.windows(mesh[0], mesh[1], base[None], VR.INTR, VR.SIZE)[0][0]
    a = np.stack([base, VR.pose((0.9, 0.5, 5.0))])
    b = np.stack([shift_to(mesh, base, 0, x1 - x0), shift_to(mesh, base, 0, x1 - x0 + 1), shift_to(mesh, base, 1, y1 - y0),
                  shift_to(mesh, base, 1, y1 - y0 + 1), VR.pose((-1.8, -1.6, 12.0)), VR.five_poses()[BORDER]])
    obs = render(b)
    obs[:, 40:44] = np.where(obs[:, 40:44] > 0, F32(2.0), obs[:, 40:44])
    obs[20:22, :] = 0
    return _scene(mesh, a, b, obs, taus=[0.0, 0.05], diameter=2.0)


FLAT = (np.array([[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32))
WALK_SIZE, WALK_INTR = (150, 300), (100.0, 100.0, 150.0, 75.0)
WALK_AREAS = ((1, 1), (1, 65), (63, 1), (64, 1), (65, 1))  # (w, h) of the rectangle a[0] shares with b[k]


@functools.lru_cache(maxsize=None)
def pair_walk():
    """a square seen face on (R = I) and 70 pixels wide.  a[0] is placed so that its window is the 70 x 70 rendered pixels and no more
    (the first of eight quarter-pixel steps along the diagonal for which that holds), and b[k] is a[0] moved so that the two windows
    share WALK_AREAS[k]: 1 x 1, a column of 65, and rows of 63, 64 and 65 pixels, on both sides of a wave's 64 lanes; a[1] = b[5] is
    the square near the camera, whose window is wider than a workgroup's 256 pixels and takes many steps of the walk"""
    z = 200.0 / 70.0
    at = [-0.9 + k * 0.25 * z / 100.0 for k in range(8)]
    cand = np.stack([np.concatenate([np.eye(3), [[t], [t], [z]]], axis=1).astype(F32) for t in at])
    box = VR.windows(FLAT[0], FLAT[1], cand, WALK_INTR, WALK_SIZE)[0]
    ww = wh = 70
    full = np.nonzero((box[:, 2] - box[:, 0] + 1 == ww) & (box[:, 3] - box[:, 1] + 1 == wh))[0]
    assert len(full), box
    base = cand[full[0]]
    wide = np.concatenate([np.eye(3), [[0.0], [0.0], [0.72]]], axis=1).astype(F32)
    b = [shift_to(FLAT, shift_to(FLAT, base, 0, ww - w, WALK_INTR, WALK_SIZE), 1, wh - h, WALK_INTR, WALK_SIZE) for w, h in WALK_AREAS]
    g = np.random.default_rng(5)
    obs = g.choice(np.array([0.0, z - 1.0, z, z + 1.0], F32), WALK_SIZE).astype(F32)
    return _scene(FLAT, np.stack([base, wide]), np.stack(b + [wide]), obs, intr=WALK_INTR, taus=[0.0, 0.05, 1.0])
