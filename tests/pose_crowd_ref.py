"""Scenes for the pose check and the refinement where their kernels have their real control flow: a thousand poses with windows of a
few words, so that one wave holds many poses and one workgroup many windows; seventy identical poses; quads seen face on, whose normal
equations are singular by construction; and one whole-image window at the 2048 x 2048 limit.  Scene builders only: every expected
value is what tests/verify_ref.py and tests/refine_ref.py compute for the scene, cached here once for the host and the device tests
(tests/test_pose_crowd_host.py asserts that the scenes are what they are built to be, tests/test_pose_crowd_gpu.py runs them).
Everything is seeded; the cached arrays are shared and must not be written to.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

from tests import raster_ref as RR
from tests import refine_ref as RF
from tests import verify_ref as VR

F32, F64 = np.float32, np.float64
TAU = 2.0 ** -6
NEAR = 1e-3
DAMPING = 1e-6
TINY_SIZE, TINY_INTR = (45, 61), (60.0, 60.0, 30.0, 22.0)  # the odd size: masks[n] starts at every alignment
MESHES = {"a": RF.mesh_a, "b": RF.mesh_b}
#          N, size, intrinsics, zmin, zmax, seed, mesh
CROWDS = {"tiny": (1024, TINY_SIZE, TINY_INTR, 15.0, 60.0, 1, "a"),   # windows of a few words: many poses to a wave
          "mid": (300, RF.BIG, RF.BIG_INTR, 20.0, 60.0, 1, "a"),
          "mixed": (64, RF.BIG, RF.BIG_INTR, 6.0, 20.0, 1, "b")}      # windows on both sides of a workgroup's 1024 words
CROWD_MIN_PAIRS, CROWD_MARGIN = 6, 1
MID_ITERS, MID_MARGIN = 3, 2
QUADS_GATE, QUADS_MIN_PAIRS, QUADS_MARGIN = 4.0, 40, 1
LIMIT = 2048
LIMIT_INTR = (0.9 * LIMIT, 0.9 * LIMIT, LIMIT / 2.0, LIMIT / 2.0)
LIMIT_MIN_PAIRS = 32


def _views(R, t):
    return np.concatenate([np.asarray(R, F32), np.asarray(t, F32)[:, :, None]], axis=2)


def _masks(g, N, size):
    """about 40 % of the bytes set, to any non-zero value"""
    return np.where(g.random((N,) + size) < 0.4, g.integers(1, 256, (N,) + size), 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------- 1. crowds
@functools.lru_cache(maxsize=None)
def crowd(N, size, intr, zmin, zmax, seed, mesh):
    """N poses of one mesh: z uniform in [zmin, zmax], the projected centre uniform over the image grown by 8 pixels on every side (some
    poses fall off-screen), a rotation about a normal axis by an angle uniform in [0, 3).  The observed depth is the composite render of
    these poses with a third of the covered pixels moved 3 tau away from the camera, a third towards it, a few zeroed, one negative and
    one NaN; the background is 0 or zmax.  -> v, f, view (N,3,4), size, intr, obs (H,W), masks (N,H,W) u8"""
    g = np.random.default_rng(seed)
    v, f = MESHES[mesh]()
    H, W = size
    fx, fy, cx, cy = intr
    view = []
    for _ in range(N):
        z, px, py = g.uniform(zmin, zmax), g.uniform(-8.0, W + 8.0), g.uniform(-8.0, H + 8.0)
        view.append(VR.pose(((px - cx) / fx * z, (py - cy) / fy * z, z), axis=g.normal(size=3), angle=g.uniform(0.0, 3.0)))
    view = np.stack(view)
    box = VR.windows(v, f, view, intr, size, NEAR)[0]
    depth = VR.pose_verify(v, f, view, intr, size, NEAR, box, np.zeros(size, F32), None, TAU)[2]
    moved = depth + g.choice(np.array([0.0, 3 * TAU, -3 * TAU], F32), size)
    obs = np.where(depth > 0, moved, np.where(g.random(size) < 0.5, F32(zmax), F32(0))).astype(F32)
    obs[g.random(size) < 0.03] = 0
    ys, xs = np.nonzero(depth > 0)
    obs[ys[0], xs[0]], obs[ys[-1], xs[-1]] = -1.0, np.nan
    return SimpleNamespace(v=v, f=f, view=view, size=size, intr=intr, obs=obs, masks=_masks(g, N, size))


def scene(name):
    return crowd(*CROWDS[name])


@functools.lru_cache(maxsize=None)
def verify_want(name, with_masks):
    """the restatement of verify.render_compare for a scene: box, counts (column 7 from the windows), ids, depth"""
    s = SCENES[name]()
    box, dropped = VR.windows(s.v, s.f, s.view, s.intr, s.size, NEAR)
    counts, ids, depth = VR.pose_verify(s.v, s.f, s.view, s.intr, s.size, NEAR, box, s.obs, s.masks if with_masks else None, TAU)
    if VR.areas(box, s.size).sum() > 0:
        assert np.array_equal(counts[:, 7], dropped)
    counts[:, 7] = dropped
    return box, counts, ids, depth


@functools.lru_cache(maxsize=None)
def crowd_starts(name, margin):
    """every pose of the crowd turned and shifted as RF.start("far") does, and the windows of these starts grown by `margin`
    -> R (N,3,3), t (N,3) float32, box (N,4) int32"""
    s = scene(name)
    Rs, ts = zip(*[RF.start("far", M) for M in s.view])
    R, t = np.stack(Rs), np.stack(ts)
    return R, t, RF.grow(VR.windows(s.v, s.f, _views(R, t), s.intr, s.size, NEAR)[0], margin, s.size)


def state_of(R, t):
    return np.concatenate([np.asarray(R, F32).reshape(len(R), 9), np.asarray(t, F32)], axis=1).astype(F64)


@functools.lru_cache(maxsize=None)
def crowd_step_want(name, max_step, with_masks):
    """one refinement step of the crowd's starts -> state (N,12) float64, acc (N,32) int64, stats (N,4) int32"""
    s = scene(name)
    R, t, box = crowd_starts(name, CROWD_MARGIN)
    return RF.step(s.v, s.f, state_of(R, t), 1.0, s.intr, s.size, NEAR, box, s.obs, s.masks if with_masks else None, RF.GATE,
                   RF.inv_unit_of(s.v), DAMPING, CROWD_MIN_PAIRS, max_step)


@functools.lru_cache(maxsize=None)
def mid_refine_want():
    """refine.refine_poses of the `mid` crowd's starts"""
    s = scene("mid")
    R, t, _ = crowd_starts("mid", MID_MARGIN)
    return RF.refine(s.v, s.f, R, t, s.intr, s.size, s.obs, iters=MID_ITERS, gate=RF.GATE, margin=MID_MARGIN, min_pairs=CROWD_MIN_PAIRS)


# ---------------------------------------------------------------------------------------------------------- 2. duplicates
@functools.lru_cache(maxsize=None)
def duplicates():
    """the inside pose of VR.five_poses seventy times, then one nearer pose that overlaps them: every window has the same size (less
    than a workgroup's words, so the windows start everywhere in a workgroup), and the seventy tie on depth at every pixel"""
    v, f = RR.icosphere(2)
    view = np.stack([VR.five_poses()[0]] * 70 + [VR.pose((0.6, 0.2, 3.2))])
    g = np.random.default_rng(4)
    return SimpleNamespace(v=v, f=f, view=view, size=VR.SIZE, intr=VR.INTR, obs=np.full(VR.SIZE, 3.5, F32), masks=_masks(g, 71, VR.SIZE))


# ---------------------------------------------------------------------------------------------------------- 3. frontal quads
@functools.lru_cache(maxsize=None)
def frontal_quads(seed=1):
    """A quad in the plane z = 0 at 130 poses with R = I exactly.  P = v + t, so both edge vectors of a face have z = +-0 and its
    normal is (+-0, +-0, -+1) exactly: J2 = c0 nrm1 - c1 nrm0 is exactly 0 for every pair, acc word (2,2) is 0 and so is every other
    word of row and column 2 of A, and the third pivot is 0 > 0: false, with or without damping.  A pose with min_pairs pairs is
    singular (status 2) by construction.  Pose 0 is (0, 0, 1.2) and covers the whole image; the observed depth is its render moved by
    0.1 in z, so with the gate of 4 every rendered pixel of every pose is a pair.  The other centres are uniform over the image grown by
    40 pixels: some poses are off-screen (status 4), some are clipped by the border to fewer than min_pairs pixels (status 1)."""
    g = np.random.default_rng(seed)
    v = np.array([[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]], F32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    N, (H, W), (fx, fy, cx, cy) = 130, TINY_SIZE, TINY_INTR
    z = g.uniform(1.2, 5.0, N)
    px, py = g.uniform(-40.0, W + 40.0, N), g.uniform(-40.0, H + 40.0, N)
    t = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], axis=1).astype(F32)
    t[0] = [0.0, 0.0, 1.2]
    R = np.stack([np.eye(3, dtype=F32)] * N)
    seen = np.concatenate([np.eye(3), [[0.0], [0.0], [1.2 + 0.1]]], axis=1).astype(F32)
    obs = VR.render_depth(v, f, seen, TINY_INTR, TINY_SIZE)[1]
    box = RF.grow(VR.windows(v, f, _views(R, t), TINY_INTR, TINY_SIZE, NEAR)[0], QUADS_MARGIN, TINY_SIZE)
    return SimpleNamespace(v=v, f=f, R=R, t=t, view=_views(R, t), size=TINY_SIZE, intr=TINY_INTR, obs=obs, masks=None, box=box)


@functools.lru_cache(maxsize=None)
def quads_step_want(damping):
    s = frontal_quads()
    return RF.step(s.v, s.f, state_of(s.R, s.t), 1.0, s.intr, s.size, NEAR, s.box, s.obs, None, QUADS_GATE, RF.inv_unit_of(s.v), damping,
                   QUADS_MIN_PAIRS, math.inf)


# ---------------------------------------------------------------------------------------------------------- 4. the size limit
QUAD = (np.array([[-3, -3, 2], [3, -3, 2], [-3, 3, 2], [3, 3, 2]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32))  # test_verify_gpu's quad


@functools.lru_cache(maxsize=None)
def limit():
    """two triangles that cover a 2048 x 2048 image: one window of 2^22 words, 4096 workgroups that meet at one pose's counters and
    sums.  The observed depth is the render itself in tiles of 64 x 64 pixels: as rendered, 2 tau farther, 2 tau nearer -- every pixel
    is a pair of the refinement"""
    v, f = QUAD
    view = VR.pose((0.0, 0.0, 1.0), angle=0.2)[None]
    size = (LIMIT, LIMIT)
    setup = RR.Setup(v, f, view[0], *LIMIT_INTR, NEAR, LIMIT, LIMIT)
    depth = VR.window_depth(VR.window_zbuffer(setup, (0, 0, LIMIT, LIMIT)))
    tile = np.add.outer(np.arange(LIMIT) // 64, np.arange(LIMIT) // 64) % 3
    obs = (depth + np.array([0.0, 2 * TAU, -2 * TAU], F32)[tile]).astype(F32)
    return SimpleNamespace(v=v, f=f, view=view, size=size, intr=LIMIT_INTR, obs=obs, masks=None,
                           box=np.array([[0, 0, LIMIT - 1, LIMIT - 1]], np.int32))


@functools.lru_cache(maxsize=None)
def limit_step_want():
    s = limit()
    return RF.step(s.v, s.f, state_of(s.view[:, :, :3], s.view[:, :, 3]), 1.0, s.intr, s.size, NEAR, s.box, s.obs, None, RF.GATE,
                   RF.inv_unit_of(s.v), DAMPING, LIMIT_MIN_PAIRS, math.inf)


SCENES = {"tiny": functools.partial(scene, "tiny"), "mid": functools.partial(scene, "mid"), "mixed": functools.partial(scene, "mixed"),
          "duplicates": duplicates, "limit": limit}
