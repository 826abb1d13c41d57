"""The pose refinement (sam6d_hip.refine, csrc/refine.hip): the host side and the numpy restatement of the recipe (tests/refine_ref.py).
No GPU: the restatement converges where a plain float64 Gauss-Newton does, its integer sums are the exact sums within their rounding
bound, a pose that cannot step keeps its bits, and the binding, the header and the refusals are in place."""
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import refine_ref as RF
from tests import verify_ref as VR
from tests._util import ROOT
from sam6d_hip import _lib, refine

F32, F64 = np.float32, np.float64
SCENES = {"48x64": (VR.SIZE, VR.INTR), "96x128": (RF.BIG, RF.BIG_INTR)}


@functools.lru_cache(maxsize=None)
def _observed(scene):
    size, intr = SCENES[scene]
    v, f = RF.mesh_a()
    return VR.render_depth(v, f, RF.TRUE, intr, size)[1]


def _errors(state):
    """(translation error, |R - R_true|_F) of one pose's float64 state against the true pose"""
    true = RF.TRUE.astype(F64)
    return float(np.linalg.norm(state[9:] - true[:, 3])), float(np.linalg.norm(state[:9].reshape(3, 3) - true[:, :3]))


def _plain(v, f, R, t, intr, size, depth, box, iters, gate, inv_unit, damping):
    """a plain float64 solver of the same normal equations: the same pairs, float64 sums without quantisation, np.linalg.solve, and the
    Cayley update in numpy's matrix arithmetic"""
    state = np.concatenate([R.reshape(9), t]).astype(F64)
    unit = 1.0 / float(inv_unit)
    for _ in range(iters):
        u = RF.pairs(v, f, RF.view_of(state, 1.0), intr, size, 1e-3, VR.clamp_box(box, size), depth, None, gate, inv_unit).astype(F64)
        J, e = u[:, :6], u[:, 6]
        A = J.T @ J
        x = np.linalg.solve(A + damping * np.diag(np.diag(A)), J.T @ e)
        w = x[:3] / 2
        X = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        C = np.eye(3) + 2 / (1 + w @ w) * (X + X @ X)
        state = np.concatenate([(C @ state[:9].reshape(3, 3)).reshape(9), state[9:] + x[3:] * unit])
    return state


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("name", sorted(RF.STARTS))
def test_converges_as_a_plain_float64_solver_does(scene, name):
    """8 iterations from both starts at both image sizes: within 1e-3 units of the true translation and 1e-3 in |R - R_true|_F, and no
    worse than twice the plain solver on the same pairs"""
    size, intr = SCENES[scene]
    v, f = RF.mesh_a()
    depth = _observed(scene)
    R, t = RF.start(name)
    got = RF.refine(v, f, R[None], t[None], intr, size, depth, iters=8, gate=RF.GATE)
    assert got["status"].tolist() == [0] and got["n_pairs"][0] > 100
    et, er = _errors(got["state"][0])
    pt, pr = _errors(_plain(v, f, R, t, intr, size, depth, got["boxes"][0], 8, RF.GATE, RF.inv_unit_of(v), 1e-6))
    e0 = _errors(np.concatenate([R.reshape(9), t]).astype(F64))
    print("\n[refine %s %s] start %.3g %.3g  restatement %.3g %.3g  plain %.3g %.3g  rms %s" % (scene, name, *e0, et, er, pt, pr, got["history"][0, :, 1]))
    assert et <= 1e-3 and er <= 1e-3
    assert et <= 2 * pt and er <= 2 * pr
    assert got["history"][0, -1, 1] < got["history"][0, 0, 1]


@pytest.mark.parametrize("mesh", ["a", "b"])
def test_integer_sums_are_the_exact_sums_within_their_rounding_bound(mesh):
    """every entry of acc * 2^-S is within pairs * 2^-(S+1) of the sum of the exact products (rational arithmetic: no rounding at all)"""
    v, f = RF.mesh_a() if mesh == "a" else RF.mesh_b()
    depth = VR.render_depth(v, f, RF.TRUE, VR.INTR, VR.SIZE)[1]
    R, t = RF.start("near")
    M = np.concatenate([R, t[:, None]], axis=1)
    box = VR.windows(v, f, M[None], VR.INTR, VR.SIZE)[0][0]
    u = RF.pairs(v, f, M, VR.INTR, VR.SIZE, 1e-3, VR.clamp_box(box, VR.SIZE), depth, None, RF.GATE, RF.inv_unit_of(v))
    acc = RF.sums(u)
    P = len(u)
    assert acc[28] == P > 100 and not acc[29:].any()
    assert np.abs(u[:, :6]).max() <= 16.0 * (1 + 2.0 ** -20) and np.abs(u[:, 6]).max() <= 16.0  # what the overflow argument rests on
    cols = [[Fraction(float(x)) for x in u[:, i]] for i in range(7)]
    for k, (i, j) in enumerate(RF.WORDS):
        exact = sum(a * b for a, b in zip(cols[i], cols[j]))
        assert abs(Fraction(int(acc[k]), 2 ** RF.S) - exact) <= Fraction(P, 2 ** (RF.S + 1)), (k, i, j)
    d = u.astype(F64)
    assert abs(float(acc[27]) * 2.0 ** -RF.S - math.fsum(d[:, 6] * d[:, 6])) <= P * 2.0 ** -(RF.S + 1)


def test_a_pose_that_cannot_step_keeps_its_bits():
    """no window, no depth, too few pairs, a refused step: the state is unchanged, bit for bit, and the status says why"""
    v, f = RF.mesh_a()
    depth = _observed("48x64")
    R, t = RF.start("near")
    off = VR.pose((10.0, 0.0, 4.0))
    Rs, ts = np.stack([R, off[:, :3], R, R]), np.stack([t, off[:, 3], t, t])
    state = np.concatenate([Rs.reshape(4, 9), ts], axis=1).astype(F64)
    box = VR.windows(v, f, np.concatenate([Rs, ts[:, :, None]], axis=2), VR.INTR, VR.SIZE)[0]
    assert box[1].tolist() == [0, 0, -1, -1]
    iu = RF.inv_unit_of(v)
    args = (v, f, state, 1.0, VR.INTR, VR.SIZE, 1e-3, box)
    new, acc, stats = RF.step(*args, depth, None, RF.GATE, iu, 1e-6, 32, math.inf)
    assert stats[:, 1].tolist() == [0, 4, 0, 0] and stats[1, 0] == 0 and not acc[1].any()
    assert np.array_equal(new[1].view(np.uint64), state[1].view(np.uint64)) and not np.array_equal(new[0], state[0])
    assert np.array_equal(new[0], new[2])  # a pose's step does not depend on its neighbours
    new, acc, stats = RF.step(*args, np.zeros_like(depth), None, RF.GATE, iu, 1e-6, 32, math.inf)  # no depth anywhere
    assert stats[:, 1].tolist() == [1, 4, 1, 1] and not stats[:, 0].any() and np.array_equal(new.view(np.uint64), state.view(np.uint64))
    new, acc, stats = RF.step(*args, depth, None, RF.GATE, iu, 1e-6, 100000, math.inf)  # more pairs asked for than pixels
    assert stats[:, 1].tolist() == [1, 4, 1, 1] and stats[0, 0] > 100 and np.array_equal(new.view(np.uint64), state.view(np.uint64))
    new, acc, stats = RF.step(*args, depth, None, RF.GATE, iu, 1e-6, 32, 1e-9)  # no step is this small
    assert stats[:, 1].tolist() == [3, 4, 3, 3] and np.array_equal(new.view(np.uint64), state.view(np.uint64))
    masks = np.zeros((4,) + VR.SIZE, np.uint8)
    masks[2] = 1
    new, acc, stats = RF.step(*args, depth, masks, RF.GATE, iu, 1e-6, 32, math.inf)  # an empty mask: no pairs
    assert stats[:, 1].tolist() == [1, 4, 0, 1] and np.array_equal(new[0].view(np.uint64), state[0].view(np.uint64))
    # sum e e travels as two 32-bit halves
    assert (int(stats[2, 3]) << 32 | int(np.uint32(stats[2, 2]))) == int(acc[2, 27]) > 0


def test_grown_windows():
    box = np.array([[5, 6, 20, 30], [0, 0, -1, -1], [0, 2, 63, 47], [3, 3, 2, 9]], np.int32)
    assert RF.grow(box, 0, VR.SIZE).tolist() == [[5, 6, 20, 30], [0, 0, -1, -1], [0, 2, 63, 47], [0, 0, -1, -1]]
    assert RF.grow(box, 8, VR.SIZE).tolist() == [[0, 0, 28, 38], [0, 0, -1, -1], [0, 0, 63, 47], [0, 0, -1, -1]]
    got = refine.grow_boxes(torch.from_numpy(box), 8, *VR.SIZE)
    assert got.dtype == torch.int32 and got.tolist() == RF.grow(box, 8, VR.SIZE).tolist()
    assert refine.grow_boxes(torch.from_numpy(box), 0, *VR.SIZE).tolist() == RF.grow(box, 0, VR.SIZE).tolist()
    v, _ = RF.mesh_b()
    assert float(refine.mesh_radius2(torch.from_numpy(v))) == float(RF.radius2(v))
    assert refine.inv_unit(RF.radius2(v), 0.001) == float(RF.inv_unit_of(v, 0.001))
    stats = np.array([[4, 0, -5, 3], [0, 1, 0, 0]], np.int32)
    iu = F32(0.37)
    want = RF.rms_of(stats, iu)
    assert want[1] == 0 and want[0] == F32(math.sqrt((3 * 2.0 ** 32 + 2.0 ** 32 - 5) * 2.0 ** -30 / 4) * (1.0 / float(iu)))
    assert np.array_equal(refine.rms_of(torch.from_numpy(stats), 1.0 / float(iu)).numpy(), want)


def test_binding_header_and_workspace():
    names = ("sam6d_pose_refine_workspace_bytes", "sam6d_pose_refine_step")
    hdr = open(os.path.join(ROOT, "include", "sam6d_hip.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES and hdr.count(name + "(") >= 1, name
    assert len(_lib.SIGNATURES["sam6d_pose_refine_step"]) == 30 and "#define SAM6D_ABI_VERSION 6" in hdr
    assert _lib.SIGNATURES["sam6d_pose_refine_step"].count(ctypes.c_double) == 2
    lib = _lib.load()
    assert lib.sam6d_pose_refine_workspace_bytes(0, 1) == 80 and lib.sam6d_pose_refine_workspace_bytes(1000, 5) == 8 * 1000 + 80 * 5
    assert lib.sam6d_pose_refine_workspace_bytes(1024 * 2048 * 2048, 1024) == 8 * 1024 * 2048 * 2048 + 80 * 1024
    assert lib.sam6d_pose_refine_workspace_bytes(-1, 5) == 0 and lib.sam6d_pose_refine_workspace_bytes(5, 0) == 0
    assert lib.sam6d_pose_refine_workspace_bytes(5, 1025) == 0 and lib.sam6d_pose_refine_workspace_bytes(2048 * 2048 + 1, 1) == 0
    src = open(os.path.join(ROOT, "openvino-sam-6d_amd", "csrc", "refine.hip")).read()
    assert "verify_raster.h" in src and "verify_faces_kernel," in src and "__global__ __launch_bounds__(64) void verify_faces_kernel" not in src
    ver = open(os.path.join(ROOT, "openvino-sam-6d_amd", "csrc", "verify.hip")).read()
    assert "verify_raster.h" in ver and "void verify_faces_kernel" not in ver  # one copy of the raster pass, in the header


def test_refine_poses_refusals():
    v, f = RF.mesh_a()
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    K = np.array([[60.0, 0, 32], [0, 60, 24], [0, 0, 1]])
    depth = torch.ones(48, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        refine.refine_poses((v, f), R, t, K, depth)
    with pytest.raises(RuntimeError, match="HIP device"):
        refine.refine_poses(dict(vertices=v.numpy(), faces=f.numpy()), R, t, K, depth)
    for kw, name in ((dict(R=R[:, :2]), "R"), (dict(t=t[:1]), "t"), (dict(depth=depth.double()), "depth"), (dict(depth=depth[None]), "depth"),
                     (dict(masks=torch.zeros(2, 48, 63, dtype=torch.uint8)), "masks"), (dict(masks=torch.zeros(2, 48, 64)), "masks"),
                     (dict(K=np.eye(4)), "K"), (dict(mesh=(v.double(), f)), "vertices"), (dict(mesh=(v, f.long())), "faces"), (dict(mesh=v), "mesh"),
                     (dict(near=0.0), "near"), (dict(depth=torch.ones(48, 2049)), "2048"),
                     (dict(R=torch.eye(3).repeat(1025, 1, 1), t=torch.zeros(1025, 3)), "N = 1025"),
                     (dict(iters=0), "iters"), (dict(iters=2.5), "iters"), (dict(gate=-1.0), "gate"), (dict(gate=float("nan")), "gate"),
                     (dict(gate=float("inf")), "gate"), (dict(margin=-1), "margin"), (dict(damping=-1e-3), "damping"), (dict(min_pairs=0), "min_pairs"),
                     (dict(max_step=0.0), "max_step"), (dict(max_step=float("nan")), "max_step"), (dict(scale=0.0), "scale")):
        args = dict(mesh=(v, f), R=R, t=t, K=K, depth=depth)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            refine.refine_poses(**args)


def test_kernel_resources():
    """no kernel of refine.hip uses scratch or spills, and each keeps within its built VGPR count rounded up
    to the next step of 8 (built: refine_view 8, refine_accumulate 78, refine_solve 70, and its copy of verify_faces 63, the figure of
    verify.hip's).  Read from the code object's metadata: the compiler's figures, not a GPU's."""
    from tests._util import kernel_resources
    limits = dict(refine_view_kernel=8, refine_accumulate_kernel=80, refine_solve_kernel=72, verify_faces_kernel=64)
    found = kernel_resources(b"refine_accumulate_kernel")
    print("\n[refine] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
