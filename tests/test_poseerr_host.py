"""The pose errors (sam6d_hip.poseerr, csrc/poseerr.hip): the host side and the numpy restatement of the recipe (tests/poseerr_ref.py).
No GPU: the binding, the restatement against an independent float64 evaluation of the textbook formulas within the bounds derived in
poseerr_ref.py, the symmetry transforms, the plain torch ops, the refusals, and the kernels' resources from the code object's metadata.
Nothing here is checked against bop_toolkit, which the suite does not have."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import poseerr_ref as PR
from tests import raster_ref as RR
from tests import verify_ref as VR
from tests._util import ROOT
from sam6d_hip import _lib, poseerr

F32, F64 = np.float32, np.float64
NAMES = ("sam6d_pose_point_errors", "sam6d_pose_point_errors_workspace_bytes", "sam6d_pose_vsd", "sam6d_pose_vsd_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ the binding
def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam6d_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared" % name
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert len(_lib.SIGNATURES["sam6d_pose_point_errors"]) == 21 and len(_lib.SIGNATURES["sam6d_pose_vsd"]) == 26
    lib = _lib.load()
    assert lib.sam6d_pose_point_errors_workspace_bytes(3, 5) == 8 * 3 * 5
    assert lib.sam6d_pose_point_errors_workspace_bytes(1024, 1024) == 8 << 20
    assert [lib.sam6d_pose_point_errors_workspace_bytes(*a) for a in ((0, 1), (1025, 1), (1, 0), (1, 1025))] == [0, 0, 0, 0]
    assert lib.sam6d_pose_vsd_workspace_bytes(0, 1) == 64 and lib.sam6d_pose_vsd_workspace_bytes(1000, 7) == 8 * 1000 + 64 * 7
    assert [lib.sam6d_pose_vsd_workspace_bytes(*a) for a in ((-1, 1), (0, 0), (0, 513), (2 * 2048 * 2048 + 1, 1))] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ against float64
def _scene(seed, N=5, V=40, spread=0.2):
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    gt = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(N)])
    est = np.stack([VR.pose(M[:, 3].astype(F64) + g.normal(size=3) * spread, axis=g.normal(size=3), angle=g.uniform(0, 3)) for M in gt])
    syms = poseerr.symmetry_transforms(discrete=[np.concatenate([VR.rotation((0, 0, 1), math.pi), [[0.1], [0.0], [0.0]]], axis=1)],
                                       continuous=[dict(axis=(0, 1, 0), offset=(0.05, 0, 0.02))], max_step=math.pi / 3)
    assert syms.shape == (6, 3, 4)
    return pts, est, gt, syms


def _textbook(pts, est, gt, syms, intr):
    """float64 from the definitions: 4 x 4 matrix products, norms, the pinhole projection"""
    def h(M):
        return np.concatenate([np.asarray(M, F64), np.broadcast_to([0.0, 0.0, 0.0, 1.0], M.shape[:-2] + (1, 4))], axis=-2)
    X = np.concatenate([pts.astype(F64), np.ones((len(pts), 1))], axis=1).T                   # (4,V)
    e = (h(est) @ X)[:, None, :3]                                                             # (N,1,3,V)
    g = (h(gt)[:, None] @ h(syms)[None] @ X)[:, :, :3]                                        # (N,S,3,V)
    dist = np.linalg.norm(e - g, axis=2)
    fx, fy, cx, cy = intr
    pe = np.stack([fx * e[:, :, 0] / e[:, :, 2] + cx, fy * e[:, :, 1] / e[:, :, 2] + cy], axis=2)
    pg = np.stack([fx * g[:, :, 0] / g[:, :, 2] + cx, fy * g[:, :, 1] / g[:, :, 2] + cy], axis=2)
    pix = np.linalg.norm(pe - pg, axis=2)
    return dist.max(axis=2).min(axis=1), pix.max(axis=2).min(axis=1), dist[:, 0].mean(axis=1), e, g


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_against_float64(seed):
    pts, est, gt, syms = _scene(seed)
    intr = (600.0, 590.0, 320.0, 240.0)
    inv_unit = F32(1.0 / 2.0)
    got = PR.point_errors(pts, est, gt, syms, intr, inv_unit)
    mssd, mspd, add, e, g = _textbook(pts, est, gt, syms, intr)
    # the operand magnitudes: B over every row of every transform, the nearest depth, the largest |x / z|, |y / z|
    G = PR.sym_gt(gt, syms).astype(F64).reshape(-1, 3, 4)
    rows = np.concatenate([est.astype(F64), G])
    B = float((np.abs(rows[:, :, :3]) @ np.abs(pts.astype(F64)).T + np.abs(rows[:, :, 3:])).max())
    both = np.concatenate([np.broadcast_to(e, g.shape), g], axis=1)
    zmin = float(both[:, :, 2].min())
    Q = float(np.abs(both[:, :, :2] / both[:, :, 2:3]).max())
    assert zmin > 1.0 and not got["n_skipped"].any()
    print("\n[poseerr] B %.3g zmin %.3g Q %.3g: mssd err %.3g (bound %.3g), mspd err %.3g (bound %.3g)"
          % (B, zmin, Q, np.abs(got["mssd"] - mssd).max(), PR.mssd_bound(B), np.abs(got["mspd"] - mspd).max(),
             PR.mspd_bound(B, zmin, Q, 600.0, 320.0)))
    assert np.abs(got["mssd"].astype(F64) - mssd).max() <= PR.mssd_bound(B)
    assert np.abs(got["mspd"].astype(F64) - mspd).max() <= PR.mspd_bound(B, zmin, Q, 600.0, 320.0)
    got_add = PR.add_of(got["add_sum"], inv_unit, len(pts)).astype(F64)
    assert np.abs(got_add - add).max() <= PR.add_bound(B, float(inv_unit), float(add.max()))
    assert mssd.min() > 1e3 * PR.mssd_bound(B) and mspd.min() > 1e3 * PR.mspd_bound(B, zmin, Q, 600.0, 320.0)  # the bounds bind


def test_restatement_rules():
    """the lowest index wins a tie, a skipped point leaves the p2 maximum and enters n_skipped, the ADD terms saturate, and a NaN
    is above every number"""
    pts = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -2.0]], F32)
    eye = np.concatenate([np.eye(3), [[0.0], [0.0], [1.0]]], axis=1).astype(F32)[None]   # the second point lies at z = -1
    moved = eye.copy()
    moved[0, 0, 3] = 0.5
    syms = np.stack([poseerr.symmetry_transforms()[0]] * 2)
    r = PR.point_errors(pts, moved, eye, syms, (100.0, 100.0, 0.0, 0.0), 1.0)
    assert r["n_skipped"].tolist() == [1] and r["mssd"].tolist() == [0.5] and r["mspd"].tolist() == [50.0]
    assert r["mssd_sym"].tolist() == [0] and r["mspd_sym"].tolist() == [0] and r["add_sum"].tolist() == [2 ** 30]
    far = moved.copy()
    far[0, 0, 3] = 1e9
    assert PR.point_errors(pts, far, eye, syms, (100.0, 100.0, 0.0, 0.0), 1.0)["add_sum"].tolist() == [2 * 2 ** 42]
    assert PR.bits(np.array([np.nan, -np.nan, np.inf, 0.0, 1.0], F32)).tolist() == [0x7FC00000, 0x7FC00000, 0x7F800000, 0, 0x3F800000]


# ------------------------------------------------------------------------------------------------------------ symmetries
def _rigid(T):
    R = T[:, :, :3].astype(F64)
    return np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(), np.abs(np.linalg.det(R) - 1.0).max()


def test_symmetry_transforms():
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F32)
    none = poseerr.symmetry_transforms()
    assert none.dtype == F32 and none.shape == (1, 3, 4) and np.array_equal(none[0], ident)
    flip = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]  # models_info's layout: sixteen numbers, row-major 4 x 4
    one = poseerr.symmetry_transforms(discrete=[flip])
    assert one.shape == (2, 3, 4) and np.array_equal(one[0], ident) and np.array_equal(one[1], np.reshape(flip, (4, 4))[:3].astype(F32))
    cont = [dict(axis=[0, 0, 1], offset=[0.5, -0.25, 3.0])]
    steps = math.ceil(math.pi / 0.01)
    assert steps == 315
    ring = poseerr.symmetry_transforms(continuous=cont)
    assert ring.shape == (steps, 3, 4) and np.array_equal(ring[0], ident)
    both = poseerr.symmetry_transforms(discrete=[flip], continuous=cont)
    assert both.shape == (2 * steps, 3, 4) and np.array_equal(both[:steps], ring)
    for T in (one, ring, both):
        orth, det = _rigid(T)
        assert orth <= 4 * 2.0 ** -24 and det <= 8 * 2.0 ** -24  # float64 construction, rounded once to float32
    # a point on the axis through the offset stays where it is; the steps are equal and compose inside the set
    on_axis = np.array([0.5, -0.25, -7.0])
    assert np.abs(ring[:, :, :3].astype(F64) @ on_axis + ring[:, :, 3] - on_axis).max() <= 8 * 2.0 ** -24 * 7.0
    coarse = poseerr.symmetry_transforms(continuous=[dict(axis=[1, 2, 2], offset=[0.1, 0.2, 0.3])], max_step=math.pi / 12)
    assert coarse.shape == (12, 3, 4)

    def h(T):
        return np.concatenate([T.astype(F64), [[0, 0, 0, 1]]], axis=0)
    for i in range(12):
        for j in range(12):
            assert np.abs((h(coarse[i]) @ h(coarse[j]))[:3] - coarse[(i + j) % 12]).max() <= 16 * 2.0 ** -24, (i, j)
    # C o D: the discrete transform first
    D, C = h(both[steps]), h(ring[7])
    assert np.abs((C @ D)[:3] - both[steps + 7]).max() <= 16 * 2.0 ** -24 * 3.0


def test_symmetry_transforms_refusals():
    cont = [dict(axis=[0, 0, 1], offset=[0, 0, 0])]
    assert poseerr.symmetry_transforms(continuous=cont, max_step=math.pi / 1024).shape[0] == 1024
    with pytest.raises(ValueError, match="1024"):
        poseerr.symmetry_transforms(continuous=cont, max_step=math.pi / 1025)
    with pytest.raises(ValueError, match="1024"):
        poseerr.symmetry_transforms(discrete=[np.eye(4)] * 3, continuous=cont)  # 4 x 315
    with pytest.raises(ValueError, match="discrete"):
        poseerr.symmetry_transforms(discrete=[np.eye(3)])
    with pytest.raises(ValueError, match="continuous"):
        poseerr.symmetry_transforms(continuous=[dict(axis=[0, 0, 1])])
    with pytest.raises(ValueError, match="axis"):
        poseerr.symmetry_transforms(continuous=[dict(axis=[0, 0, 0], offset=[0, 0, 0])])
    with pytest.raises(ValueError, match="max_step"):
        poseerr.symmetry_transforms(continuous=cont, max_step=0.0)


# ------------------------------------------------------------------------------------------------------------ plain torch ops
def test_recall_union_boxes_and_vsd_from_counts():
    err = torch.tensor([0.1, 0.2, 0.3, 0.4])
    assert poseerr.recall(err, [0.05, 0.2, 0.25, 1.0]).tolist() == [0.0, 0.25, 0.5, 1.0]  # strictly below
    with pytest.raises(ValueError, match="err"):
        poseerr.recall(torch.zeros(2, 2), [0.1])
    a = torch.tensor([[3, 4, 10, 12], [0, 0, -1, -1], [5, 5, 6, 6], [0, 0, -1, -1], [7, 2, 6, 9]], dtype=torch.int32)
    b = torch.tensor([[1, 6, 8, 20], [2, 3, 4, 5], [0, 0, -1, -1], [0, 0, -1, -1], [1, 1, 2, 2]], dtype=torch.int32)
    got = poseerr.union_boxes(a, b)
    assert got.dtype == torch.int32 and got.tolist() == [PR.union_box(x, y) for x, y in zip(a.tolist(), b.tolist())]
    assert got.tolist() == [[1, 4, 10, 20], [2, 3, 4, 5], [5, 5, 6, 6], [0, 0, -1, -1], [1, 1, 2, 2]]
    counts = np.array([[10, 4, 7, 7, 4, 1, 0], [0, 0, 0, 0, 0, 0, 0], [5, 5, 5, 5, 0, 0, 0]], np.int32)
    want = PR.vsd_of(counts)
    assert want.tolist() == [[1.0, F32(7) / F32(10), F32(6) / F32(10)], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]
    got = poseerr.vsd_from_counts(torch.from_numpy(counts))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    v, f = RR.octahedron()
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    K = np.array([[60.0, 0, 32], [0, 60, 24], [0, 0, 1]])
    depth = torch.ones(48, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.pose_errors(v, R, t, R, t, K)
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.pose_errors(dict(vertices=v.numpy(), faces=f.numpy()), R, t, R, t, K)
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.pose_errors(v, R, t, R, t, K, syms=poseerr.symmetry_transforms())
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.vsd((v, f), R, t, R, t, K, depth, 0.015, [0.05])
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.vsd(dict(vertices=v.numpy(), faces=f.numpy()), R, t, R, t, K, depth, 0.015, [0.05])
    base = dict(mesh_or_points=v, R_est=R, t_est=t, R_gt=R, t_gt=t, K=K)
    for kw, name in ((dict(R_est=R[:, :2]), "R_est"), (dict(R_est=R.double()), "R_est"), (dict(t_est=t[:1]), "t_est"), (dict(R_gt=R[:1]), "R_gt"),
                     (dict(t_gt=t.double()), "t_gt"), (dict(t_gt=t[:, :2]), "t_gt"), (dict(mesh_or_points=v.double()), "points"),
                     (dict(mesh_or_points=v[:, :2]), "points"), (dict(mesh_or_points=torch.zeros(0, 3)), "V = 0"), (dict(K=np.eye(4)), "K"),
                     (dict(syms=torch.zeros(2, 4, 4)), "syms"), (dict(syms=np.zeros((2, 3, 4))), "syms"),
                     (dict(syms=torch.zeros(1025, 3, 4)), "S = 1025"), (dict(unit=0.0), "unit"), (dict(unit=float("nan")), "unit"),
                     (dict(R_est=torch.eye(3).repeat(1025, 1, 1), t_est=torch.zeros(1025, 3), R_gt=torch.eye(3).repeat(1025, 1, 1),
                           t_gt=torch.zeros(1025, 3)), "N = 1025")):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            poseerr.pose_errors(**args)
    base = dict(mesh=(v, f), R_est=R, t_est=t, R_gt=R, t_gt=t, K=K, depth=depth, delta=0.015, taus=[0.05, 0.1])
    many = dict(R_est=torch.eye(3).repeat(513, 1, 1), t_est=torch.zeros(513, 3), R_gt=torch.eye(3).repeat(513, 1, 1), t_gt=torch.zeros(513, 3))
    for kw, name in ((dict(R_est=R[:, :2]), "R"), (dict(t_est=t[:1]), "t"), (dict(R_gt=R[:1]), "R_gt"), (dict(t_gt=t.double()), "t_gt"),
                     (dict(depth=depth.double()), "depth"), (dict(depth=depth[None]), "depth"), (dict(K=np.eye(4)), "K"),
                     (dict(mesh=(v.double(), f)), "vertices"), (dict(mesh=(v, f.long())), "faces"), (dict(mesh=v), "mesh"),
                     (dict(delta=-1.0), "delta"), (dict(delta=float("inf")), "delta"), (dict(taus=[]), "T = 0"), (dict(taus=[0.1] * 17), "T = 17"),
                     (dict(taus=[0.1, -0.1]), "taus"), (dict(taus=[float("nan")]), "taus"), (dict(diameter=0.0), "diameter"),
                     (dict(near=0.0), "near"), (many, "N = 513")):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            poseerr.vsd(**args)


# ------------------------------------------------------------------------------------------------------------ the kernels
def test_kernel_resources():
    """no kernel of poseerr.hip uses scratch or spills a vector register, and each keeps within its built
    VGPR count rounded up to the next step of 8 (built: vsd_compare 25; verify_faces, the shared raster pass, 63 as in its other two
    code objects).  The point errors have no kernel of their own here: they run posematch.hip's, which tests/test_posematch_host.py
    holds to their counts.  Read from the code object's metadata: the compiler's figures."""
    from tests._util import kernel_resources
    limits = dict(vsd_compare_kernel=32, verify_faces_kernel=64)
    found = kernel_resources(b"vsd_compare_kernel")
    print("\n[poseerr] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
