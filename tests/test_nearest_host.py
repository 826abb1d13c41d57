"""ADI and the model diameter (sam6d_hip.poseerr.adi / model_diameter / models_info / auc, csrc/nearest.hip): the host side and the
numpy restatement of the recipe (tests/nearest_ref.py).  No GPU: the binding, the restatement against an independent float64
evaluation within the bounds derived in nearest_ref.py, the exactness of the skip rule's bounds as a property of float32 arithmetic,
the plain torch ops, the refusals, the kernels' resources from the code object's metadata, and the clustered scene of the GPU test:
the restated skip rule fires on it, and not everywhere.  Nothing here is checked against bop_toolkit, which the suite does not have."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import nearest_ref as NR
from tests import poseerr_ref as PR
from tests import raster_ref as RR
from tests import verify_ref as VR
from tests._util import ROOT
from sam6d_hip import _lib, poseerr

F32, F64 = np.float32, np.float64
NAMES = ("sam6d_pose_adi", "sam6d_pose_adi_workspace_bytes", "sam6d_points_diameter", "sam6d_points_diameter_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ the binding
def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam6d_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared" % name
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert len(_lib.SIGNATURES["sam6d_pose_adi"]) == 11 and len(_lib.SIGNATURES["sam6d_points_diameter"]) == 9
    assert "#define SAM6D_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "sam6d_hip.h")).read()
    lib = _lib.load()
    assert lib.sam6d_pose_adi_workspace_bytes(1, 1) == 24 and lib.sam6d_pose_adi_workspace_bytes(257, 3) == 24 * 3 * 2
    assert lib.sam6d_pose_adi_workspace_bytes(1 << 20, 1024) == 24 * 1024 * 4096
    assert [lib.sam6d_pose_adi_workspace_bytes(*a) for a in ((0, 1), ((1 << 20) + 1, 1), (1, 0), (1, 1025))] == [0, 0, 0, 0]
    assert lib.sam6d_points_diameter_workspace_bytes(1) == 32 and lib.sam6d_points_diameter_workspace_bytes(4099) == 8 + 24 * 17
    assert [lib.sam6d_points_diameter_workspace_bytes(v) for v in (0, -1, (1 << 20) + 1)] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ against float64
def _scene(seed, N=4, V=300, spread=0.2):
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    gt = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(N)])
    est = np.stack([VR.pose(M[:, 3].astype(F64) + g.normal(size=3) * spread, axis=g.normal(size=3), angle=g.uniform(0, 3)) for M in gt])
    return pts, est, gt


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_against_float64(seed):
    """np.linalg.norm over the full float64 table, the minimum over j and the mean over i; the maximum over all pairs"""
    pts, est, gt = _scene(seed)
    inv_unit = F32(1.0 / 2.0)
    X = np.concatenate([pts.astype(F64), np.ones((len(pts), 1))], axis=1).T               # (4,V)
    e, g = (est.astype(F64) @ X).transpose(0, 2, 1), (gt.astype(F64) @ X).transpose(0, 2, 1)   # (N,V,3)
    exact = np.linalg.norm(e[:, :, None, :] - g[:, None, :, :], axis=-1).min(axis=2).mean(axis=1)
    rows = np.concatenate([est, gt]).astype(F64)
    B = float((np.abs(rows[:, :, :3]) @ np.abs(pts.astype(F64)).T + np.abs(rows[:, :, 3:])).max())
    got = NR.adi_of(NR.adi_sum(pts, est, gt, inv_unit), inv_unit, len(pts)).astype(F64)
    bound = NR.adi_bound(B, float(inv_unit), float(exact.max()))
    p = pts.astype(F64)
    exact_d = np.linalg.norm(p[:, None] - p[None], axis=-1).max()
    got_d, bound_d = float(NR.diameter(pts)), NR.diameter_bound(float(np.abs(p).max()))
    print("\n[nearest] B %.3g: adi err %.3g (bound %.3g), diameter err %.3g (bound %.3g)"
          % (B, np.abs(got - exact).max(), bound, abs(got_d - exact_d), bound_d))
    assert np.abs(got - exact).max() <= bound and abs(got_d - exact_d) <= bound_d
    assert exact.min() > 1e3 * bound and exact_d > 1e3 * bound_d  # the bounds bind
    # the pruned walk of the restatement is the full table's result, bit for bit
    for E, G in zip(est, gt):
        full = NR.nearest_d2(PR.transform(E, pts), PR.transform(G, pts))
        assert np.array_equal(NR.adi_walk(pts, E, G)[0], full) and np.array_equal(NR.adi_walk(pts, E, G, prune=False)[0], full)
    assert NR.diameter_walk(pts, NR.axis_seeds(pts))[0] == NR.diameter_bits(pts) == NR.diameter_walk(pts, [0], prune=False)[0]


def test_restatement_rules():
    """a NaN never wins a minimum and is above every maximum, a point without a nearest distance and a far one cost 2^42, V = 1"""
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]], F32)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F32)[None]
    moved = eye.copy()
    moved[0, 0, 3] = 0.25
    assert NR.adi_sum(pts, moved, eye, 1.0).tolist() == [3 * 2 ** 28]
    assert NR.adi_sum(pts, eye, eye, 1.0).tolist() == [0]
    bad = moved.copy()
    bad[0, 1, 3] = np.nan
    assert NR.adi_sum(pts, bad, eye, 1.0).tolist() == [3 * 2 ** 42]
    far = moved.copy()
    far[0, 0, 3] = 1e9
    assert NR.adi_sum(pts, far, eye, 1.0).tolist() == [3 * 2 ** 42]
    hole = pts.copy()
    hole[1, 2] = np.nan  # a NaN among the ground-truth points is never the nearest
    assert NR.adi_sum(hole, eye, eye, 1.0).tolist() == [2 ** 42] and np.isnan(NR.diameter(hole))
    assert NR.diameter(pts) == np.sqrt(F32(10.0)) and NR.diameter(pts[:1]) == 0.0
    assert np.isnan(NR.diameter(np.array([[np.inf, 0.0, 0.0]], F32)))
    # an infinite coordinate: the seeds see +inf, under which every finite point could skip every tile; the point itself never skips
    # its own tile, where x - x is the NaN that is above +inf
    hole[1, 2] = np.inf
    assert NR.seed_bits(hole, [0]) == 0x7F800000 and NR.diameter_bits(hole) == 0x7FC00000 == NR.diameter_walk(hole, [0])[0]


# ------------------------------------------------------------------------------------------------------------ the bounds are exact
def _tile_cases(g, kind):
    """one tile of 256 ground-truth points and 400 estimate points, float32 as the kernels form them"""
    x = g.uniform(-1.0, 1.0, (4096, 3)).astype(F32)
    x = x[np.argsort(x[:, g.integers(3)])]  # slabs, as a sorted model's tiles are compact
    far = kind == "far"
    t = np.array([4096.0, -4096.0, 4096.0]) if far else g.uniform(-1, 1, 3) + [0, 0, 6]
    G = VR.pose(t, axis=g.normal(size=3), angle=g.uniform(0, 3))
    turn = VR.rotation(g.normal(size=3), 0.03) @ G[:, :3].astype(F64)  # the estimate: 0.03 rad and a little way off
    E = np.concatenate([turn, (t + g.normal(size=3) * (2.0 ** -10 if far else 0.05))[:, None]], axis=1).astype(F32) if kind != "self" else G
    a = int(g.integers(0, 4096 - 256))
    own = g.integers(a, a + 256, 200)          # points of the tile itself
    other = g.integers(0, 4096, 200)           # points anywhere in the model
    rows = np.concatenate([own, other])
    return PR.transform(E, x[rows]), PR.transform(G, x[a:a + 256]), x[rows], x[a:a + 256]


def test_bounds_hold_in_float32():
    """lb <= min_j d2_ij and ub >= max_j d2_ij with no margin, over 1.2e5 (point, tile) cases: estimates near the ground truth, the
    point itself in the tile under the same pose (zero distances), and translations of 4096 units against a unit model, where the
    cancellation quantises every distance to multiples of 2^-11"""
    g = np.random.default_rng(7)
    n = tight = positive = zeros = 0
    for k in range(300):
        kind = ("near", "self", "far")[k % 3]
        e, gj, x, xj = _tile_cases(g, kind)
        lo, hi = NR.boxes(gj)
        d2 = NR.d2_table(e, gj)
        lb, dmin = NR.lower_bound(e, lo[0], hi[0]), d2.min(axis=1)
        assert lb.dtype == F32 and d2.dtype == F32 and (lb <= dmin).all(), (kind, k)
        lo, hi = NR.boxes(xj if kind != "far" else gj)
        p = x if kind != "far" else e
        d2x = NR.d2_table(p, xj if kind != "far" else gj)
        ub, dmax = NR.upper_bound(p, lo[0], hi[0]), d2x.max(axis=1)
        assert ub.dtype == F32 and (ub >= dmax).all(), (kind, k)
        n += len(e)
        tight += int((lb == dmin).sum()) + int((ub == dmax).sum())
        positive += int((lb > 0).sum())
        zeros += int((dmin == 0).sum())
    print("\n[nearest] %d cases: %d bounds attained exactly, %d lower bounds above 0, %d zero distances" % (n, tight, positive, zeros))
    assert n >= 100000 and positive > n // 10 and zeros > 1000 and tight > 1000


# ------------------------------------------------------------------------------------------------------------ plain torch ops
def test_extent_auc_and_morton_order():
    pts = torch.tensor([[1.0, -2.0, 0.5], [3.0, 4.0, 0.5], [-1.0, 0.0, 2.5]])
    assert poseerr._extent(pts).tolist() == [-1.0, -2.0, 0.5, 4.0, 6.0, 2.0]
    assert poseerr.INFO_FIELDS == ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")
    m = 0.5  # (exact in float32, as m / 2 and 2 m are)
    got = poseerr.auc(torch.tensor([0.0, m / 2, m, 2 * m, float("nan")]), m)
    assert got.dtype == torch.float64 and got.dim() == 0 and abs(float(got) - 0.3) <= 1e-15
    assert float(poseerr.auc(torch.tensor([0.0, 0.0], dtype=torch.float64), 5.0)) == 1.0
    assert float(poseerr.auc(torch.tensor([7.0]), 5.0)) == 0.0
    for bad, name in ((dict(err=torch.zeros(2, 2), max_err=1.0), "err"), (dict(err=torch.zeros(0), max_err=1.0), "err"),
                      (dict(err=[0.1], max_err=1.0), "err"), (dict(err=torch.zeros(2), max_err=0.0), "max_err"),
                      (dict(err=torch.zeros(2), max_err=float("nan")), "max_err"), (dict(err=torch.zeros(2), max_err=float("inf")), "max_err")):
        with pytest.raises(ValueError, match=name):
            poseerr.auc(**bad)
    g = torch.Generator().manual_seed(0)
    cloud = torch.rand(1000, 3, generator=g)
    cloud[5, 1], cloud[6, 0] = float("nan"), float("inf")
    order = poseerr.morton_order(cloud)
    assert order.dtype == torch.int64 and sorted(order.tolist()) == list(range(1000))  # a permutation, whatever the points hold
    corners = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    assert poseerr.morton_order(corners).tolist() == [1, 2, 4, 3, 0]  # x is the lowest bit, z the highest
    assert poseerr.morton_order(torch.zeros(3, 3)).tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    v, f = RR.octahedron()
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.adi(v, R, t, R, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        poseerr.adi(dict(vertices=v.numpy(), faces=f.numpy()), R, t, R, t)
    for fn in (poseerr.model_diameter, poseerr.models_info):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(v)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn((v, f))
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(dict(vertices=v.numpy(), faces=f.numpy()))
        for bad, name in ((v.double(), "points"), (v[:, :2], "points"), (torch.zeros(0, 3), "V = 0"), (v.numpy(), "points")):
            with pytest.raises(ValueError, match=name):
                fn(bad)
    base = dict(mesh_or_points=v, R_est=R, t_est=t, R_gt=R, t_gt=t)
    many = dict(R_est=torch.eye(3).repeat(1025, 1, 1), t_est=torch.zeros(1025, 3), R_gt=torch.eye(3).repeat(1025, 1, 1), t_gt=torch.zeros(1025, 3))
    for kw, name in ((dict(R_est=R[:, :2]), "R_est"), (dict(R_est=R.double()), "R_est"), (dict(t_est=t[:1]), "t_est"), (dict(R_gt=R[:1]), "R_gt"),
                     (dict(t_gt=t.double()), "t_gt"), (dict(t_gt=t[:, :2]), "t_gt"), (dict(mesh_or_points=v.double()), "points"),
                     (dict(mesh_or_points=v[:, :2]), "points"), (dict(mesh_or_points=torch.zeros(0, 3)), "V = 0"), (dict(unit=0.0), "unit"),
                     (dict(unit=float("nan")), "unit"), (many, "N = 1025")):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            poseerr.adi(**args)


# ------------------------------------------------------------------------------------------------------------ the kernels
def test_kernel_resources():
    """no kernel of nearest.hip uses scratch or spills a vector register, and each keeps within its built
    VGPR count rounded up to the next step of 8 (built: nn_boxes 14, nn_adi 40, nn_seed 8, nn_diameter 36, nn_diameter_finish 7).
    Read from the code object's metadata: the compiler's figures."""
    from tests._util import kernel_resources
    limits = dict(nn_boxes_kernel=16, nn_adi_kernel=40, nn_seed_kernel=8, nn_diameter_kernel=40, nn_diameter_finish_kernel=8)
    found = kernel_resources(b"nn_adi_kernel")
    print("\n[nearest] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])


# ------------------------------------------------------------------------------------------------------------ the GPU test's scene
def test_two_clusters_scene_prunes_and_not_everything():
    """The scene tests/test_nearest_gpu.py runs unsorted, walked here by the restated skip rule: at least half of its (1024-point
    chunk, tile) combinations are skipped, so a device prune that never fires would be a prune the restatement contradicts, and
    not all are (a prune that skips everything gives 2^42 per point).  The nearest vertex of some points lies in another tile than
    their own, and the pruned walk gives the full table's minima."""
    pts, est, gt = NR.two_clusters()
    assert pts.shape == (2050, 3)
    total = skipped = 0
    for E, G in zip(est, gt):
        m, walked = NR.adi_walk(pts, E, G)
        e, g = PR.transform(E, pts), PR.transform(G, pts)
        d2 = NR.d2_table(e, g)
        assert np.array_equal(m, d2.min(axis=1))
        assert walked.shape == (3, 9) and walked.any(axis=1).all()
        total, skipped = total + walked.size, skipped + int((~walked).sum())
        elsewhere = int((d2.argmin(axis=1) // NR.TILE != np.arange(len(pts)) // NR.TILE).sum())
        assert elsewhere > 20, elsewhere
    print("\n[nearest] two clusters: %d of %d (chunk, tile) combinations skipped" % (skipped, total))
    assert 2 * skipped >= total and skipped < total
    bits, walked = NR.diameter_walk(pts, NR.axis_seeds(pts))
    assert bits == NR.diameter_bits(pts) and not walked.all()
