"""The pose errors on the device (sam6d_hip.poseerr over csrc/poseerr.hip) against their numpy restatement (tests/poseerr_ref.py; VSD's
z-buffers from tests/verify_ref.py's window_zbuffer).  Every comparison is bit for bit.  Nothing here is checked against bop_toolkit,
which the suite does not have."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import poseerr_ref as PR
from tests import raster_ref as RR
from tests import refine_ref as RF
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INTR = (600.0, 590.0, 320.0, 240.0)
DELTA = 2.0 ** -6  # with depths in [2, 4) every z - DELTA is a float32
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F32)
FLIP = np.concatenate([VR.rotation((0, 0, 1), math.pi), [[0.1], [0.0], [0.0]]], axis=1)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ point errors
@functools.lru_cache(maxsize=None)
def _scene(V, N, S, seed=0):
    """V points in the unit cube, N ground truths five to eight units away, the estimates turned and moved a little, S symmetries"""
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    gt = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(N)])
    est = np.stack([VR.pose(M[:, 3].astype(F64) + g.normal(size=3) * 0.2, axis=g.normal(size=3), angle=g.uniform(0, 3)) for M in gt])
    if S == 1:
        syms = poseerr.symmetry_transforms()
    elif S == 2:
        syms = poseerr.symmetry_transforms(discrete=[FLIP])
    elif S % 2:
        syms = poseerr.symmetry_transforms(continuous=[dict(axis=(0, 1, 0), offset=(0.05, 0, 0.02))], max_step=math.pi / S)
    else:
        syms = poseerr.symmetry_transforms(discrete=[FLIP], continuous=[dict(axis=(0, 1, 0), offset=(0.05, 0, 0.02))], max_step=2 * math.pi / S)
    assert syms.shape == (S, 3, 4)
    return pts, est, gt, syms


def _errors(dev, pts, est, gt, syms, unit=2.0, intr=INTR):
    """pose_errors for the view matrices est, gt (scale 1: R * 1.0f is R)"""
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    return poseerr.pose_errors(_t(pts, dev), _t(est[:, :, :3], dev), _t(est[:, :, 3], dev), _t(gt[:, :, :3], dev), _t(gt[:, :, 3], dev), intr,
                               syms=None if syms is None else _t(syms, dev), unit=unit)


def _same(dev, got, want, V, unit=2.0, skipped=False):
    for k, dt in (("mssd", torch.float32), ("mspd", torch.float32), ("mssd_sym", torch.int32), ("mspd_sym", torch.int32),
                  ("n_skipped", torch.int32), ("add_sum", torch.int64)):
        g = getattr(got, k)
        assert g.dtype == dt and torch.equal(g, _t(want[k], dev)), (k, g.cpu().numpy(), want[k])
    assert got.add.dtype == torch.float32 and torch.equal(got.add, _t(PR.add_of(want["add_sum"], F32(1.0 / unit), V), dev))
    assert np.isfinite(want["mssd"]).all() and np.isfinite(want["mspd"]).all()
    if not skipped:
        assert not want["n_skipped"].any()  # a skip cannot hide a failure


def _check(dev, pts, est, gt, syms, unit=2.0, **kw):
    want = PR.point_errors(pts, est, gt, IDENT[None] if syms is None else syms, INTR, F32(1.0 / unit))
    _same(dev, _errors(dev, pts, est, gt, syms, unit), want, len(pts), unit, **kw)
    return want


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 4099])
def test_points_chunk_and_wave_edges(dev, V):
    want = _check(dev, *_scene(V, 3, 6))
    assert (want["mssd"] > 0).all() and (want["mspd"] > 0).all() and (want["add_sum"] > 0).all()


@pytest.mark.parametrize("S", [1, 2, 33, 1024])
def test_symmetry_counts(dev, S):
    """one symmetry, an odd count, and eight LDS tiles of 128"""
    want = _check(dev, *_scene(65, 2, S))
    if S == 1024:
        assert want["mssd_sym"].max() >= 128  # a minimum beyond the first tile


@pytest.mark.parametrize("N", [1, 3, 1024])
def test_pose_counts(dev, N):
    _check(dev, *_scene(65, N, 2))


@pytest.mark.parametrize("where", ["first", "last"])
def test_maximum_on_an_end_vertex(dev, where):
    """one vertex thirty times as far from the centre as the rest: the first of the first workgroup, the last of the second"""
    pts, est, gt, syms = _scene(1030, 2, 2)
    pts = (pts * F32(0.1)).astype(F32)
    k = 0 if where == "first" else len(pts) - 1
    pts[k] = [3.0, -3.0, 3.0]
    e, g = PR.transform(est, pts)[:, None], PR.transform(PR.sym_gt(gt, syms), pts)
    d2 = ((e - g).astype(F64) ** 2).sum(axis=-1)
    ue, ve = PR.project(e, INTR)
    ug, vg = PR.project(g, INTR)
    p2 = (ue - ug).astype(F64) ** 2 + (ve - vg).astype(F64) ** 2
    assert (d2.argmax(axis=2) == k).all() and (p2.argmax(axis=2) == k).all()
    _check(dev, pts, est, gt, syms)


def test_identical_symmetries_the_lower_index_wins(dev):
    pts, est, gt, _ = _scene(65, 3, 1)
    ring = poseerr.symmetry_transforms(continuous=[dict(axis=(0, 1, 0), offset=(0.05, 0, 0.02))], max_step=math.pi / 5)
    syms = np.stack([ring[2], ring[1], ring[1], ring[3], ring[1]])
    est = PR.sym_gt(gt, ring[1:2])[:, 0].copy()
    est[:, :, 3] += F32(0.01)  # near gt o ring[1]: that symmetry is the best, at indices 1, 2 and 4
    want = _check(dev, pts, est, gt, syms)
    assert want["mssd_sym"].tolist() == [1, 1, 1] and want["mspd_sym"].tolist() == [1, 1, 1] and (want["mssd"] > 0).all()


def test_est_equal_gt_is_exactly_zero(dev):
    pts, _, gt, _ = _scene(257, 3, 1)
    for syms in (None, poseerr.symmetry_transforms(discrete=[FLIP])):
        got = _errors(dev, pts, gt, gt, syms)
        for k in ("mssd", "mspd", "add", "mssd_sym", "mspd_sym", "n_skipped", "add_sum"):
            assert not getattr(got, k).any(), k
        _check(dev, pts, gt, gt, syms)


def test_a_symmetry_that_maps_est_onto_gt(dev):
    """est = fl32(gt o syms[3]): G of that symmetry has est's bits, so both errors are exactly 0 there and nowhere else"""
    pts, _, gt, _ = _scene(65, 3, 1)
    syms = poseerr.symmetry_transforms(continuous=[dict(axis=(1, 1, 0), offset=(0.0, 0.1, 0.0))], max_step=math.pi / 5)
    est = PR.sym_gt(gt, syms)[:, 3]
    want = _check(dev, pts, est, gt, syms)
    assert want["mssd_sym"].tolist() == [3, 3, 3] and want["mspd_sym"].tolist() == [3, 3, 3]
    assert not want["mssd"].any() and not want["mspd"].any() and (want["add_sum"] > 0).all()


def test_a_point_behind_the_camera(dev):
    """pose 1 has one vertex behind the camera under the estimate: it is counted, and the pixel error is the other vertices'"""
    pts, est, gt, syms = _scene(65, 3, 2)
    pts = pts.copy()
    pts[40] = [0.0, 0.0, -6.5]
    est, gt = est.copy(), gt.copy()
    est[[0, 2], 2, 3] += F32(6.0)  # the other poses: far enough for every vertex
    gt[[0, 2], 2, 3] += F32(6.0)
    est[1], gt[1] = VR.pose((0.1, 0.0, 6.0), axis=(1.0, 0.0, 0.0), angle=0.05), VR.pose((0.0, 0.1, 10.0), angle=0.0)
    want = _check(dev, pts, est, gt, syms, skipped=True)
    assert want["n_skipped"].tolist() == [0, 1, 0]
    rest = np.delete(pts, 40, axis=0)
    without = PR.point_errors(rest, est, gt, syms, INTR, F32(0.5))
    assert want["mspd"][1] == without["mspd"][1] and want["add_sum"][1] > without["add_sum"][1]  # left out of MSPD alone


def test_point_errors_many_symmetries_through_the_c_entry(dev):
    """sam6d_pose_point_errors itself at S = 1024 over two poses of 65 points: so few workgroups per symmetry that a launch which
    splits the symmetries deals them out in many short runs, and the minimum lies in a later run than the first"""
    pts, est, gt, syms = _scene(65, 2, 1024)
    V, N, S = 65, 2, 1024
    want = PR.point_errors(pts, est, gt, syms, INTR, 0.5)
    assert want["mssd_sym"].max() >= 256 and not want["n_skipped"].any()
    d = [_t(np.asarray(a, F32), dev) for a in (pts, est, gt, syms)]
    out = dict(mssd=torch.float32, mspd=torch.float32, mssd_sym=torch.int32, mspd_sym=torch.int32, n_skipped=torch.int32, add_sum=torch.int64)
    out = {k: torch.full((N,), 77, dtype=dt, device=dev) for k, dt in out.items()}
    need = _lib.load().sam6d_pose_point_errors_workspace_bytes(N, S)
    ws = torch.full((need // 8,), 77, dtype=torch.int64, device=dev)
    _lib.call("sam6d_pose_point_errors", d[0].data_ptr(), V, d[1].data_ptr(), d[2].data_ptr(), N, d[3].data_ptr(), S, *INTR, 0.5,
              *(out[k].data_ptr() for k in ("mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")), ws.data_ptr(), need,
              torch.cuda.current_stream().cuda_stream)
    for k, b in out.items():
        assert np.array_equal(b.cpu().numpy(), want[k]), (k, b.cpu().numpy(), want[k])


def test_point_error_refusals_write_nothing(dev):
    pts, est, gt, syms = _scene(65, 3, 2)
    V, N, S, G = 65, 3, 2, 16
    d = {k: _t(a, dev) for k, a in dict(pts=pts, est=est, gt=gt, syms=syms).items()}
    sizes = dict(mssd=(N, torch.float32), mspd=(N, torch.float32), mssd_sym=(N, torch.int32), mspd_sym=(N, torch.int32),
                 n_skipped=(N, torch.int32), add_sum=(N, torch.int64))
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
    need = _lib.load().sam6d_pose_point_errors_workspace_bytes(N, S)
    assert need == 8 * N * S
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(V=V, N=N, S=S, inv_unit=0.5, ws_ptr=ws.data_ptr() + 8 * G, ws_bytes=need, **nulls):
        p = dict(points=d["pts"].data_ptr(), est=d["est"].data_ptr(), gt=d["gt"].data_ptr(), syms=d["syms"].data_ptr(), **ptr)
        p.update(nulls)
        _lib.call("sam6d_pose_point_errors", p["points"], V, p["est"], p["gt"], N, p["syms"], S, *INTR, inv_unit, p["mssd"], p["mspd"],
                  p["mssd_sym"], p["mspd_sym"], p["n_skipped"], p["add_sum"], ws_ptr, ws_bytes, stream)

    run()
    want = PR.point_errors(pts, est, gt, syms, INTR, 0.5)
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all(), k
        assert np.array_equal(h[G:-G], want[k]), k
    hw = ws.cpu().numpy()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()
    before = {k: b.clone() for k, b in bufs.items()}
    ws_before = ws.clone()
    cases = [(dict(V=0), "V = 0"), (dict(V=(1 << 20) + 1), "V = 1048577"), (dict(N=0), "N = 0"), (dict(N=1025), "N = 1025"), (dict(S=0), "S = 0"),
             (dict(S=1025), "S = 1025"), (dict(inv_unit=0.0), "inv_unit"), (dict(inv_unit=-1.0), "inv_unit"), (dict(inv_unit=float("inf")), "inv_unit"),
             (dict(inv_unit=float("nan")), "inv_unit"), (dict(ws_bytes=need - 1), "workspace"), (dict(ws_ptr=None), "workspace"),
             (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned")]
    cases += [({k: None}, k) for k in ("points", "est", "gt", "syms", "mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")]
    for kw, name in cases:
        with pytest.raises(RuntimeError, match=name):
            run(**kw)
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and torch.equal(ws, ws_before)  # a refused call writes nothing


# ------------------------------------------------------------------------------------------------------------ VSD
@functools.lru_cache(maxsize=None)
def _sphere():
    return RR.icosphere(2)


INSIDE, BORDER, THROUGH, OFF, BEHIND = range(5)  # VR.five_poses


def _render(view):
    """the nearest rendered depth of the views at VR.SIZE, 0 where nothing is"""
    v, f = _sphere()
    box = VR.windows(v, f, view, VR.INTR, VR.SIZE)[0]
    return VR.pose_verify(v, f, view, VR.INTR, VR.SIZE, 1e-3, box, np.zeros(VR.SIZE, F32), None, 0.0)[2]


def _vsd(dev, est, gt, obs, taus, delta=DELTA, diameter=None, mesh=None, intr=VR.INTR):
    v, f = mesh or _sphere()
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    got, counts = poseerr.vsd((_t(v, dev), _t(f, dev)), _t(est[:, :, :3], dev), _t(est[:, :, 3], dev), _t(gt[:, :, :3], dev), _t(gt[:, :, 3], dev),
                              intr, _t(obs, dev), delta, taus, diameter=diameter)
    inv_norm = 1.0 if diameter is None else F32(1.0 / diameter)
    want = PR.vsd_counts(v, f, np.concatenate([est, gt]), intr, obs.shape, 1e-3, obs, delta, taus, inv_norm)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (len(est), 4 + len(taus))
    assert torch.equal(counts, _t(want, dev)), (counts.cpu().numpy(), want)
    assert got.dtype == torch.float32 and torch.equal(got, _t(PR.vsd_of(want), dev))
    assert (want[:, 0] + want[:, 1] == want[:, 2] + want[:, 3]).all() and (want[:, 4:] <= want[:, 1:2]).all()
    return want, got.cpu().numpy()


def test_vsd_est_equal_gt_unoccluded(dev):
    """tau = 0: every pixel's distance 0 >= 0 costs (BOP's step cost is >=), the error is 1; tau > 0: the error is 0.  N = 1"""
    gt = VR.five_poses()[INSIDE:INSIDE + 1]
    obs = _render(gt)
    want, vsd = _vsd(dev, gt, gt, obs, [0.0, 0.05])
    n = int((obs > 0).sum())
    assert want.tolist() == [[n, n, n, n, n, 0]] and n > 500 and vsd.tolist() == [[1.0, 0.0]]


def test_vsd_disjoint_renders(dev):
    five = VR.five_poses()
    est, gt = VR.pose((-1.2, -0.05, 4.0))[None], VR.pose((1.2, -0.05, 4.0))[None]
    obs = _render(five[INSIDE:INSIDE + 1])  # something else in between
    want, vsd = _vsd(dev, est, gt, obs, [0.05])
    assert want[0, 1] == 0 and want[0, 2] > 100 and want[0, 3] > 100 and want[0, 0] == want[0, 2] + want[0, 3] and vsd.tolist() == [[1.0]]


@pytest.mark.parametrize("T", [1, 16])
def test_vsd_mixed_pairs(dev, T):
    """six pairs in one call: a moved estimate, a window cut by the image border, an estimate wholly outside the image, both outside
    (n_union 0, the error 1), a pose through the camera plane, est == gt; the depth image is the ground truths' render with a plane in
    front of the left half of the image, a strip without readings, a negative value and a NaN"""
    five = VR.five_poses()
    gt = np.stack([five[INSIDE], five[BORDER], five[INSIDE], five[OFF], five[THROUGH], VR.pose((-0.9, 0.6, 5.0))])
    est = np.stack([VR.pose((0.2, -0.1, 4.1), angle=0.8), VR.pose((1.8, 1.3, 4.2)), five[OFF], five[BEHIND], VR.pose((0.1, 0.0, 0.6)), gt[5]])
    obs = _render(gt)
    obs[:, :30] = np.where(obs[:, :30] > 0, F32(2.5), obs[:, :30])  # the plane: in front of the spheres' left parts
    obs[40:, :] = 0
    obs[20, 33], obs[21, 34] = -1.0, np.nan
    taus = [0.02 * (k + 1) for k in range(T)]
    want, vsd = _vsd(dev, est, gt, obs, taus, diameter=2.0)
    assert want[3].tolist() == [0] * (4 + T) and (vsd[3] == 1.0).all()          # both outside
    assert want[2, 2] == 0 and want[2, 3] > 0 and (vsd[2] == 1.0).all()         # the estimate outside
    assert want[1, 0] > 0 and want[0, 1] > 0 and 0 < want[0, 4] <= want[0, 1]
    assert (np.diff(want[:, 4:], axis=1) <= 0).all()                            # a larger tau costs no more
    assert want[5, 4] == 0 and vsd[5, 0] == 0.0


def test_vsd_depth_all_zero(dev):
    """no reading anywhere: everything rendered is visible"""
    five = VR.five_poses()
    est, gt = VR.pose((0.3, -0.05, 4.2))[None], five[INSIDE:INSIDE + 1]
    want, _ = _vsd(dev, est, gt, np.zeros(VR.SIZE, F32), [0.05, 0.2])
    re, rg = _render(est) > 0, _render(gt) > 0
    assert want[0, :4].tolist() == [int((re | rg).sum()), int((re & rg).sum()), int(re.sum()), int(rg.sum())]


def test_vsd_occluding_plane_in_front_of_half(dev):
    gt = VR.five_poses()[INSIDE:INSIDE + 1]
    est = VR.pose((0.15, -0.05, 4.05))[None]
    free = _render(gt)
    obs = free.copy()
    obs[:, :33] = 2.0
    want, _ = _vsd(dev, est, gt, obs, [0.05])
    open_, _ = _vsd(dev, est, gt, free, [0.05])
    assert 0 < want[0, 3] < open_[0, 3] and want[0, 3] == int((free[:, 33:] > 0).sum())  # the ground truth is visible right of the plane alone


def test_vsd_reading_exactly_delta_in_front(dev):
    """at the principal point c = 1 and D = z: a reading exactly delta in front keeps the pixel visible (<=), the next float does not"""
    gt = VR.five_poses()[INSIDE:INSIDE + 1]
    free = _render(gt)
    z = free[24, 32]
    assert 2.0 + DELTA <= z < 4.0
    seen = []
    for o in (z - F32(DELTA), np.nextafter(z - F32(DELTA), F32(0))):
        obs = free.copy()
        obs[24, 32] = o
        assert o < z and (z - o == F32(DELTA)) == (len(seen) == 0)
        seen.append(_vsd(dev, gt, gt, obs, [0.05])[0][0, 3])
    assert seen[0] == int((free > 0).sum()) == seen[1] + 1


def test_vsd_crowd_of_tiny_windows(dev):
    """512 pairs with windows of a few words: many pairs to a wave, many windows to a workgroup (the scenes of pose_crowd_ref)"""
    g = np.random.default_rng(3)
    mesh = RF.mesh_a()
    size, intr = (45, 61), (60.0, 60.0, 30.0, 22.0)
    fx, fy, cx, cy = intr
    gt, est = [], []
    for _ in range(512):
        z, px, py = g.uniform(15.0, 60.0), g.uniform(-8.0, size[1] + 8.0), g.uniform(-8.0, size[0] + 8.0)
        axis, angle = g.normal(size=3), g.uniform(0.0, 3.0)
        t = np.array([(px - cx) / fx * z, (py - cy) / fy * z, z])
        gt.append(VR.pose(t, axis=axis, angle=angle))
        est.append(VR.pose(t + g.normal(size=3) * [0.3, 0.3, 1.0], axis=axis, angle=angle + 0.2))
    gt, est = np.stack(gt), np.stack(est)
    box = VR.windows(mesh[0], mesh[1], gt, intr, size)[0]
    depth = VR.pose_verify(mesh[0], mesh[1], gt, intr, size, 1e-3, box, np.zeros(size, F32), None, 0.0)[2]
    obs = np.where(depth > 0, depth, np.where(g.random(size) < 0.5, F32(60.0), F32(0))).astype(F32)
    obs[g.random(size) < 0.05] = 0
    want, _ = _vsd(dev, est, gt, obs, [0.25, 1.0, 4.0], delta=0.5, mesh=mesh, intr=intr)
    areas = VR.areas(PR.pair_boxes(mesh[0], mesh[1], np.concatenate([est, gt]), intr, size), size)
    assert 0 < np.median(areas[areas > 0]) < 64 and (areas == 0).any() and (want[:, 1] > 0).sum() > 100 and (want[:, 4] > want[:, 6]).any()


def test_vsd_total_zero(dev):
    five = VR.five_poses()
    want, vsd = _vsd(dev, np.stack([five[OFF], five[BEHIND]]), np.stack([five[BEHIND], five[OFF]]), np.ones(VR.SIZE, F32), [0.05, 0.1])
    assert not want.any() and (vsd == 1.0).all()


def test_vsd_refusals_write_nothing_and_wild_windows_stay_inside(dev):
    v, f = _sphere()
    five = VR.five_poses()
    est, gt = np.stack([VR.pose((0.2, -0.1, 4.1)), five[BORDER], five[OFF]]), np.stack([five[INSIDE], VR.pose((1.8, 1.3, 4.2)), five[INSIDE]])
    view = np.concatenate([est, gt])
    obs = _render(gt)
    (H, W), N, T, G = VR.SIZE, 3, 2, 16
    ctypes_floats = ctypes.c_float * T
    taus = ctypes_floats(0.05, 0.1)
    pair = PR.pair_boxes(v, f, view, VR.INTR, VR.SIZE)
    box = np.concatenate([pair, pair])
    offset = np.concatenate([[0], np.cumsum(VR.areas(box, VR.SIZE))]).astype(np.int64)
    total = int(offset[-1])
    d = {k: _t(a, dev) for k, a in dict(v=v, f=f, view=view, obs=obs, box=box, offset=offset).items()}
    need = _lib.load().sam6d_pose_vsd_workspace_bytes(total, N)
    assert need == 8 * total + 64 * N
    counts = torch.full((N * (4 + T) + 2 * G,), 77, dtype=torch.int32, device=dev)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(N=N, H=H, T=T, delta=DELTA, inv_norm=1.0, near=1e-3, wave_area=0, total=total, fx=VR.INTR[0], taus=taus, ws_ptr=ws.data_ptr() + 8 * G,
            ws_bytes=need, vert=d["v"].data_ptr(), view=d["view"].data_ptr(), box=d["box"].data_ptr(), offset=d["offset"].data_ptr(),
            obs=d["obs"].data_ptr(), out=counts.data_ptr() + 4 * G):
        _lib.call("sam6d_pose_vsd", vert, len(v), d["f"].data_ptr(), len(f), view, N, fx, *VR.INTR[1:], H, W, near, wave_area, box, offset, total,
                  obs, delta, taus, T, inv_norm, out, ws_ptr, ws_bytes, stream)

    def guards():
        h, hw = counts.cpu().numpy(), ws.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all() and (hw[:G] == 77).all() and (hw[-G:] == 77).all()
        return h[G:-G].reshape(N, 4 + T)

    run()
    assert np.array_equal(guards(), PR.vsd_counts(v, f, view, VR.INTR, VR.SIZE, 1e-3, obs, DELTA, [0.05, 0.1]))
    before, ws_before = counts.clone(), ws.clone()
    for kw, name in ((dict(vert=None), "vertices"), (dict(view=None), "view"), (dict(box=None), "box"), (dict(offset=None), "offset"),
                     (dict(obs=None), "depth_obs"), (dict(taus=None), "taus"), (dict(out=None), "counts"), (dict(ws_ptr=None), "workspace"),
                     (dict(H=2049), "H x W"), (dict(N=0), "N = 0"), (dict(N=513), "N = 513"), (dict(near=0.0), "near"), (dict(T=0), "T = 0"),
                     (dict(T=17), "T = 17"), (dict(delta=-1.0), "delta"), (dict(delta=float("nan")), "delta"), (dict(inv_norm=0.0), "inv_norm"),
                     (dict(inv_norm=float("inf")), "inv_norm"), (dict(taus=ctypes_floats(0.05, -0.1)), "taus"),
                     (dict(taus=ctypes_floats(float("nan"), 0.1)), "taus"), (dict(fx=0.0), "fx"), (dict(wave_area=-1), "wave_area"),
                     (dict(total=-1), "total"), (dict(total=2 * N * H * W + 1), "total"), (dict(ws_bytes=need - 1), "workspace"),
                     (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned")):
        with pytest.raises(RuntimeError, match=name):
            run(**kw)
    assert torch.equal(counts, before) and torch.equal(ws, ws_before)  # a refused call writes nothing
    # boxes and offsets the host never sees: nothing outside the buffers is touched, whatever they hold
    wild = np.array([[-5, -7, 5000, 4000], [60, 40, 70, 50], [10, 10, 5, 5], [0, 0, -1, -1], [0, 0, 63, 47], [3, 3, 9, 9]], np.int32)
    run(box=_t(wild, dev).data_ptr())
    guards()
    for off in ([0, total, -40, 1 << 40, 7, 3, total], [0, 5, 9, -(1 << 62), 0, 0, 0], [0, 1, 2, (1 << 63) - 1, 0, 0, 0], [5, 4, 3, 2, 1, 0, 0]):
        run(offset=_t(np.array(off, np.int64), dev).data_ptr())
        guards()
