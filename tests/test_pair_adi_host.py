"""All-pairs ADI with its cap (sam6d_hip.posematch.pair_adi / nms_poses_adi, csrc/pairadi.hip): the host side and the numpy restatement
(tests/pair_adi_ref.py).  No GPU: that the lower bound never exceeds the full table's sum, as a property of float32, on random and on
adversarial inputs; that a skipped pair is above the cap; that the inputs the GPU test reuses give skipped and computed pairs; that
NMS on the capped matrix is NMS on the uncapped one, also with the threshold on an entry and one ulp beside it; the use case (a cuboid
without a symmetry annotation); the binding and the refusals.  Nothing here is checked against bop_toolkit, which the suite does not
have."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import nearest_ref as NR
from tests import pair_adi_ref as AR
from tests import posematch_ref as MR
from tests import poseerr_ref as PR
from tests import verify_ref as VR
from tests._util import ROOT
from sam6d_hip import _lib, posematch

F32, F64 = np.float32, np.float64
NAMES = ("sam6d_pose_pair_adi", "sam6d_pose_pair_adi_workspace_bytes")
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F32)
# the shapes of tests/test_pair_adi_gpu.py: every V with (3, 5), every (A, B) with V = 257
GPU_CASES = [(V, 3, 5) for V in (1, 255, 256, 257, 1023, 1024, 1025, 2049)] + [(257, 1, 1), (257, 5, 3), (257, 33, 2)]


# ------------------------------------------------------------------------------------------------------------ the binding
def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam6d_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared" % name
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert len(_lib.SIGNATURES[NAMES[0]]) == 15
    ws = _lib.load().sam6d_pose_pair_adi_workspace_bytes
    assert ws(1, 1, 1) == 24 and ws(257, 3, 5) == 24 * 5 * 2 and ws(1 << 20, 2, 1024) == 24 * 1024 * 4096
    assert ws(2048, 1024, 1024) == 24 * 1024 * 8 and ws(1024, 1024, 1024) == 24 * 1024 * 4
    bad = ((0, 1, 1), ((1 << 20) + 1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1025, 1), (1, 1, 1025), (4097, 1024, 1024), (1 << 20, 65, 64))
    assert [ws(*x) for x in bad] == [0] * len(bad)
    assert posematch.MAX_ADI_WORKGROUPS == 1 << 22


# ------------------------------------------------------------------------------------------------------------ soundness
def _check_sound(points, a, b, inv_unit=AR.INV_UNIT, order=None):
    """lower_sum <= adi_sum entry by entry, and per point lb_i <= m_i; -> (lower_sum, adi_sum)"""
    points = np.asarray(points, F32)
    full = AR.pair_adi_sum(points, a, b, inv_unit)
    lower = AR.pair_lower_sum(points, a, b, inv_unit, order)
    assert (lower <= full).all(), (lower, full)
    assert (lower >= 0).all() and (full <= len(points) * 2 ** 42).all()
    moved = points if order is None else points[order]
    with np.errstate(all="ignore"):
        for E in np.asarray(a, F32):
            for G in np.asarray(b, F32):
                e, g = PR.transform(E, moved), PR.transform(G, moved)
                lb, m = AR.point_lower_bounds(e, g), NR.nearest_d2(e, g)
                assert not np.isnan(lb).any() and not np.isnan(m).any()
                assert (lb <= m).all()
    return lower, full


@pytest.mark.parametrize("V", [1, 255, 257, 1025])
def test_lower_sum_never_exceeds_adi_sum_on_random_poses(V):
    g = np.random.default_rng(V)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    a = np.stack([VR.pose(g.uniform(-3, 3, 3), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(3)])
    b = np.stack([VR.pose(g.uniform(-3, 3, 3), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(2)] + [a[0]])
    lower, full = _check_sound(pts, a, b)
    assert (lower < full).any() or V == 1
    if V == 1:  # one point, one tile: the box is the point and the bound is the distance itself
        assert np.array_equal(lower, full)
    _check_sound(pts, a, b, order=AR.morton_order(pts))


def test_lower_sum_never_exceeds_adi_sum_on_adversarial_inputs():
    g = np.random.default_rng(9)
    # points on box faces: an integer grid under integer translations, so that e lies exactly on the faces of g's tiles
    grid = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    shifts = np.stack([IDENTITY] * 4)
    shifts[1, :, 3], shifts[2, :, 3], shifts[3, :, 3] = (7.0, 0.0, 0.0), (8.0, -8.0, 10.0), (0.5, 0.0, -9.0)
    lower, full = _check_sound(grid, shifts, shifts)
    assert (np.diag(full) == 0).all() and (np.diag(lower) == 0).all() and (lower > 0).any()
    # +0 and -0 in the points and in the poses
    zeros = g.choice(F32([0.0, -0.0, 1.0, -1.0]), (300, 3)).astype(F32)
    signed = np.stack([IDENTITY, -IDENTITY, IDENTITY * F32(-0.0), IDENTITY])
    signed[3, :, 3] = -0.0
    _check_sound(zeros, signed, signed)
    # a NaN in a pose, on either side; an infinite translation; an infinite coordinate of the model
    pts = g.uniform(-1.0, 1.0, (600, 3)).astype(F32)
    poses = np.stack([VR.pose((0.1 * k, 0.0, 5.0), angle=0.7 + 0.01 * k) for k in range(4)])
    poses[1, 0, 3], poses[2, 1, 1], poses[3, 2, 3] = np.nan, np.nan, np.inf
    lower, full = _check_sound(pts, poses, poses)
    assert full[0, 1] == 600 * 2 ** 42 and lower[0, 1] == full[0, 1]  # an empty box in x: the gap is +inf
    assert full[1, 0] == 600 * 2 ** 42 and lower[1, 0] < full[1, 0]   # a NaN coordinate of e: its gap is 0
    for bad in (np.inf, -np.inf):
        hole = pts.copy()
        hole[300, 1], hole[17, 0] = bad, -bad
        _check_sound(hole, poses[:1], poses[:1])
        _check_sound(hole, poses, poses)
    # a tile whose points are all NaN (the empty box), beside tiles that have numbers
    empty = pts.copy()
    empty[256:512] = np.nan
    lo, hi = NR.boxes(empty)
    assert np.isposinf(lo[1]).all() and np.isneginf(hi[1]).all() and np.isfinite(lo[[0, 2]]).all()
    lower, full = _check_sound(empty, poses[:1], np.stack([poses[0], VR.pose((3.0, 0.0, 5.0))]))
    assert full[0, 0] == 256 * 2 ** 42 and lower[0, 1] > 0
    # V = 1
    _check_sound(pts[:1], poses, poses)


# ------------------------------------------------------------------------------------------------------------ the decision
@pytest.mark.parametrize("V, A, B", GPU_CASES)
def test_gpu_inputs_skip_some_pairs_and_not_all_and_every_skipped_pair_is_above_the_cap(V, A, B):
    """A condition on the inputs of tests/test_pair_adi_gpu.py: under each cap, sorted or not, at least one pair is skipped and at
    least one is computed.  The one exception is A = B = 1, which has one pair: there the smaller cap skips it and the larger one
    does not.  And for every skipped pair the full table's sum is above cap_sum."""
    pts, a, b, full = AR.scene(V, A, B)
    for sort in (False, True):
        lower = AR.scene_lower(V, A, B, sort)
        assert (lower <= full).all()
        kinds = []
        for cap in AR.CAPS:
            want = AR.capped(full, lower, cap, AR.INV_UNIT, V)
            limit = AR.cap_sum(cap, AR.INV_UNIT, V)
            assert limit > 0 and (full[want["skipped"]] > limit).all()
            assert (want["adi_sum"][want["skipped"]] == -1).all() and np.isposinf(want["adi"][want["skipped"]]).all()
            assert np.array_equal(want["adi_sum"][~want["skipped"]], full[~want["skipped"]])
            kinds.append((bool(want["skipped"].any()), bool((~want["skipped"]).any())))
        if A * B > 1:
            assert kinds == [(True, True), (True, True)], kinds
        else:
            assert kinds == [(True, False), (False, True)], kinds


def test_cap_sum():
    assert AR.cap_sum(0.0, 1.0, 7) == 0 and AR.cap_sum(1.0, 1.0, 1) == 1 << 30 and AR.cap_sum(0.5, 0.5, 3) == 3 << 28
    assert AR.cap_sum(1e300, 1.0, 1 << 20) == (1 << 63) - 1 and AR.cap_sum(2.0 ** 33, 1.0, 1) == (1 << 63) - 1
    assert AR.cap_sum(2.0 ** 32, 1.0, 1) == 1 << 62
    for cap, inv_unit, V in ((0.03, AR.INV_UNIT, 257), (1.0, F32(1.0 / 3.0), 2049), (1e-12, 1.0, 1), (1e300, 1.0, 5)):
        assert posematch._cap_sum("pair_adi", cap, float(F32(inv_unit)), V) == AR.cap_sum(cap, inv_unit, V)


# ------------------------------------------------------------------------------------------------------------ NMS
def test_nms_on_the_capped_matrix_is_nms_on_the_uncapped_matrix():
    pts, poses, scores = AR.nms_scene()
    V, N = len(pts), len(poses)
    full = AR.pair_adi_sum(pts, poses, poses, AR.INV_UNIT)
    lower = AR.pair_lower_sum(pts, poses, poses, AR.INV_UNIT)
    uncapped = NR.adi_of(full, AR.INV_UNIT, V)
    assert uncapped.dtype == F32 and uncapped.shape == (N, N)
    off = uncapped[~np.eye(N, dtype=bool)]
    picks = np.unique(off[np.isfinite(off)])
    picks = picks[:: max(1, len(picks) // 12)]
    thresholds = [0.0, 1e-4, 0.01, 0.05, 0.3, 1.0, 5.0, 100.0, 1e4]
    for v in picks:  # exactly on an entry's float32 value, and one ulp to either side
        thresholds += [float(v), float(np.nextafter(v, F32(np.inf))), float(np.nextafter(v, F32(-np.inf)))]
    n_skipped, counts = 0, set()
    for thresh in thresholds:
        if thresh < 0.0:
            continue
        want = MR.nms(uncapped, scores, thresh)
        cap = AR.nms_cap(thresh)
        got = AR.capped(full, lower, cap, AR.INV_UNIT, V)
        # what the derivation in nms_poses_adi says: no skipped entry is below the threshold pose_nms compares with
        assert not (uncapped[got["skipped"]] < F32(thresh)).any()
        have = MR.nms(got["adi"], scores, thresh)
        assert all(np.array_equal(x, y) for x, y in zip(have, want)), thresh
        n_skipped += int(got["skipped"].sum())
        counts.add(int(want[1][0]))
    assert n_skipped > 0 and len(counts) >= 3, (n_skipped, counts)
    (keep, count, by), adi = AR.nms_adi(pts, poses, scores, 0.05, AR.INV_UNIT)
    assert np.array_equal(keep, MR.nms(uncapped, scores, 0.05)[0]) and np.isposinf(adi).any()


def test_a_cuboid_without_symmetry_annotation():
    """two poses half a turn about the cuboid's axis and one distinct pose: MSSD without syms keeps three, ADI keeps two"""
    pts, poses, scores, thresh = AR.cuboid_case()
    mssd = MR.pair_errors(pts, poses, poses, IDENTITY[None], (100.0, 100.0, 50.0, 50.0))["mssd"]
    assert MR.nms(mssd, scores, thresh)[1][0] == 3 and mssd[0, 1] > 5 * thresh
    (keep, count, by), adi = AR.nms_adi(pts, poses, scores, thresh)
    assert count[0] == 2 and keep.tolist() == [0, 2, -1] and by.tolist() == [0, 0, 2]
    assert adi[0, 1] < 1e-5 and adi[1, 0] < 1e-5 and adi[0, 2] > thresh


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch():
    pts = torch.zeros(8, 3)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    s = torch.zeros(2)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_adi(pts, R, t, R, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_adi(pts, R, t, R, t, cap=0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_adi(dict(vertices=pts.numpy()), R, t, R, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_adi(pts, R[:0], t[:0], R, t)  # an empty side is no way round the device check
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.nms_poses_adi(pts, R, t, s, 0.1)
    with pytest.raises(ValueError, match="R_a"):
        posematch.pair_adi(pts, R[0], t, R, t)
    with pytest.raises(ValueError, match="t_a"):
        posematch.pair_adi(pts, R, t[:1], R, t)
    with pytest.raises(ValueError, match="R_b"):
        posematch.pair_adi(pts, R, t, R.double(), t)
    with pytest.raises(ValueError, match="t_b"):
        posematch.pair_adi(pts, R, t, R, t.reshape(3, 2))
    with pytest.raises(ValueError, match="R_b"):
        posematch.pair_adi(pts, R, t, R.repeat(513, 1, 1), t.repeat(513, 1))
    with pytest.raises(ValueError, match="points"):
        posematch.pair_adi(torch.zeros(8, 2), R, t, R, t)
    with pytest.raises(ValueError, match="V = 0"):
        posematch.pair_adi(torch.zeros(0, 3), R, t, R, t)
    with pytest.raises(ValueError, match="unit"):
        posematch.pair_adi(pts, R, t, R, t, unit=0.0)
    for cap in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="cap"):
            posematch.pair_adi(pts, R, t, R, t, cap=cap)
    big_R, big_t = R.repeat(512, 1, 1), t.repeat(512, 1)
    with pytest.raises(ValueError, match="A B ceil\\(V / 1024\\) = 1024 x 1024 x 5"):  # the launch's cap, before anything is launched
        posematch.pair_adi(torch.zeros(4097, 3), big_R, big_t, big_R, big_t)
    for thresh in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="thresh"):
            posematch.nms_poses_adi(pts, R, t, s, thresh)
    with pytest.raises(ValueError, match="scores"):
        posematch.pose_nms(torch.zeros(2, 2), torch.zeros(3), 0.1)


# ------------------------------------------------------------------------------------------------------------ the kernels
def test_kernel_resources():
    """pairadi.hip's code object holds its three kernels and no copy of nearest.hip's, none uses scratch
    or spills a vector register, and each keeps within its built VGPR count rounded up to the next step of 8 (built: bound 46, walk
    39 -- nn_adi_kernel's figure, the same nn_adi_chunk -- finish 6).  Read from the code object's metadata: the compiler's figures."""
    from tests._util import kernel_resources
    limits = dict(pair_adi_bound_kernel=48, pair_adi_walk_kernel=40, pair_adi_finish_kernel=8)
    found = kernel_resources(b"pair_adi_walk_kernel")
    print("\n[pairadi] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
