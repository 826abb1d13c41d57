"""All-pairs VSD on the device (csrc/vsdpairs.hip through sam6d_hip.posematch.pair_vsd) against the numpy restatement
tests/vsdpairs_ref.py and, where the old route can take the pairs, against poseerr.vsd on the expanded pairs: every comparison is
torch.equal.  The scenes are vsdpairs_ref's; each test asserts from the restatement's boxes that its scene is what it claims to be."""
import ctypes

import numpy as np
import pytest
import torch

from tests import posematch_ref as MR
from tests import verify_ref as VR
from tests import vsdpairs_ref as VP
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr, posematch

pytestmark = pytest.mark.gpu

F32 = np.float32
DELTA = VP.DELTA


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poses(view, dev):
    view = np.asarray(view, F32)
    return _t(view[:, :, :3], dev), _t(view[:, :, 3], dev)


def _run(dev, s):
    mesh = (_t(s.mesh[0], dev), _t(s.mesh[1], dev))
    return posematch.pair_vsd(mesh, *_poses(s.a, dev), *_poses(s.b, dev), s.intr, _t(s.obs, dev), s.delta, s.taus, diameter=s.diameter)


def _old_route(dev, s):
    """what exists without pair_vsd: the A B pairs expanded and fed to poseerr.vsd, 512 a call -> counts (A, B, 4+T)"""
    A, B = len(s.a), len(s.b)
    mesh, obs = (_t(s.mesh[0], dev), _t(s.mesh[1], dev)), _t(s.obs, dev)
    est, gt = np.repeat(s.a, B, axis=0), np.tile(s.b, (A, 1, 1))
    rows = [poseerr.vsd(mesh, *_poses(est[k:k + 512], dev), *_poses(gt[k:k + 512], dev), s.intr, obs, s.delta, s.taus, diameter=s.diameter)[1]
            for k in range(0, A * B, 512)]
    return torch.cat(rows, dim=0).reshape(A, B, -1)


def _check(dev, s, want=None, pin=None):
    """pair_vsd on a scene against the restatement (and the old route: by default where it is one call) -> counts, view_counts, box, X"""
    counts, view_counts, box, X = want or VP.want(s)
    A, B, T = len(s.a), len(s.b), len(s.taus)
    got = _run(dev, s)
    assert got.counts.dtype == torch.int32 and tuple(got.counts.shape) == (A, B, 4 + T)
    assert torch.equal(got.counts, _t(counts, dev)), (got.counts.cpu().numpy(), counts)
    assert got.vsd.dtype == torch.float32 and torch.equal(got.vsd, _t(VP.vsd_of(counts), dev))
    for field, col in ((got.n_render_a, view_counts[:A, 0]), (got.n_visible_a, view_counts[:A, 1]), (got.n_render_b, view_counts[A:, 0]),
                       (got.n_visible_b, view_counts[A:, 1])):
        assert field.dtype == torch.int32 and torch.equal(field, _t(col, dev))
    if pin if pin is not None else A * B <= 512:
        assert torch.equal(got.counts, _old_route(dev, s))
    return counts, view_counts, box, X


# ------------------------------------------------------------------------------------------------------------ pinned to the old route
def test_the_mixed_matrix_equals_the_restatement_and_the_pair_entry(dev):
    """9 x 8: empty windows, a pose through the camera plane, the occluding plane, the strip without readings, -1 and NaN"""
    s = VP.mixed()
    counts, view_counts, _, X = _check(dev, s, VP.mixed_want())
    assert (counts[:, :, 1] > 0).sum() >= 20 and (counts[:, :, 2] > view_counts[:9, 1][:, None]).sum() >= 5 and (X[:, :, 2] == 0).any()


def test_529_pairs_are_two_calls_of_the_old_route(dev):
    s = VP.crowd(23, 23)
    counts, _, _, _ = _check(dev, s, VP.crowd_want(23, 23), pin=True)
    assert len(s.a) * len(s.b) == 529 > poseerr.MAX_PAIRS and (counts[:, :, 1] > 0).sum() >= 5


# ------------------------------------------------------------------------------------------------------------ shapes
def test_one_pair_est_equal_gt_unoccluded(dev):
    """tau = 0: every pixel's distance 0 >= 0 costs, the error is 1; tau > 0: the error is 0"""
    gt = VR.five_poses()[VP.INSIDE:VP.INSIDE + 1]
    obs = VP.render(gt)
    counts, view_counts, _, _ = _check(dev, VP._scene(VP.RR.icosphere(2), gt, gt, obs, taus=[0.0, 0.05]))
    n = int((obs > 0).sum())
    assert counts.tolist() == [[[n, n, n, n, n, 0]]] and n > 500 and view_counts.tolist() == [[n, n], [n, n]]
    assert VP.vsd_of(counts).tolist() == [[[1.0, 0.0]]]


@pytest.mark.parametrize("T", [1, 16])
def test_five_poses_against_five_poses(dev, T):
    five = VR.five_poses()
    s = VP._scene(VP.RR.icosphere(2), five, five, VP.occluded(VP.render(five)), taus=[0.02 * (k + 1) for k in range(T)], diameter=2.0)
    counts, view_counts, box, _ = _check(dev, s)
    assert (VR.areas(box[:5], s.size) > 0).tolist() == [True, True, True, False, False]
    assert not counts[3:, 3:].any() and (counts[:3, :3, 0] > 0).all() and (np.diff(counts[:, :, 4:], axis=2) <= 0).all()
    lone = counts[3:, :3]  # an estimate without a window against a ground truth with one: [G, 0, 0, G, 0 ..]
    assert (lone[:, :, 0] == lone[:, :, 3]).all() and (lone[:, :, 3] > 0).all() and not lone[:, :, 1:3].any() and not lone[:, :, 4:].any()


def test_window_arithmetic_edges(dev):
    """windows that share exactly one pixel column or row, that abut without sharing, one nested in the other, one cut by the image
    border meeting one that is not; then the same poses with the roles of a and b exchanged"""
    s = VP.window_edges()
    _, _, box, X = _check(dev, s)
    (ax0, ay0, ax1, ay1), b = box[0], box[2:]
    assert b[0, 0] == ax1 and tuple(X[0, 0, 2:]) == (1, ay1 - ay0 + 1)                  # one shared column
    assert b[1, 0] == ax1 + 1 and tuple(X[0, 1, 2:]) == (0, 0)                          # x1_i + 1 == x0_j
    assert b[2, 1] == ay1 and tuple(X[0, 2, 2:]) == (ax1 - ax0 + 1, 1)                  # one shared row
    assert b[3, 1] == ay1 + 1 and tuple(X[0, 3, 2:]) == (0, 0)
    assert ax0 < b[4, 0] and b[4, 2] < ax1 and ay0 < b[4, 1] and b[4, 3] < ay1 and tuple(X[0, 4]) == (b[4, 0], b[4, 1], b[4, 2] - b[4, 0] + 1, b[4, 3] - b[4, 1] + 1)
    H, W = s.size
    assert b[5, 2] == W - 1 and b[5, 3] == H - 1 and 0 < box[1, 0] and box[1, 2] < W - 1 and box[1, 3] < H - 1 and X[1, 5, 2] > 0 and X[1, 5, 3] > 0
    _check(dev, VP._scene(s.mesh, s.b, s.a, s.obs, taus=s.taus, diameter=s.diameter))


def test_wave_and_workgroup_edges_of_the_pair_walk(dev):
    """shared rectangles of 1 x 1, 1 x 65, 63, 64 and 65 pixels, of 70 x 70 (twenty steps of the workgroup) and one 278 wide"""
    s = VP.pair_walk()
    counts, _, _, X = _check(dev, s)
    assert [tuple(x[2:]) for x in X[0, :5]] == list(VP.WALK_AREAS) and [int(x[2] * x[3]) for x in X[0, :5]] == [1, 65, 63, 64, 65]
    assert tuple(X[0, 5, 2:]) == (70, 70) and X[1, 5, 2] > 256 and X[1, 5, 2] * X[1, 5, 3] > 40000
    assert counts[0, 0, 1] == 1 and (counts[0, :5, 1] > 0).all() and counts[1, 5, 1] == X[1, 5, 2] * X[1, 5, 3]   # the one shared pixel counts


def test_crowd_of_tiny_windows(dev):
    """64 x 48 poses with windows of a few words, some empty: many views to a workgroup of the view pass, pairs with and without
    overlap"""
    s = VP.crowd(64, 48)
    counts, _, box, X = _check(dev, s, VP.crowd_want(64, 48))
    areas = VR.areas(box, s.size)
    assert 0 < np.median(areas[areas > 0]) < 64 and (areas == 0).any() and (counts[:, :, 1] > 0).sum() >= 20
    assert (X[:, :, 2] > 0).sum() > (counts[:, :, 1] > 0).sum() and (X[:, :, 2] == 0).sum() > 1000


@pytest.mark.parametrize("A, B", [(1024, 1), (1, 1024)])
def test_the_limits_of_a_and_b(dev, A, B):
    counts, _, _, _ = _check(dev, VP.crowd(A, B, 1024), VP.crowd_want(A, B, 1024), pin=False)
    assert counts.shape == (A, B, 7) and (counts[:, :, 1] > 0).any()


# ------------------------------------------------------------------------------------------------------------ depth images
def test_depth_all_zero(dev):
    """no reading anywhere: everything rendered is visible"""
    est, gt = VR.pose((0.3, -0.05, 4.2))[None], VR.five_poses()[VP.INSIDE:VP.INSIDE + 1]
    counts, view_counts, _, _ = _check(dev, VP._scene(VP.RR.icosphere(2), est, gt, np.zeros(VR.SIZE, F32), taus=[0.05, 0.2]))
    re, rg = VP.render(est) > 0, VP.render(gt) > 0
    assert counts[0, 0, :4].tolist() == [int((re | rg).sum()), int((re & rg).sum()), int(re.sum()), int(rg.sum())]
    assert view_counts.tolist() == [[int(re.sum())] * 2, [int(rg.sum())] * 2]


def test_reading_exactly_delta_in_front_of_the_ground_truth(dev):
    """at the principal point c = 1 and D = z: a reading exactly delta in front keeps the pixel visible (<=), the next float does not"""
    gt = VR.five_poses()[VP.INSIDE:VP.INSIDE + 1]
    free = VP.render(gt)
    z = free[24, 32]
    assert 2.0 + DELTA <= z < 4.0
    seen = []
    for o in (z - F32(DELTA), np.nextafter(z - F32(DELTA), F32(0))):
        obs = free.copy()
        obs[24, 32] = o
        assert o < z and (z - o == F32(DELTA)) == (len(seen) == 0)
        counts, _, _, X = _check(dev, VP._scene(VP.RR.icosphere(2), gt, gt, obs))
        assert X[0, 0, 0] <= 32 < X[0, 0, 0] + X[0, 0, 2] and X[0, 0, 1] <= 24 < X[0, 0, 1] + X[0, 0, 3]   # the pixel is inside X
        seen.append(int(counts[0, 0, 3]))
    assert seen[0] == int((free > 0).sum()) == seen[1] + 1


def test_reading_exactly_delta_in_front_of_the_estimate_where_the_ground_truth_is_visible(dev):
    """the estimate lies behind the ground truth; one reading at the principal point, none elsewhere.  Exactly delta in front of the
    estimate the pixel is the estimate's own; the next float occludes the estimate, and the pixel stays in visib_est through the ground
    truth's visibility alone: the has_e && !own_e && own_g term is 1"""
    gt, est = VR.five_poses()[VP.INSIDE:VP.INSIDE + 1], VR.pose((0.1, -0.05, 4.05))[None]
    z_e, z_g = VP.render(est)[24, 32], VP.render(gt)[24, 32]
    assert 2.0 + DELTA <= z_g < z_e < 4.0
    extra = []
    for o in (z_e - F32(DELTA), np.nextafter(z_e - F32(DELTA), F32(0))):
        obs = np.zeros(VR.SIZE, F32)
        obs[24, 32] = o
        assert z_g - o <= F32(DELTA) and (z_e - o == F32(DELTA)) == (len(extra) == 0)
        counts, view_counts, _, _ = _check(dev, VP._scene(VP.RR.icosphere(2), est, gt, obs))
        assert counts[0, 0, 2] == view_counts[0, 0] and view_counts[1, 1] == view_counts[1, 0]   # every estimate pixel is in visib_est
        extra.append(int(counts[0, 0, 2] - view_counts[0, 1]))
    assert extra == [0, 1]


# ------------------------------------------------------------------------------------------------------------ other
def test_a_set_against_itself(dev):
    """a and b the same tensors: est == gt on the diagonal, so no pixel costs for tau > 0 and the error is 0 where anything is visible"""
    s = VP.mixed()
    mesh = (_t(s.mesh[0], dev), _t(s.mesh[1], dev))
    R, t = _poses(s.a, dev)
    got = posematch.pair_vsd(mesh, R, t, R, t, s.intr, _t(s.obs, dev), s.delta, s.taus, diameter=s.diameter)
    want = VP.want(VP._scene(s.mesh, s.a, s.a, s.obs, taus=s.taus, diameter=s.diameter))[0]
    assert torch.equal(got.counts, _t(want, dev)) and min(s.taus) > 0
    diag = got.counts.cpu().numpy()[np.arange(9), np.arange(9)]
    assert not diag[:, 4:].any() and (diag[:, 0] > 0).sum() >= 5 and (diag[:, 0] == 0).any()
    vsd = got.vsd.cpu().numpy()[np.arange(9), np.arange(9)]
    assert (vsd[diag[:, 0] > 0] == 0).all() and (vsd[diag[:, 0] == 0] == 1).all()
    assert torch.equal(got.n_render_a, got.n_render_b) and torch.equal(got.n_visible_a, got.n_visible_b)


def test_vsd_matches_is_match_poses_per_tau(dev):
    s = VP.crowd(64, 48)
    counts, view_counts, _, _ = VP.crowd_want(64, 48)
    got = _run(dev, s)
    g = np.random.default_rng(9)
    scores = g.random(64).astype(F32)
    thresholds = [0.3, 0.6, 0.95, 1.5]
    visib = got.n_visible_b.to(torch.float32) / got.n_render_b.clamp(min=1).to(torch.float32)
    valid = (got.n_render_b > 0) & (visib >= 0.1)
    want_valid = (view_counts[64:, 0] > 0) & (view_counts[64:, 1].astype(F32) / np.maximum(view_counts[64:, 0], 1).astype(F32) >= F32(0.1))
    assert torch.equal(valid, _t(want_valid, dev)) and 0 < want_valid.sum() < 48
    vsd = VP.vsd_of(counts)
    for kw in (dict(), dict(valid=valid), dict(valid=valid, max_ests=20)):
        n_matched, n_targets = posematch.vsd_matches(got.vsd, _t(scores, dev), thresholds, **kw)
        ref = dict(valid=want_valid if "valid" in kw else None, max_ests=kw.get("max_ests", 0))
        want = np.stack([MR.match(vsd[:, :, k], scores, thresholds, **ref)[2] for k in range(len(s.taus))])
        assert n_matched.dtype == torch.int32 and tuple(n_matched.shape) == (3, 4) and torch.equal(n_matched, _t(want, dev))
        assert n_targets == (int(want_valid.sum()) if "valid" in kw else 48) and want[:, 0].max() > 0 and (np.diff(want, axis=1) >= 0).all()
        recall = posematch.instance_recall(n_matched, n_targets)
        assert tuple(recall.shape) == (3, 4) and 0 < float(recall.mean()) <= 1


def test_total_zero(dev):
    five = VR.five_poses()
    s = VP._scene(VP.RR.icosphere(2), five[[VP.OFF, VP.BEHIND]], five[[VP.BEHIND, VP.OFF, VP.OFF]], np.ones(VR.SIZE, F32), taus=[0.05, 0.1])
    counts, view_counts, _, _ = _check(dev, s)
    assert not counts.any() and not view_counts.any() and (_run(dev, s).vsd == 1).all()


def test_refusals_write_nothing_and_wild_windows_stay_inside(dev):
    """through the C entry, with guard words before and after counts, view_counts and the workspace"""
    v, f = VP.RR.icosphere(2)
    five = VR.five_poses()
    a, b = np.stack([VR.pose((0.2, -0.1, 4.1)), five[VP.BORDER], five[VP.OFF]]), np.stack([five[VP.INSIDE], VR.pose((1.8, 1.3, 4.2))])
    view = np.concatenate([a, b])
    obs = VP.render(b)
    (H, W), A, B, T, G = VR.SIZE, 3, 2, 2, 16
    NV = A + B
    ctypes_floats = ctypes.c_float * T
    taus = ctypes_floats(0.05, 0.1)
    box = VR.windows(v, f, view, VR.INTR, VR.SIZE)[0]
    offset = np.concatenate([[0], np.cumsum(VR.areas(box, VR.SIZE))]).astype(np.int64)
    total = int(offset[-1])
    d = {k: _t(x, dev) for k, x in dict(v=v, f=f, view=view, obs=obs, box=box, offset=offset).items()}
    need = _lib.load().sam6d_pose_pair_vsd_workspace_bytes(total, A, B)
    assert need == 8 * total + 8 * ((total + 1) // 2) + 32 * NV
    counts = torch.full((A * B * (4 + T) + 2 * G,), 77, dtype=torch.int32, device=dev)
    per_view = torch.full((NV * 2 + 2 * G,), 77, dtype=torch.int32, device=dev)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(A=A, B=B, H=H, T=T, delta=DELTA, inv_norm=1.0, near=1e-3, wave_area=0, total=total, fx=VR.INTR[0], taus=taus,
            ws_ptr=ws.data_ptr() + 8 * G, ws_bytes=need, vert=d["v"].data_ptr(), faces=d["f"].data_ptr(), view=d["view"].data_ptr(),
            box=d["box"].data_ptr(), offset=d["offset"].data_ptr(), obs=d["obs"].data_ptr(), out=counts.data_ptr() + 4 * G,
            out_view=per_view.data_ptr() + 4 * G):
        _lib.call("sam6d_pose_pair_vsd", vert, len(v), faces, len(f), view, A, B, fx, *VR.INTR[1:], H, W, near, wave_area, box, offset, total,
                  obs, delta, taus, T, inv_norm, out, out_view, ws_ptr, ws_bytes, stream)

    def guards():
        h, hv, hw = counts.cpu().numpy(), per_view.cpu().numpy(), ws.cpu().numpy()
        assert all((x[:G] == 77).all() and (x[-G:] == 77).all() for x in (h, hv, hw))
        return h[G:-G].reshape(A, B, 4 + T), hv[G:-G].reshape(NV, 2)

    run()
    want = VP.pair_vsd(v, f, a, b, VR.INTR, VR.SIZE, 1e-3, obs, DELTA, [0.05, 0.1])
    got = guards()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[0][:, :, 1] > 0).any()
    before = [x.clone() for x in (counts, per_view, ws)]
    for kw, name in ((dict(vert=None), "vertices"), (dict(faces=None), "faces"), (dict(view=None), "view"), (dict(box=None), "box"),
                     (dict(offset=None), "offset"), (dict(obs=None), "depth_obs"), (dict(taus=None), "taus"), (dict(out=None), "counts"),
                     (dict(out_view=None), "view_counts"), (dict(ws_ptr=None), "workspace"), (dict(H=2049), "H x W"), (dict(A=0), "A = 0"),
                     (dict(A=1025), "A = 1025"), (dict(B=0), "B = 0"), (dict(B=1025), "B = 1025"), (dict(near=0.0), "near"), (dict(T=0), "T = 0"),
                     (dict(T=17), "T = 17"), (dict(delta=-1.0), "delta"), (dict(delta=float("nan")), "delta"), (dict(inv_norm=0.0), "inv_norm"),
                     (dict(inv_norm=float("inf")), "inv_norm"), (dict(taus=ctypes_floats(0.05, -0.1)), "taus"),
                     (dict(taus=ctypes_floats(float("nan"), 0.1)), "taus"), (dict(fx=0.0), "fx"), (dict(wave_area=-1), "wave_area"),
                     (dict(total=-1), "total"), (dict(total=NV * H * W + 1), "total"), (dict(ws_bytes=need - 1), "workspace"),
                     (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned")):
        with pytest.raises(RuntimeError, match=name):
            run(**kw)
    assert all(torch.equal(x, y) for x, y in zip((counts, per_view, ws), before))  # a refused call writes nothing
    # boxes and offsets the host never sees: nothing outside the buffers is touched, whatever they hold
    wild = np.array([[-5, -7, 5000, 4000], [60, 40, 70, 50], [10, 10, 5, 5], [0, 0, 63, 47], [3, 3, 9, 9]], np.int32)
    run(box=_t(wild, dev).data_ptr())
    guards()
    for off in ([0, total, -40, 1 << 40, 7, total], [0, 5, 9, -(1 << 62), 0, 0], [0, 1, 2, (1 << 63) - 1, 0, 0], [5, 4, 3, 2, 1, 0]):
        run(offset=_t(np.array(off, np.int64), dev).data_ptr())
        guards()
