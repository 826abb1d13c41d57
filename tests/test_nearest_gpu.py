"""ADI and the model diameter on the device (sam6d_hip.poseerr.adi / model_diameter / models_info over csrc/nearest.hip) against
their numpy restatement by brute force (tests/nearest_ref.py).  Every comparison is bit for bit, with and without the skipping, sorted
and unsorted.  Nothing here is checked against bop_toolkit, which the suite does not have."""
import functools

import numpy as np
import pytest
import torch

from tests import nearest_ref as NR
from tests import poseerr_ref as PR
from tests import raster_ref as RR
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
UNIT = 2.0
TERM_MAX = 2 ** 42


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ ADI
def _near(M, g, angle, move):
    """the pose M turned by `angle` about a random axis through the object's origin and moved by about `move`"""
    R = VR.rotation(g.normal(size=3), angle) @ M[:, :3].astype(F64)
    return np.concatenate([R, (M[:, 3].astype(F64) + g.normal(size=3) * move)[:, None]], axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def _scene(V, N, seed=0):
    """V points in the unit cube, N ground truths five to eight units away; the estimates by turns a little off (0.05 rad, 0.02
    units), moved alone, and an unrelated rotation, where the first tile does not tighten the minimum; and the brute-force sums"""
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    gt = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(N)])
    est = np.stack([_near(M, g, (0.05, 0.0, g.uniform(1, 3))[n % 3], (0.02, 0.1, 0.2)[n % 3]) for n, M in enumerate(gt)])
    return pts, est, gt, NR.adi_sum(pts, est, gt, F32(1.0 / UNIT))


def _adi(dev, pts, est, gt, **kw):
    """adi for the view matrices est, gt (scale 1: R * 1.0f is R)"""
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    return poseerr.adi(_t(pts, dev), _t(est[:, :, :3], dev), _t(est[:, :, 3], dev), _t(gt[:, :, :3], dev), _t(gt[:, :, 3], dev), unit=UNIT, **kw)


def _same(dev, got, want, V):
    assert got.adi_sum.dtype == torch.int64 and torch.equal(got.adi_sum, _t(want, dev)), (got.adi_sum.cpu().numpy(), want)
    assert got.adi.dtype == torch.float32 and torch.equal(got.adi, _t(NR.adi_of(want, F32(1.0 / UNIT), V), dev))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1025, 4099])
def test_adi_wave_tile_and_chunk_edges(dev, V):
    pts, est, gt, want = _scene(V, 3)
    assert (want > 0).all() and (want < V * TERM_MAX).all()
    _same(dev, _adi(dev, pts, est, gt), want, V)
    _same(dev, _adi(dev, pts, est, gt, prune=False, sort=False), want, V)


@pytest.mark.parametrize("N", [1, 1024])
def test_adi_pose_counts(dev, N):
    pts, est, gt, want = _scene(65, N)
    _same(dev, _adi(dev, pts, est, gt), want, 65)


def test_adi_routes_and_point_orders_agree(dev):
    """pruned or not, sorted or not, the points in a random order: the same integer"""
    pts, est, gt, want = _scene(1025, 3)
    for kw in (dict(prune=False), dict(prune=True), dict(sort=False), dict(sort=False, prune=False)):
        _same(dev, _adi(dev, pts, est, gt, **kw), want, 1025)
    perm = np.random.default_rng(5).permutation(1025)
    for kw in (dict(), dict(sort=False)):
        _same(dev, _adi(dev, pts[perm], est, gt, **kw), want, 1025)


def test_adi_est_equal_gt_is_exactly_zero(dev):
    pts, _, gt, _ = _scene(257, 3)
    for kw in (dict(), dict(prune=False), dict(sort=False)):
        got = _adi(dev, pts, gt, gt, **kw)
        assert not got.adi_sum.any() and not got.adi.any()


def test_adi_two_clusters_unsorted(dev):
    """the scene tests/test_nearest_host.py walks with the restated skip rule: more than half of its (chunk, tile) combinations are
    skipped and the nearest vertex of some points lies in another tile than their own.  Unsorted, so the tiles are the scene's"""
    pts, est, gt = NR.two_clusters()
    want = NR.adi_sum(pts, est, gt, F32(1.0 / UNIT))
    assert (want > 0).all() and (want < len(pts) * 2 ** 30).all()  # below 2 units a point: every point found a vertex of its own ball
    for kw in (dict(sort=False), dict(sort=False, prune=False), dict()):
        _same(dev, _adi(dev, pts, est, gt, **kw), want, len(pts))


def test_adi_far_from_the_origin_ties_and_zeros(dev):
    """a unit model 4096 units from the camera: every coordinate is a multiple of 2^-11, many distances tie and many are 0"""
    g = np.random.default_rng(11)
    pts = g.uniform(-1.0, 1.0, (513, 3)).astype(F32)
    gt = np.stack([VR.pose((4096.0, -4096.0, 4096.0), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(3)])
    est = np.stack([_near(M, g, 2.0 ** -12, 2.0 ** -12) for M in gt])
    m = np.stack([NR.nearest_d2(PR.transform(E, pts), PR.transform(G, pts)) for E, G in zip(est, gt)])
    assert (m == 0).sum() > 100 and (m > 0).sum() > 1000 and all(len(np.unique(row)) < 32 for row in m)
    want = NR.adi_sum(pts, est, gt, F32(1.0 / UNIT))
    for kw in (dict(), dict(prune=False), dict(sort=False)):
        _same(dev, _adi(dev, pts, est, gt, **kw), want, 513)


def test_adi_a_nan_in_one_pose(dev):
    pts, est, gt, want = _scene(257, 3)
    est = est.copy()
    est[1, 0, 3] = np.nan
    bad = NR.adi_sum(pts, est, gt, F32(1.0 / UNIT))
    assert bad[1] == 257 * TERM_MAX and bad[0] == want[0] and bad[2] == want[2]
    for kw in (dict(), dict(prune=False)):
        _same(dev, _adi(dev, pts, est, gt, **kw), bad, 257)


# ------------------------------------------------------------------------------------------------------------ the diameter
def _bits(x):
    return int(x.reshape(1).view(torch.int32).item()) & 0xFFFFFFFF


def _diameter(dev, pts, **kw):
    got = poseerr.model_diameter(_t(pts, dev), **kw)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.device.type == "cuda"
    return got


def _check_diameter(dev, pts, routes=(dict(), dict(prune=False), dict(sort=False), dict(sort=False, prune=False))):
    want = NR.diameter(pts)
    for kw in routes:
        got = _diameter(dev, pts, **kw)
        assert _bits(got) == int(np.array([want], F32).view(np.uint32)[0]), (kw, float(got), float(want))
    return want


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1025, 4099])
def test_diameter_tile_and_chunk_edges(dev, V):
    pts = np.random.default_rng(V).uniform(-1.0, 1.0, (V, 3)).astype(F32)
    want = _check_diameter(dev, pts)
    assert (want == 0) == (V == 1)


@pytest.mark.parametrize("ends", [(0, 1029), (3, 200), (1029, 1029)])
def test_diameter_where_the_farthest_pair_lies(dev, ends):
    """a small cloud and two far vertices: the first and the last index (two chunks), both inside one tile; and a single far vertex"""
    pts = (np.random.default_rng(2).uniform(-1.0, 1.0, (1030, 3)) * 0.1).astype(F32)
    pts[ends[0]], pts[ends[1]] = [3.0, -3.0, 3.0], [-3.0, 2.5, -3.0]
    d2 = NR.d2_table(pts, pts)
    assert set(ends) <= set(int(i) for i in np.unravel_index(d2.argmax(), d2.shape))
    _check_diameter(dev, pts)


def test_diameter_sphere_and_needle(dev):
    """points on a sphere in random order, where the restated rule skips nothing, and a 100 : 1 needle sorted along the curve, where
    it skips almost every tile pair"""
    g = np.random.default_rng(3)
    sphere = g.normal(size=(2040, 3))
    sphere = (sphere / np.linalg.norm(sphere, axis=1, keepdims=True)).astype(F32)
    walked = NR.diameter_walk(sphere, NR.axis_seeds(sphere))[1]
    assert walked.shape == (2, 8) and all(walked[c, 4 * c:].all() for c in range(2))
    _check_diameter(dev, sphere, routes=(dict(sort=False), dict(sort=False, prune=False), dict()))
    needle = (g.uniform(-1.0, 1.0, (2040, 3)) * [100.0, 1.0, 1.0]).astype(F32)
    order = poseerr.morton_order(torch.from_numpy(needle)).numpy()
    walked = NR.diameter_walk(needle[order], NR.axis_seeds(needle[order]))[1]
    assert 1 <= walked.sum() <= 3, walked  # of 8 + 4 tile pairs
    _check_diameter(dev, needle)


def test_diameter_tie_and_values_that_are_not_finite(dev):
    pts = (np.random.default_rng(4).uniform(-1.0, 1.0, (600, 3)) * 0.1).astype(F32)
    pts[[7, 300]], pts[[8, 599]] = [2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]  # the farthest pair twice
    assert _check_diameter(dev, pts) == 4.0
    for bad in (np.inf, -np.inf, np.nan):
        hole = pts.copy()
        hole[450, 1] = bad
        for kw in (dict(), dict(sort=False), dict(prune=False)):
            assert torch.isnan(_diameter(dev, hole, **kw)), (bad, kw)
    assert np.isnan(NR.diameter(hole))


def test_models_info_of_a_small_mesh(dev):
    v, f = RR.icosphere(2, 60.0)
    v = (v * F32([1.0, 0.5, 0.25]) + F32([5.0, 0.0, -7.0])).astype(F32)
    info = poseerr.models_info(dict(vertices=v, faces=f))  # numpy, as onboard.load_mesh returns it
    assert tuple(info) == poseerr.INFO_FIELDS and all(type(x) is float for x in info.values())
    assert F32(info["diameter"]) == NR.diameter(v) and abs(info["diameter"] - 120.0) < 1e-3
    lo, hi = v.min(axis=0), v.max(axis=0)
    assert [info["min_x"], info["min_y"], info["min_z"]] == [float(x) for x in lo]
    assert [info["size_x"], info["size_y"], info["size_z"]] == [float(x) for x in hi - lo]
    assert poseerr.models_info((_t(v, dev), _t(f, dev))) == info


# ------------------------------------------------------------------------------------------------------------ the C entries
def test_adi_refusals_write_nothing(dev):
    pts, est, gt, want = _scene(257, 3)
    V, N, G = 257, 3, 16
    d = {k: _t(a, dev) for k, a in dict(pts=pts, est=est, gt=gt).items()}
    out = torch.full((N + 2 * G,), 77, dtype=torch.int64, device=dev)
    need = _lib.load().sam6d_pose_adi_workspace_bytes(V, N)
    assert need == 24 * N * 2
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(V=V, N=N, inv_unit=1.0 / UNIT, flags=0, ws_ptr=ws.data_ptr() + 8 * G, ws_bytes=need, **nulls):
        p = dict(points=d["pts"].data_ptr(), est=d["est"].data_ptr(), gt=d["gt"].data_ptr(), adi_sum=out.data_ptr() + 8 * G)
        p.update(nulls)
        _lib.call("sam6d_pose_adi", p["points"], V, p["est"], p["gt"], N, inv_unit, flags, p["adi_sum"], ws_ptr, ws_bytes, stream)

    for flags in (0, 1):
        run(flags=flags)
        h, hw = out.cpu().numpy(), ws.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all() and np.array_equal(h[G:-G], want)
        assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()
    before, ws_before = out.clone(), ws.clone()
    cases = [(dict(V=0), "V = 0"), (dict(V=(1 << 20) + 1), "V = 1048577"), (dict(N=0), "N = 0"), (dict(N=1025), "N = 1025"),
             (dict(inv_unit=0.0), "inv_unit"), (dict(inv_unit=-1.0), "inv_unit"), (dict(inv_unit=float("inf")), "inv_unit"),
             (dict(inv_unit=float("nan")), "inv_unit"), (dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(ws_bytes=need - 1), "workspace"),
             (dict(ws_ptr=None), "workspace"), (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned"), (dict(adi_sum=out.data_ptr() + 8 * G + 4), "aligned")]
    cases += [({k: None}, k) for k in ("points", "est", "gt", "adi_sum")]
    for kw, name in cases:
        with pytest.raises(RuntimeError, match=name):
            run(**kw)
    assert torch.equal(out, before) and torch.equal(ws, ws_before)  # a refused call writes nothing


def test_diameter_refusals_and_seeds_out_of_range(dev):
    V, G = 1025, 16
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (V, 3)).astype(F32)
    want = np.array([NR.diameter(pts)], F32).view(np.int32)[0]
    p = _t(pts, dev)
    out = torch.full((1 + 2 * G,), 77, dtype=torch.int32, device=dev)
    need = _lib.load().sam6d_points_diameter_workspace_bytes(V)
    assert need == 8 + 24 * 5
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    seeds = _t(np.array(NR.axis_seeds(pts) + [0, 1], np.int32), dev)

    def run(V=V, seeds=seeds.data_ptr(), n_seeds=8, flags=0, points=p.data_ptr(), diameter=out.data_ptr() + 4 * G, ws_ptr=ws.data_ptr() + 8 * G,
            ws_bytes=need):
        _lib.call("sam6d_points_diameter", points, V, seeds, n_seeds, flags, diameter, ws_ptr, ws_bytes, stream)

    def guards():
        h, hw = out.cpu().numpy(), ws.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all() and (hw[:G] == 77).all() and (hw[-G:] == 77).all()
        return h[G]

    # a seed outside [0, V) is ignored: just outside on either side, alone or beside good ones; the result does not depend on the seeds
    outside = _t(np.array([-1, V, V + 7, -V, 5, V, 9, -1], np.int32), dev)
    none = _t(np.array([-1, V, V + 7, -V, -2, V, V + 1, -1], np.int32), dev)
    for kw in (dict(), dict(flags=1), dict(n_seeds=1), dict(seeds=outside.data_ptr()), dict(seeds=none.data_ptr()), dict(seeds=none.data_ptr(), n_seeds=3)):
        out[G] = 77
        run(**kw)
        assert guards() == want, kw
    before, ws_before = out.clone(), ws.clone()
    for kw, name in ((dict(V=0), "V = 0"), (dict(V=(1 << 20) + 1), "V = 1048577"), (dict(n_seeds=0), "n_seeds = 0"), (dict(n_seeds=9), "n_seeds = 9"),
                     (dict(flags=2), "flags"), (dict(points=None), "points"), (dict(seeds=None), "seeds"), (dict(diameter=None), "diameter"),
                     (dict(ws_ptr=None), "workspace"), (dict(ws_bytes=need - 1), "workspace"), (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned")):
        with pytest.raises(RuntimeError, match=name):
            run(**kw)
    assert torch.equal(out, before) and torch.equal(ws, ws_before)  # a refused call writes nothing
