"""All-pairs ADI with its cap on the device (sam6d_hip.posematch.pair_adi / nms_poses_adi over csrc/pairadi.hip) against the numpy
restatement (tests/pair_adi_ref.py).  Every comparison is bit for bit: adi_sum, lower_sum, skipped and the bits of adi, with and
without a cap, pruned and not, sorted and not.  The inputs are those tests/test_pair_adi_host.py shows to give both skipped and
computed pairs under each cap.  Nothing here is checked against bop_toolkit, which the suite does not have."""
import numpy as np
import pytest
import torch

from tests import pair_adi_ref as AR
from tests import posematch_ref as MR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr, posematch

pytestmark = pytest.mark.gpu

F32 = np.float32
ROUTES = [dict(sort=s, prune=p) for s in (True, False) for p in (True, False)]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poses(dev, M):
    M = np.asarray(M, F32)
    return _t(M[:, :, :3], dev), _t(M[:, :, 3], dev)


def _pair_adi(dev, pts, a, b, **kw):
    """pair_adi for the view matrices a, b (scale 1: R * 1.0f is R)"""
    return posematch.pair_adi(_t(pts, dev), *_poses(dev, a), *_poses(dev, b), unit=AR.UNIT, **kw)


def _device_order(dev, pts):
    """the order pair_adi(sort=True) searches in; the restatement's lower_sum is formed over the same tiles"""
    return poseerr.morton_order(_t(pts, dev)).cpu().numpy()


def _scene_lower(dev, V, A, B, sort):
    pts, a, b, _ = AR.scene(V, A, B)
    if not sort:
        return AR.scene_lower(V, A, B, False)
    order = _device_order(dev, pts)
    if np.array_equal(order, AR.morton_order(pts)):
        return AR.scene_lower(V, A, B, True)
    return AR.pair_lower_sum(pts, a, b, AR.INV_UNIT, order)


def _same(dev, got, want):
    assert got.adi_sum.dtype == torch.int64 and got.skipped.dtype == torch.bool and got.adi.dtype == torch.float32
    assert torch.equal(got.skipped, _t(want["skipped"], dev)), (got.skipped.cpu().numpy(), want["skipped"])
    assert torch.equal(got.adi_sum, _t(want["adi_sum"], dev)), (got.adi_sum.cpu().numpy(), want["adi_sum"])
    if want["lower_sum"] is None:
        assert got.lower_sum is None
    else:
        assert got.lower_sum.dtype == torch.int64
        assert torch.equal(got.lower_sum, _t(want["lower_sum"], dev)), (got.lower_sum.cpu().numpy(), want["lower_sum"])
    assert torch.equal(got.adi.view(torch.int32), _t(want["adi"].view(np.int32), dev))


def _check_scene(dev, V, A, B):
    """every cap under every route against the restatement; the computed entries are the full table's in every combination"""
    pts, a, b, full = AR.scene(V, A, B)
    for route in ROUTES:
        lower = _scene_lower(dev, V, A, B, route["sort"])
        for cap in (None,) + AR.CAPS:
            want = AR.capped(full, lower, cap, AR.INV_UNIT, V)
            got = _pair_adi(dev, pts, a, b, cap=cap, **route)
            assert tuple(got.adi.shape) == (A, B)
            _same(dev, got, want)
            keep = ~want["skipped"]
            assert np.array_equal(got.adi_sum.cpu().numpy()[keep], full[keep])


@pytest.mark.parametrize("V", [1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_tile_and_chunk_edges(dev, V):
    _check_scene(dev, V, 3, 5)


@pytest.mark.parametrize("A, B", [(1, 1), (3, 5), (5, 3), (33, 2)])
def test_shapes(dev, A, B):
    _check_scene(dev, 257, A, B)


def test_computed_entries_are_the_pair_by_pair_entry(dev):
    """every pair that is not skipped: poseerr.adi on the expanded pair, bit for bit in adi_sum and adi"""
    V, A, B = 1025, 3, 5
    pts, a, b, full = AR.scene(V, A, B)
    est, gt = MR.expand(a, b)
    listed = poseerr.adi(_t(pts, dev), *_poses(dev, est), *_poses(dev, gt), unit=AR.UNIT)
    assert torch.equal(listed.adi_sum.reshape(A, B), _t(full, dev))
    for cap in (None,) + AR.CAPS:
        got = _pair_adi(dev, pts, a, b, cap=cap)
        keep = ~got.skipped
        assert bool(keep.any()) and (cap is None or bool(got.skipped.any()))
        assert torch.equal(got.adi_sum[keep], listed.adi_sum.reshape(A, B)[keep])
        assert torch.equal(got.adi[keep].view(torch.int32), listed.adi.reshape(A, B)[keep].view(torch.int32))
        assert bool((got.adi_sum[got.skipped] == -1).all()) and bool(torch.isposinf(got.adi[got.skipped]).all())


def _nms_same(dev, got, want):
    keep, count, by = want
    assert torch.equal(got.keep_idx, _t(keep, dev)) and torch.equal(got.count, _t(count, dev)) and torch.equal(got.suppressed_by, _t(by, dev))


def test_nms_poses_adi(dev):
    pts, poses, scores = AR.nms_scene()
    V = len(pts)
    order = _device_order(dev, pts)
    uncapped = _pair_adi(dev, pts, poses, poses).adi
    assert torch.equal(uncapped.view(torch.int32), _t(AR.pair_adi(pts, poses, poses, AR.INV_UNIT)["adi"].view(np.int32), dev))
    mid = np.sort(uncapped.cpu().numpy()[~np.eye(len(poses), dtype=bool)])
    n_skipped = 0
    for thresh in (0.0, 0.01, 0.05, 1.0, float(mid[len(mid) // 3]), float(np.nextafter(mid[len(mid) // 3], F32(np.inf)))):
        got, adi = posematch.nms_poses_adi(_t(pts, dev), *_poses(dev, poses), _t(scores, dev), thresh, unit=AR.UNIT)
        want, want_adi = AR.nms_adi(pts, poses, scores, thresh, AR.INV_UNIT, order)
        assert torch.equal(adi.view(torch.int32), _t(want_adi.view(np.int32), dev))
        _nms_same(dev, got, want)
        plain = posematch.pose_nms(uncapped, _t(scores, dev), thresh)
        assert torch.equal(got.keep_idx, plain.keep_idx) and torch.equal(got.count, plain.count) and torch.equal(got.suppressed_by, plain.suppressed_by)
        n_skipped += int(torch.isposinf(adi).sum())
    assert n_skipped > 0


def test_a_cuboid_without_symmetry_annotation(dev):
    """two poses half a turn about the cuboid's axis and one distinct pose: MSSD-NMS without syms keeps three, ADI-NMS two"""
    pts, poses, scores, thresh = AR.cuboid_case()
    by_mssd, _ = posematch.nms_poses(_t(pts, dev), *_poses(dev, poses), _t(scores, dev), thresh)
    by_adi, adi = posematch.nms_poses_adi(_t(pts, dev), *_poses(dev, poses), _t(scores, dev), thresh)
    assert int(by_mssd.count) == 3 and int(by_adi.count) == 2
    assert by_adi.kept().tolist() == [0, 2] and by_adi.suppressed_by.tolist() == [0, 0, 2]
    _nms_same(dev, by_adi, AR.nms_adi(pts, poses, scores, thresh, order=_device_order(dev, pts))[0])


def test_empty_sides_without_a_launch(dev, monkeypatch):
    pts, a, b, _ = AR.scene(257, 3, 5)

    def no_call(*args, **kw):
        raise AssertionError("an empty side must not reach the library")
    monkeypatch.setattr(_lib, "call", no_call)
    for A, B in ((0, 5), (3, 0), (0, 0)):
        for cap in (None, 0.5):
            got = _pair_adi(dev, pts, a[:A], b[:B], cap=cap)
            for x, dtype in ((got.adi, torch.float32), (got.adi_sum, torch.int64), (got.skipped, torch.bool)):
                assert tuple(x.shape) == (A, B) and x.dtype == dtype and x.device.type == "cuda"
            assert (got.lower_sum is None) if cap is None else (tuple(got.lower_sum.shape) == (A, B) and got.lower_sum.dtype == torch.int64)
    got, adi = posematch.nms_poses_adi(_t(pts, dev), *_poses(dev, a[:0]), _t(np.zeros(0, F32), dev), 0.1)
    assert tuple(adi.shape) == (0, 0) and int(got.count) == 0 and got.keep_idx.numel() == 0


def test_guard_words_and_refusals_write_nothing(dev):
    V, A, B, G = 257, 3, 5, 16
    P = A * B
    pts, a, b, full = AR.scene(V, A, B)
    lower = AR.scene_lower(V, A, B, False)
    d = {k: _t(x, dev) for k, x in dict(pts=pts, a=a, b=b).items()}
    need = _lib.load().sam6d_pose_pair_adi_workspace_bytes(V, A, B)
    assert need == 24 * B * 2
    out = {k: torch.full((P + 2 * G,), 77, dtype=torch.int64, device=dev) for k in ("adi_sum", "lower_sum")}
    skipped = torch.full((P + 2 * G,), 77, dtype=torch.uint8, device=dev)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    inv_unit = float(AR.INV_UNIT)

    def run(V=V, A=A, B=B, inv_unit=inv_unit, flags=0, cap_sum=-1, ws_ptr=ws.data_ptr() + 8 * G, ws_bytes=need, **ptrs):
        p = dict(points=d["pts"].data_ptr(), a=d["a"].data_ptr(), b=d["b"].data_ptr(), adi_sum=out["adi_sum"].data_ptr() + 8 * G,
                 lower_sum=out["lower_sum"].data_ptr() + 8 * G, skipped=skipped.data_ptr() + G)
        p.update(ptrs)
        _lib.call("sam6d_pose_pair_adi", p["points"], V, p["a"], A, p["b"], B, inv_unit, flags, cap_sum, p["adi_sum"], p["lower_sum"], p["skipped"],
                  ws_ptr, ws_bytes, stream)

    def guards(x):
        h = x.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all()
        return h[G:-G]

    for flags in (0, 1):
        for cap in AR.CAPS:
            want = AR.capped(full, lower, cap, AR.INV_UNIT, V)
            run(flags=flags, cap_sum=AR.cap_sum(cap, AR.INV_UNIT, V))
            assert np.array_equal(guards(out["adi_sum"]), want["adi_sum"].reshape(-1))
            assert np.array_equal(guards(out["lower_sum"]), lower.reshape(-1))
            assert np.array_equal(guards(skipped), want["skipped"].reshape(-1).astype(np.uint8))
            guards(ws)
        out["lower_sum"].fill_(77)
        run(flags=flags, lower_sum=None)  # no cap: lower_sum may be null, and one that is given is not touched
        run(flags=flags)
        assert np.array_equal(guards(out["adi_sum"]), full.reshape(-1)) and (guards(skipped) == 0).all()
        assert (out["lower_sum"] == 77).all()
        guards(ws)
    before = [x.clone() for x in (out["adi_sum"], out["lower_sum"], skipped, ws)]
    cases = [(dict(V=0), "V = 0"), (dict(V=(1 << 20) + 1), "V = 1048577"), (dict(A=0), "A = 0"), (dict(A=1025), "A = 1025"), (dict(B=0), "B = 0"),
             (dict(B=1025), "B = 1025"), (dict(V=4097, A=1024, B=1024), "1024 x 1024 x 5 is above the cap"),
             (dict(inv_unit=0.0), "inv_unit"), (dict(inv_unit=-1.0), "inv_unit"), (dict(inv_unit=float("inf")), "inv_unit"),
             (dict(inv_unit=float("nan")), "inv_unit"), (dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(ws_bytes=need - 1), "workspace"),
             (dict(ws_ptr=None), "workspace is a null"), (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned"),
             (dict(adi_sum=out["adi_sum"].data_ptr() + 8 * G + 4), "aligned"),
             (dict(cap_sum=5, lower_sum=out["lower_sum"].data_ptr() + 8 * G + 4), "aligned"), (dict(cap_sum=5, lower_sum=None), "lower_sum is a null"),
             (dict(points=None), "points is a null"), (dict(a=None), " a is a null"), (dict(b=None), " b is a null"),
             (dict(adi_sum=None), "adi_sum is a null"), (dict(skipped=None), "skipped is a null")]
    for kw, name in cases:
        for cap_sum in (-1, 1 << 30):
            with pytest.raises(RuntimeError, match=name):
                run(**dict(dict(cap_sum=cap_sum), **kw))
    after = (out["adi_sum"], out["lower_sum"], skipped, ws)
    assert all(torch.equal(x, y) for x, y in zip(after, before))  # a refused call writes nothing
