"""All-pairs pose errors, matching and pose NMS on the device (sam6d_hip.posematch over csrc/posematch.hip) against their numpy
restatement (tests/posematch_ref.py: the pair errors are poseerr_ref's point_errors on the expanded pair list).  Every comparison is
bit for bit (a NaN equals a NaN), the pair-error matrix also equals poseerr.pose_errors on the expanded pair list on the device, and
every output of a raw call lies between guard words.  The matching and NMS recipes are the package's own; nothing here is checked
against bop_toolkit, which the suite does not have."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import poseerr_ref as PR
from tests import posematch_ref as MR
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr, posematch

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN = float("nan")
INTR = (600.0, 590.0, 320.0, 240.0)
UNIT = 2.0
G, FILL = 16, 77  # guard words on each side of every output, and what they hold
FLIP = np.concatenate([VR.rotation((0, 0, 1), math.pi), [[0.1], [0.0], [0.0]]], axis=1)
RING = dict(axis=(0, 1, 0), offset=(0.05, 0, 0.02))
PAIR_OUT = dict(mssd=torch.float32, mspd=torch.float32, mssd_sym=torch.int32, mspd_sym=torch.int32, n_skipped=torch.int32, add_sum=torch.int64)
NO_K = ("mssd", "mssd_sym", "add_sum")  # what a call without intrinsics writes


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Guarded:
    """named outputs between guard words"""

    def __init__(self, dev, sizes):
        self.sizes = sizes
        self.buf = {k: torch.full((n + 2 * G,), FILL, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
        self.ptr = {k: b.data_ptr() + G * b.element_size() for k, b in self.buf.items()}

    def read(self, untouched=()):
        """the outputs, after a look at every guard word; those named in `untouched` must still hold the fill"""
        out = {}
        for k, b in self.buf.items():
            h = b.cpu().numpy()
            assert (h[:G] == FILL).all() and (h[-G:] == FILL).all(), k
            assert k not in untouched or (h == FILL).all(), k
            out[k] = h[G:-G]
        return out


# ------------------------------------------------------------------------------------------------------------ pair errors
def _syms(S):
    if S == 1:
        return poseerr.symmetry_transforms()
    if S == 2:
        return poseerr.symmetry_transforms(discrete=[FLIP])
    if S % 2:
        return poseerr.symmetry_transforms(continuous=[RING], max_step=math.pi / S)
    return poseerr.symmetry_transforms(discrete=[FLIP], continuous=[RING], max_step=2 * math.pi / S)


@functools.lru_cache(maxsize=None)
def _scene(V, A, B, S, seed=0):
    """V points in the unit cube, B poses five to eight units away, A poses near them (a[i] near b[i % B]), S symmetries"""
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    b = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(B)])
    a = np.stack([VR.pose(b[i % B][:, 3].astype(F64) + g.normal(size=3) * 0.2, axis=g.normal(size=3), angle=g.uniform(0, 3)) for i in range(A)])
    syms = _syms(S)
    assert syms.shape == (S, 3, 4)
    return pts, a, b, syms


def _raw_pair(dev, pts, a, b, syms, intr=INTR, unit=UNIT):
    """sam6d_pose_pair_errors through ctypes, every output and the workspace between guard words -> dict of (A,B) arrays"""
    A, B, S = len(a), len(b), len(syms)
    d = [_t(np.asarray(x, F32), dev) for x in (pts, a, b, syms)]
    out = Guarded(dev, {k: (A * B, dt) for k, dt in PAIR_OUT.items()})
    need = _lib.load().sam6d_pose_pair_errors_workspace_bytes(A, B, S)
    assert need == 8 * A * B * S
    ws = Guarded(dev, dict(ws=(need // 8, torch.int64)))
    _lib.call("sam6d_pose_pair_errors", d[0].data_ptr(), len(pts), d[1].data_ptr(), A, d[2].data_ptr(), B, d[3].data_ptr(), S,
              *(intr or (0.0, 0.0, 0.0, 0.0)), float(F32(1.0 / unit)), 0 if intr else posematch.NO_MSPD,
              *(out.ptr[k] for k in ("mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")), ws.ptr["ws"], need,
              torch.cuda.current_stream().cuda_stream)
    ws.read()
    got = out.read(untouched=() if intr else tuple(k for k in PAIR_OUT if k not in NO_K))
    return {k: v.reshape(A, B) for k, v in got.items()}


def _expanded_on_device(dev, pts, a, b, syms, unit=UNIT):
    """poseerr.pose_errors on the expanded pair list, 1024 pairs a call -> dict of (A,B) arrays"""
    est, gt = MR.expand(a, b)
    P, sy = _t(pts, dev), _t(syms, dev)
    parts = []
    for k in range(0, len(est), 1024):
        e, g = est[k:k + 1024], gt[k:k + 1024]
        parts.append(poseerr.pose_errors(P, _t(e[:, :, :3], dev), _t(e[:, :, 3], dev), _t(g[:, :, :3], dev), _t(g[:, :, 3], dev), INTR, syms=sy, unit=unit))
    return {k: torch.cat([getattr(p, k) for p in parts]).cpu().numpy().reshape(len(a), len(b)) for k in PAIR_OUT}


def _same(got, want, keys=tuple(PAIR_OUT)):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=got[k].dtype == F32), (k, got[k], want[k])


def _check_pair(dev, pts, a, b, syms):
    """with K against the restatement and against pose_errors on the device; without K the MSSD half has the same bits"""
    want = MR.pair_errors(pts, a, b, syms, INTR, F32(1.0 / UNIT))
    got = _raw_pair(dev, pts, a, b, syms)
    _same(got, want)
    _same(got, _expanded_on_device(dev, pts, a, b, syms))
    _same(_raw_pair(dev, pts, a, b, syms, intr=None), want, NO_K)
    return want


@pytest.mark.parametrize("V", [1, 1023, 1025, 4097])
def test_pair_chunk_edges(dev, V):
    """the edges of the 1024-point chunk, with a shape and its transpose (a transposed index cannot pass both)"""
    w = _check_pair(dev, *_scene(V, 3, 5, 1))
    assert (w["mssd"] > 0).all() and (w["mspd"] > 0).all() and (w["add_sum"] > 0).all() and not w["n_skipped"].any()
    _check_pair(dev, *_scene(V, 5, 3, 2))


@pytest.mark.parametrize("A,B,S", [(1, 1, 1), (3, 5, 1), (5, 3, 2), (2, 43, 3), (2, 1, 129), (1, 128, 1)])
def test_pair_shapes(dev, A, B, S):
    """one triple; non-square; 129 matrices, one beyond the LDS tile of 128, as B S and as S alone; exactly one tile"""
    w = _check_pair(dev, *_scene(65, A, B, S))
    assert len(np.unique(w["mssd"])) == A * B  # every pair has an error of its own: a wrong (i, j) cannot hide
    if S == 129:
        assert w["mssd_sym"].max() > 0


@pytest.mark.parametrize("A,B", [(1024, 1), (1, 1024)])
def test_pair_the_limits_of_a_and_b(dev, A, B):
    _check_pair(dev, *_scene(64, A, B, 1))


@pytest.mark.parametrize("B,S", [(3, 43), (3, 100)])
def test_pair_the_split_over_blockidx_z_does_not_change_a_bit(dev, B, S):
    """V = 1025 is two chunks.  A = 1: two workgroups per run of matrices, so the 129 (300) matrices are dealt to 17 (38) values of
    blockIdx.z in runs of 8.  A = 1024 with every a[i] the same pose: 2048 workgroups already; 129 matrices are one run, blockIdx.z is 0
    alone and one workgroup walks them all, across the LDS tile of 128; 300 matrices are cut by the longest run of 256 (two whole tiles)
    into two.  Every row of the second call has the bits of the first (include/sam6d_hip.h: the split follows from the sizes alone)."""
    pts, a, b, syms = _scene(1025, 1, B, S)
    want = _check_pair(dev, pts, a, b, syms)
    for intr in (INTR, None):
        got = _raw_pair(dev, pts, np.repeat(a, 1024, axis=0), b, syms, intr=intr)
        for k in (PAIR_OUT if intr else NO_K):
            assert np.array_equal(got[k], np.repeat(want[k], 1024, axis=0)), k


def test_pair_equal_poses_are_exactly_zero(dev):
    pts, _, b, syms = _scene(257, 1, 4, 1)
    w = _check_pair(dev, pts, b, b, syms)
    for k in PAIR_OUT:
        assert not np.diag(w[k]).any(), k
    off = ~np.eye(4, dtype=bool)
    assert (w["mssd"][off] > 0).all() and (w["add_sum"][off] > 0).all()


def test_pair_a_point_behind_the_camera_under_one_side(dev):
    """a[0] puts vertex 40 behind the camera, no b does: row 0 counts one skipped point, row 1 none, and MSPD leaves the vertex out"""
    pts, _, _, syms = _scene(65, 1, 1, 2)
    pts = pts.copy()
    pts[40] = [0.0, 0.0, -6.5]
    a = np.stack([VR.pose((0.1, 0.0, 6.0), axis=(1.0, 0.0, 0.0), angle=0.05), VR.pose((0.1, 0.0, 12.0), axis=(1.0, 0.0, 0.0), angle=0.05)])
    b = np.stack([VR.pose((0.0, 0.1, 10.0), angle=0.0), VR.pose((0.2, 0.1, 13.0), angle=0.1), VR.pose((0.0, 0.0, 11.0), angle=0.3)])
    w = _check_pair(dev, pts, a, b, syms)
    assert w["n_skipped"].tolist() == [[1, 1, 1], [0, 0, 0]]
    without = MR.pair_errors(np.delete(pts, 40, axis=0), a, b, syms, INTR, F32(1.0 / UNIT))
    assert np.array_equal(w["mspd"][0], without["mspd"][0]) and (w["add_sum"][0] > without["add_sum"][0]).all()


def test_pair_a_nan_pose_in_one_row_and_one_column(dev):
    pts, a, b, syms = _scene(65, 3, 4, 2)
    a, b = a.copy(), b.copy()
    a[1, 0, 1], b[2, 1, 3] = NAN, NAN
    w = _check_pair(dev, pts, a, b, syms)
    bad = np.zeros((3, 4), bool)
    bad[1, :], bad[:, 2] = True, True
    assert np.array_equal(np.isnan(w["mssd"]), bad) and (w["add_sum"][bad] == 65 * 2 ** 42).all() and (w["add_sum"][~bad] < 65 * 2 ** 34).all()
    assert (w["n_skipped"][~bad] == 0).all() and np.isfinite(w["mspd"][~bad]).all()


def test_pair_identical_symmetries_the_lower_index_wins(dev):
    pts, _, b, _ = _scene(65, 1, 3, 1)
    ring = poseerr.symmetry_transforms(continuous=[RING], max_step=math.pi / 5)
    syms = np.stack([ring[2], ring[1], ring[1], ring[3], ring[1]])
    a = PR.sym_gt(b, ring[1:2])[:, 0].copy()
    a[:, :, 3] += F32(0.01)  # a[i] near b[i] o ring[1]: that symmetry is the best on the diagonal, at indices 1, 2 and 4
    w = _check_pair(dev, pts, a, b, syms)
    assert np.diag(w["mssd_sym"]).tolist() == [1, 1, 1] and np.diag(w["mspd_sym"]).tolist() == [1, 1, 1] and (w["mssd"] > 0).all()


def test_pair_errors_python_entry(dev):
    pts, a, b, syms = _scene(1025, 3, 5, 2)
    want = MR.pair_errors(pts, a, b, syms, INTR, F32(1.0 / UNIT))
    args = [_t(x, dev) for x in (pts, a[:, :, :3], a[:, :, 3], b[:, :, :3], b[:, :, 3])]
    got = posematch.pair_errors(*args, K=INTR, syms=syms, unit=UNIT)  # (a host array of symmetries is uploaded)
    for k, dt in PAIR_OUT.items():
        t = getattr(got, k)
        assert t.dtype == dt and tuple(t.shape) == (3, 5) and np.array_equal(t.cpu().numpy(), want[k]), k
    add = PR.add_of(want["add_sum"], F32(1.0 / UNIT), len(pts))
    assert got.add.dtype == torch.float32 and np.array_equal(got.add.cpu().numpy(), add)
    bare = posematch.pair_errors(*args, syms=_t(syms, dev), unit=UNIT)
    assert bare.mspd is None and bare.mspd_sym is None and bare.n_skipped is None
    assert all(np.array_equal(getattr(bare, k).cpu().numpy(), want[k]) for k in NO_K) and np.array_equal(bare.add.cpu().numpy(), add)


def test_pose_errors_are_the_diagonal_of_pair_errors(dev):
    """V = 1025 is two chunks, S = 129 two LDS tiles, and runs of 8 matrices end inside a tile: every field of pose_errors(a, b) is
    the diagonal of pair_errors(a, b) and the restatement's, n_skipped and add_sum included.  Pose 1 has one vertex behind the camera
    under the estimate (as test_poseerr_gpu's test_a_point_behind_the_camera has it)"""
    pts, a, b, syms = _scene(1025, 3, 3, 129)
    pts, a, b = pts.copy(), a.copy(), b.copy()
    pts[40] = [0.0, 0.0, -6.5]
    a[[0, 2], 2, 3] += F32(6.0)  # the other poses: far enough for every vertex
    b[[0, 2], 2, 3] += F32(6.0)
    a[1], b[1] = VR.pose((0.1, 0.0, 6.0), axis=(1.0, 0.0, 0.0), angle=0.05), VR.pose((0.0, 0.1, 10.0), angle=0.0)
    want = PR.point_errors(pts, a, b, syms, INTR, F32(1.0 / UNIT))
    assert want["n_skipped"].tolist() == [0, 1, 0]  # a skip cannot hide a failure
    assert np.isfinite(want["mssd"]).all() and np.isfinite(want["mspd"]).all() and want["mssd_sym"].max() > 0
    want["add"] = PR.add_of(want["add_sum"], F32(1.0 / UNIT), len(pts))
    args = [_t(x, dev) for x in (pts, a[:, :, :3], a[:, :, 3], b[:, :, :3], b[:, :, 3])]
    pose = poseerr.pose_errors(*args, INTR, syms=_t(syms, dev), unit=UNIT)
    pair = posematch.pair_errors(*args, K=INTR, syms=_t(syms, dev), unit=UNIT)
    for k, dt in dict(PAIR_OUT, add=torch.float32).items():
        p, q = getattr(pose, k), getattr(pair, k)
        assert p.dtype == q.dtype == dt and tuple(p.shape) == (3,) and tuple(q.shape) == (3, 3), k
        assert np.array_equal(p.cpu().numpy(), want[k]) and torch.equal(q.diagonal(), p), (k, p.cpu().numpy(), q.cpu().numpy(), want[k])


# ------------------------------------------------------------------------------------------------------------ matching
POOL = np.array([0.0, -0.0, 0.125, 0.25, 0.25, 0.5, 0.75, 1.0, 2.0, -1.0, np.inf, NAN], F32)


def _lumpy(g, shape, pool=POOL):
    return pool[g.integers(0, len(pool), shape)]


def _raw_match(dev, err, scores, thr, valid=None, max_ests=0):
    A, B, T = err.shape[0], err.shape[1], len(thr)
    d = [_t(np.asarray(err, F32), dev), _t(np.asarray(scores, F32), dev), _t(np.asarray(thr, F32), dev)]
    v = None if valid is None else _t(np.asarray(valid, bool), dev)
    out = Guarded(dev, dict(est_match=(T * A, torch.int32), gt_match=(T * B, torch.int32), n_matched=(T, torch.int32)))
    need = _lib.load().sam6d_pose_match_workspace_bytes(A)
    ws = Guarded(dev, dict(ws=(need // 4, torch.int32)))
    _lib.call("sam6d_pose_match", d[0].data_ptr(), A, B, d[1].data_ptr(), d[2].data_ptr(), T, None if v is None else v.data_ptr(), max_ests,
              out.ptr["est_match"], out.ptr["gt_match"], out.ptr["n_matched"], ws.ptr["ws"], need, torch.cuda.current_stream().cuda_stream)
    order = ws.read()["ws"][:A]
    assert order.tolist() == MR.order(scores)
    got = out.read()
    return got["est_match"].reshape(T, A), got["gt_match"].reshape(T, B), got["n_matched"]


def _check_match(dev, err, scores, thr, valid=None, max_ests=0):
    want = MR.match(err, scores, thr, valid, max_ests)
    for g, w in zip(_raw_match(dev, err, scores, thr, valid, max_ests), want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (g, w)
    return want


@pytest.mark.parametrize("A,B,T", [(1, 1, 1), (7, 3, 2), (3, 7, 2), (1024, 65, 64), (65, 1024, 1)])
def test_match_shapes(dev, A, B, T):
    """errors and scores from a small pool: equal scores, equal errors, err == thr, -0 beside 0, NaN and infinity in every case"""
    g = np.random.default_rng(A * 7 + B)
    thr = np.resize(np.array([0.25, 1.0, np.inf, 0.125, 0.5, 0.0, NAN, 2.0], F32), T)
    for valid, max_ests in ((None, 0), (g.random(B) < 0.7, 0), (None, max(1, A // 2))):
        want = _check_match(dev, _lumpy(g, (A, B)), _lumpy(g, A), thr, valid, max_ests)
        if A >= 64 and valid is None:
            assert want[2].max() == min(A if max_ests == 0 else max_ests, B)
        if T == 64:
            assert want[2][6] == 0 and want[2][5] > 0  # a NaN threshold matches nothing, 0 the negative errors
    # and errors all different: the nearest free target, not the first
    err = g.permutation(A * B).reshape(A, B).astype(F32) / F32(A * B)
    want = _check_match(dev, err, g.random(A).astype(F32), np.resize(np.array([0.5, 2.0, 0.01], F32), T))
    assert want[2].max() == min(A, B) or T == 1


def test_match_rules(dev):
    """the cases of test_posematch_host.test_matching_rules on the device: ties of both kinds, err == thr, a NaN error, one valid
    target, and max_ests cutting the order in the middle of a tie"""
    err = np.array([[0.3, 0.3, 0.1], [0.1, 0.3, 0.1], [0.2, NAN, 0.05]], F32)
    scores = np.array([0.9, 0.9, 0.5], F32)
    est, gt, n = _check_match(dev, err, scores, [1.0, 0.3, 0.1, 0.05])
    assert est.tolist() == [[2, 0, -1], [2, 0, -1], [-1, -1, 2], [-1, -1, -1]] and n.tolist() == [2, 2, 1, 0]
    assert _check_match(dev, err, scores, [1.0], max_ests=1)[0].tolist() == [[2, -1, -1]]
    assert _check_match(dev, err, scores, [1.0], valid=[False, True, False])[1].tolist() == [[-1, 0, -1]]
    # 1024 equal scores, max_ests in their middle: the first 500 indices take part, each takes its own column's neighbour
    err = np.full((1024, 600), 0.5, F32)
    want = _check_match(dev, err, np.ones(1024, F32), [0.75], max_ests=500)
    assert want[0][0, :500].tolist() == list(range(500)) and (want[0][0, 500:] == -1).all() and want[2].tolist() == [500]
    one = np.zeros(1024, bool)
    one[777] = True
    want = _check_match(dev, _lumpy(np.random.default_rng(5), (65, 1024)), np.arange(65, dtype=F32), [np.inf], valid=one)
    assert want[2].tolist() == [1] and (want[1][0] >= 0).sum() == 1 and want[1][0, 777] >= 0


def test_match_poses_python_entry(dev):
    g = np.random.default_rng(9)
    err, scores = _lumpy(g, (7, 5)), _lumpy(g, 7)
    valid = np.array([True, False, True, True, False])
    got = posematch.match_poses(_t(err, dev), _t(scores, dev), [0.25, 1.0], valid=_t(valid, dev), max_ests=4)
    want = MR.match(err, scores, [0.25, 1.0], valid, 4)
    for t, w in zip((got.est_match, got.gt_match, got.n_matched), want):
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), w)
    assert got.n_targets == 3
    assert posematch.instance_recall(got.n_matched, got.n_targets).tolist() == [float(F32(n) / F32(3)) for n in want[2]]
    for e, v, shape in ((err, np.zeros(5, bool), (7, 5)), (err[:, :0], None, (7, 0)), (err[:0], None, (0, 5))):  # no launch
        got = posematch.match_poses(_t(e, dev), _t(scores[:shape[0]], dev), torch.tensor([0.25, 1.0]), valid=_t(v, dev))
        assert got.est_match.shape == (2, shape[0]) and got.gt_match.shape == (2, shape[1]) and got.est_match.dtype == torch.int32
        assert (got.est_match == -1).all() and (got.gt_match == -1).all() and got.n_matched.tolist() == [0, 0]
        assert got.n_targets == (0 if shape != (0, 5) else 5)
    assert torch.isnan(posematch.instance_recall(got.n_matched, 0)).all()


# ------------------------------------------------------------------------------------------------------------ NMS
def _raw_nms(dev, err, scores, thresh):
    N = len(scores)
    d = [_t(np.asarray(err, F32), dev), _t(np.asarray(scores, F32), dev)]
    out = Guarded(dev, dict(keep_idx=(N, torch.int64), count=(1, torch.int32), suppressed_by=(N, torch.int32)))
    need = _lib.load().sam6d_pose_nms_workspace_bytes(N)
    ws = Guarded(dev, dict(ws=(need // 8, torch.int64)))
    _lib.call("sam6d_pose_nms", d[0].data_ptr(), d[1].data_ptr(), N, float(thresh), out.ptr["keep_idx"], out.ptr["count"], out.ptr["suppressed_by"],
              ws.ptr["ws"], need, torch.cuda.current_stream().cuda_stream)
    ws.read()
    got = out.read()
    return got["keep_idx"], got["count"], got["suppressed_by"]


def _check_nms(dev, err, scores, thresh):
    want = MR.nms(err, scores, thresh)
    for g, w in zip(_raw_nms(dev, err, scores, thresh), want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (g, w)
    return want


@pytest.mark.parametrize("N", [1, 2, 64, 65, 1024])
def test_nms_mask_word_edges(dev, N):
    """matrices that are not symmetric, from a small pool (thresh equal to an entry; NaN; ties in the scores), then a sparse one in
    which most poses are kept, then all poses identical: one is kept"""
    g = np.random.default_rng(N)
    for thresh in (0.25, 1.0):
        _check_nms(dev, _lumpy(g, (N, N)), _lumpy(g, N), thresh)
    err = g.random((N, N)).astype(F32)
    keep_idx, count, by = _check_nms(dev, err, g.random(N).astype(F32), 2.0 / N)
    assert N < 64 or N // 4 < count[0] < N
    keep_idx, count, by = _check_nms(dev, np.zeros((N, N), F32), np.ones(N, F32), 1e-6)
    assert count.tolist() == [1] and keep_idx[0] == 0 and not by.any()
    keep_idx, count, by = _check_nms(dev, err, -np.arange(N, dtype=F32), 0.0)  # nothing is below 0: all kept, in order
    assert keep_idx.tolist() == list(range(N)) and by.tolist() == list(range(N))


def test_nms_rules(dev):
    """the chain that defines greedy, the asymmetric matrix, thresh equal to an entry, a NaN on the diagonal"""
    err = np.array([[0, 0.1, 0.9], [0.1, 0, 0.1], [0.9, 0.1, 0]], F32)
    keep_idx, count, by = _check_nms(dev, err, [3.0, 2.0, 1.0], 0.5)
    assert keep_idx.tolist() == [0, 2, -1] and count.tolist() == [2] and by.tolist() == [0, 0, 2]
    err = np.array([[0, 0.9], [0.1, 0]], F32)
    assert _check_nms(dev, err, [2.0, 1.0], 0.5)[0].tolist() == [0, 1] and _check_nms(dev, err, [1.0, 2.0], 0.5)[2].tolist() == [1, 1]
    err = np.array([[NAN, 0.5], [0.5, NAN]], F32)
    assert _check_nms(dev, err, [2.0, 1.0], 0.5)[1].tolist() == [2] and _check_nms(dev, err, [2.0, 1.0], np.nextafter(F32(0.5), F32(1)))[1].tolist() == [1]


def test_nms_python_entries(dev):
    """pose_nms, and nms_poses = pair_errors of the set with itself, then pose_nms: three clusters of near-duplicates"""
    pts, _, b, _ = _scene(257, 1, 3, 1)
    g = np.random.default_rng(2)
    poses = np.repeat(b, 4, axis=0).copy()
    poses[:, :, 3] += (g.normal(size=(12, 3)) * 0.002).astype(F32)
    scores = g.random(12).astype(F32)
    R, t = _t(poses[:, :, :3], dev), _t(poses[:, :, 3], dev)
    got, mssd = posematch.nms_poses(_t(pts, dev), R, t, _t(scores, dev), 0.05, syms=_syms(2))
    w = MR.pair_errors(pts, poses, poses, _syms(2), INTR, F32(1.0))
    assert np.array_equal(mssd.cpu().numpy(), w["mssd"])
    want = MR.nms(w["mssd"], scores, 0.05)
    for x, y in zip((got.keep_idx, got.count, got.suppressed_by), want):
        assert np.array_equal(x.cpu().numpy(), y)
    best = [4 * c + int(np.argmax(scores[4 * c:4 * c + 4])) for c in range(3)]
    assert sorted(got.kept().tolist()) == sorted(best) and got.suppressed_by.tolist() == [best[i // 4] for i in range(12)]
    again = posematch.pose_nms(mssd, _t(scores, dev), 0.05)
    assert torch.equal(again.keep_idx, got.keep_idx) and again.keep_idx.dtype == torch.int64
    none = posematch.pose_nms(torch.zeros((0, 0), device=dev), torch.zeros((0,), device=dev), 0.05)
    assert none.keep_idx.numel() == 0 and none.count.tolist() == [0] and none.kept().numel() == 0


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    """argument checks through ctypes: each returns non-zero with a message that names the argument, and no output, guard or
    workspace word changes"""
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    pts, a, b, syms = _scene(65, 3, 4, 2)
    d = {k: _t(x, dev) for k, x in dict(points=pts, a=a, b=b, syms=syms).items()}
    out = Guarded(dev, {k: (1024, dt) for k, dt in PAIR_OUT.items()})
    ws = Guarded(dev, dict(ws=(1024, torch.int64)))

    def pair(V=65, A=3, B=4, S=2, inv_unit=0.5, flags=0, ws_ptr=ws.ptr["ws"], ws_bytes=None, **nulls):
        p = dict({k: v.data_ptr() for k, v in d.items()}, **out.ptr)
        p.update(nulls)
        need = lib.sam6d_pose_pair_errors_workspace_bytes(3, 4, 2)
        _lib.call("sam6d_pose_pair_errors", p["points"], V, p["a"], A, p["b"], B, p["syms"], S, *INTR, inv_unit, flags, p["mssd"], p["mspd"],
                  p["mssd_sym"], p["mspd_sym"], p["n_skipped"], p["add_sum"], ws_ptr, need if ws_bytes is None else ws_bytes, stream)

    cases = [(dict(V=0), "V = 0"), (dict(V=(1 << 20) + 1), "V = 1048577"), (dict(A=0), "A = 0"), (dict(A=1025), "A = 1025"), (dict(B=0), "B = 0"),
             (dict(B=1025), "B = 1025"), (dict(S=0), "S = 0"), (dict(S=1025), "S = 1025"), (dict(A=1024, B=1024, S=5, ws_bytes=1 << 40), "A B S = 5242880"),
             (dict(A=64, B=64, S=1024, ws_bytes=(32 << 20) - 8), "workspace"), (dict(inv_unit=0.0), "inv_unit"), (dict(inv_unit=NAN), "inv_unit"),
             (dict(flags=2), "flags"), (dict(ws_bytes=8 * 24 - 1), "workspace"), (dict(ws_ptr=None), "workspace"), (dict(ws_ptr=ws.ptr["ws"] + 4), "aligned")]
    null = " %s is a null pointer"
    cases += [({k: None}, null % k) for k in ("points", "a", "b", "syms", "mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")]
    cases += [(dict(flags=1, mssd=None), null % "mssd"), (dict(flags=1, add_sum=None), null % "add_sum")]
    for kw, name in cases:
        with pytest.raises(RuntimeError, match=name):
            pair(**kw)

    err, scores, thr = (torch.zeros((8, 8), device=dev), torch.zeros(8, device=dev), torch.ones(2, device=dev))
    mout = Guarded(dev, dict(est_match=(64, torch.int32), gt_match=(64, torch.int32), n_matched=(64, torch.int32)))
    nout = Guarded(dev, dict(keep_idx=(8, torch.int64), count=(1, torch.int32), suppressed_by=(8, torch.int32)))

    def match(A=8, B=8, T=2, max_ests=0, ws_ptr=ws.ptr["ws"], ws_bytes=32, **nulls):
        p = dict(dict(err=err.data_ptr(), scores=scores.data_ptr(), thr=thr.data_ptr()), **mout.ptr)
        p.update(nulls)
        _lib.call("sam6d_pose_match", p["err"], A, B, p["scores"], p["thr"], T, None, max_ests, p["est_match"], p["gt_match"], p["n_matched"], ws_ptr,
                  ws_bytes, stream)

    def nms(N=8, ws_ptr=ws.ptr["ws"], ws_bytes=32 + 64, **nulls):
        p = dict(dict(err=err.data_ptr(), scores=scores.data_ptr()), **nout.ptr)
        p.update(nulls)
        _lib.call("sam6d_pose_nms", p["err"], p["scores"], N, 0.5, p["keep_idx"], p["count"], p["suppressed_by"], ws_ptr, ws_bytes, stream)

    for kw, name in [(dict(A=0), "A = 0"), (dict(A=1025), "A = 1025"), (dict(B=0), "B = 0"), (dict(B=1025), "B = 1025"), (dict(T=0), "T = 0"),
                     (dict(T=65), "T = 65"), (dict(max_ests=-1), "max_ests"), (dict(ws_bytes=31), "workspace"), (dict(ws_ptr=None), "workspace"),
                     (dict(ws_ptr=ws.ptr["ws"] + 2), "aligned")] + [({k: None}, null % k) for k in ("err", "scores", "thr", "est_match", "gt_match", "n_matched")]:
        with pytest.raises(RuntimeError, match=name):
            match(**kw)
    for kw, name in [(dict(N=0), "N = 0"), (dict(N=1025), "N = 1025"), (dict(ws_bytes=95), "workspace"), (dict(ws_ptr=None), "workspace"),
                     (dict(ws_ptr=ws.ptr["ws"] + 4), "aligned"), (dict(keep_idx=nout.ptr["keep_idx"] + 4), "aligned")] \
            + [({k: None}, null % k) for k in ("err", "scores", "keep_idx", "count", "suppressed_by")]:
        with pytest.raises(RuntimeError, match=name):
            nms(**kw)
    for bufs in (out, mout, nout, ws):
        bufs.read(untouched=tuple(bufs.buf))  # a refused call writes nothing
    pair(flags=1, mspd=None, mspd_sym=None, n_skipped=None)  # and without MSPD its three outputs may be null
    got = out.read(untouched=("mspd", "mspd_sym", "n_skipped"))
    want = MR.pair_errors(pts, a, b, syms, INTR, 0.5)
    assert all(np.array_equal(got[k][:12].reshape(3, 4), want[k]) and (got[k][12:] == FILL).all() for k in NO_K)
