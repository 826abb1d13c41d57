"""All-pairs pose errors, matching and pose NMS (sam6d_hip.posematch, csrc/posematch.hip): the host side and the numpy restatement
(tests/posematch_ref.py).  No GPU: the binding, the matching and NMS restatements against an independent naive implementation
(sort, then scan, with Python lists, sets and dicts) on seeded small cases, the cases that define the recipes, the pair errors against
float64 within poseerr_ref's bounds, the refusals, and the import without a library.  The recipes are the package's own: nothing here
is checked against bop_toolkit, which the suite does not have."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import poseerr_ref as PR
from tests import posematch_ref as MR
from tests import verify_ref as VR
from tests._util import ROOT
from sam6d_hip import _lib, poseerr, posematch

F32, F64 = np.float32, np.float64
NAN = float("nan")
NAMES = ("sam6d_pose_pair_errors", "sam6d_pose_pair_errors_workspace_bytes", "sam6d_pose_match", "sam6d_pose_match_workspace_bytes",
         "sam6d_pose_nms", "sam6d_pose_nms_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ the binding
def test_new_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sam6d_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared" % name
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert [len(_lib.SIGNATURES[n]) for n in NAMES[::2]] == [23, 14, 10]
    lib = _lib.load()
    assert lib.sam6d_pose_pair_errors_workspace_bytes(3, 5, 2) == 8 * 30
    assert lib.sam6d_pose_pair_errors_workspace_bytes(1024, 1024, 4) == lib.sam6d_pose_pair_errors_workspace_bytes(64, 64, 1024) == 32 << 20
    bad = ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025), (1024, 1024, 5), (2, 2049, 1024))
    assert [lib.sam6d_pose_pair_errors_workspace_bytes(*a) for a in bad] == [0] * len(bad)
    assert [lib.sam6d_pose_match_workspace_bytes(a) for a in (0, 1, 4, 5, 1024, 1025)] == [0, 16, 16, 32, 4096, 0]
    assert [lib.sam6d_pose_nms_workspace_bytes(n) for n in (0, 1, 64, 65, 1024, 1025)] == [0, 16 + 8, 256 + 512, 272 + 65 * 16, 4096 + 1024 * 128, 0]


def test_the_module_imports_without_a_library():
    """SAM6D_LIB names a file that does not exist: the import succeeds, the first launch would raise"""
    code = ("import sys; sys.path.insert(0, %r); from sam6d_hip import posematch, _lib; import os; assert not os.path.exists(_lib.LIB_PATH); "
            "assert _lib._lib is None; print(posematch.MAX_TRIPLES)" % os.path.join(ROOT, "openvino-sam-6d_amd"))
    env = dict(os.environ, SAM6D_LIB=os.path.join(ROOT, "no", "such", "libsam6d_hip.so"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == str(1 << 22), out.stderr


# ------------------------------------------------------------------------------------------------------------ matching and NMS
def _naive_order(scores):
    s = [float(v) for v in np.asarray(scores, F32)]
    return sorted(range(len(s)), key=lambda i: (1, 0.0, i) if math.isnan(s[i]) else (0, -s[i], i))  # (-(-0.0) == 0.0: equal)


def _naive_match(err, scores, thresholds, valid, max_ests):
    """sort, then scan: per threshold a dict target -> estimate and a set of the taken"""
    err = np.asarray(err, F32)
    A, B = err.shape
    walk = _naive_order(scores)
    walk = walk[:max_ests] if max_ests > 0 else walk
    est_rows, gt_rows = [], []
    for thr in np.asarray(thresholds, F32):
        taken = {}
        for i in walk:
            cands = sorted((float(err[i, j]), j) for j in range(B) if (valid is None or valid[j]) and j not in taken and err[i, j] < thr)
            if cands:
                taken[cands[0][1]] = i
        inv = {i: j for j, i in taken.items()}
        est_rows.append([inv.get(i, -1) for i in range(A)])
        gt_rows.append([taken.get(j, -1) for j in range(B)])
    return np.array(est_rows, np.int32).reshape(-1, A), np.array(gt_rows, np.int32).reshape(-1, B), np.array([sum(j >= 0 for j in r) for r in gt_rows], np.int32)


def _naive_nms(err, scores, thresh):
    err = np.asarray(err, F32)
    walk = _naive_order(scores)
    dead, by, kept = set(), {}, []
    for p, r in enumerate(walk):
        if r in dead:
            continue
        kept.append(r)
        by[r] = r
        for i in walk[p + 1:]:
            if i not in dead and err[r, i] < F32(thresh):
                dead.add(i)
                by[i] = r
    return kept, [by[i] for i in range(len(walk))]


def _lumpy(g, shape):
    """values from a small set, so that ties, exact thresholds, -0, NaN and infinities are everywhere"""
    pool = np.array([0.0, -0.0, 0.25, 0.25, 0.5, 0.75, 1.0, 2.0, -1.0, np.inf, NAN, NAN], F32)
    return pool[g.integers(0, len(pool), shape)]


@pytest.mark.parametrize("seed", range(4))
def test_matching_restatement_against_sort_then_scan(seed):
    """75 cases a seed: equal scores, equal errors, err == thr, NaN scores and NaN errors"""
    g = np.random.default_rng(seed)
    ties = exact = nan_s = nan_e = 0
    for _ in range(75):
        A, B, T = int(g.integers(1, 9)), int(g.integers(1, 9)), int(g.integers(1, 4))
        err, scores = _lumpy(g, (A, B)), _lumpy(g, A)
        thr = np.array([0.25, 0.5, 1.0, np.inf], F32)[g.integers(0, 4, T)]
        valid = None if g.random() < 0.5 else g.random(B) < 0.7
        max_ests = int(g.integers(0, A + 2))
        got, want = MR.match(err, scores, thr, valid, max_ests), _naive_match(err, scores, thr, valid, max_ests)
        for a, b in zip(got, want):
            assert a.dtype == np.int32 and np.array_equal(a, b), (err, scores, thr, valid, max_ests, a, b)
        ties += len(set(scores[~np.isnan(scores)].tolist())) < (~np.isnan(scores)).sum()
        exact += bool(np.isin(err, thr).any())
        nan_s += bool(np.isnan(scores).any())
        nan_e += bool(np.isnan(err).any())
    assert min(ties, exact, nan_s, nan_e) > 20


@pytest.mark.parametrize("seed", range(4))
def test_nms_restatement_against_sort_then_scan(seed):
    g = np.random.default_rng(100 + seed)
    for _ in range(75):
        N = int(g.integers(1, 12))
        err, scores = _lumpy(g, (N, N)), _lumpy(g, N)  # not symmetric
        thresh = float(np.array([0.25, 0.5, 1.0, np.inf, NAN], F32)[g.integers(0, 5)])
        keep_idx, count, by = MR.nms(err, scores, thresh)
        kept, by_naive = _naive_nms(err, scores, thresh)
        assert count.tolist() == [len(kept)] and keep_idx[:len(kept)].tolist() == kept and (keep_idx[len(kept):] == -1).all(), (err, scores, thresh)
        assert by.dtype == np.int32 and by.tolist() == by_naive, (err, scores, thresh)


def test_the_order():
    s = np.array([0.5, NAN, 0.5, -np.inf, 0.0, -0.0, np.inf, -1.0, NAN], F32)
    assert MR.order(s) == _naive_order(s) == [6, 0, 2, 4, 5, 7, 3, 1, 8]


def test_matching_rules():
    err = np.array([[0.3, 0.3, 0.1], [0.1, 0.3, 0.1], [0.2, NAN, 0.05]], F32)
    scores = np.array([0.9, 0.9, 0.5], F32)
    est, gt, n = MR.match(err, scores, [1.0, 0.3, 0.1, 0.05])
    # estimate 0 goes first (equal scores: the lower index) and takes target 2; estimate 1 takes target 0 (equal errors: the lower j is
    # free); estimate 2 is left with target 1, a NaN
    assert est[0].tolist() == [2, 0, -1] and gt[0].tolist() == [1, -1, 0] and n[0] == 2
    assert est[1].tolist() == [2, 0, -1]                  # 0.3 < 0.3 is false: the 0.3 entries are out
    assert est[2].tolist() == [-1, -1, 2] and n[2] == 1   # err == thr is no match; estimate 2's 0.05 is
    assert est[3].tolist() == [-1, -1, -1] and n[3] == 0
    # max_ests in the middle of a tie: only estimate 0 of the two equal scores takes part
    est, gt, n = MR.match(err, scores, [1.0], max_ests=1)
    assert est.tolist() == [[2, -1, -1]] and gt.tolist() == [[-1, -1, 0]] and n.tolist() == [1]
    est, gt, n = MR.match(err, scores, [1.0], valid=[False, True, False])
    assert est.tolist() == [[1, -1, -1]] and gt.tolist() == [[-1, 0, -1]]


def test_nms_rules():
    inf = np.inf
    # the chain: a suppresses b, b would suppress c, a does not suppress c -> c is kept
    err = np.array([[0, 0.1, 0.9], [0.1, 0, 0.1], [0.9, 0.1, 0]], F32)
    keep_idx, count, by = MR.nms(err, [3.0, 2.0, 1.0], 0.5)
    assert keep_idx.tolist() == [0, 2, -1] and count.tolist() == [2] and by.tolist() == [0, 0, 2]
    # not symmetric: the row is the kept, higher-ranked pose
    err = np.array([[0, 0.9], [0.1, 0]], F32)
    assert MR.nms(err, [2.0, 1.0], 0.5)[0].tolist() == [0, 1] and MR.nms(err, [1.0, 2.0], 0.5)[0].tolist() == [1, -1]
    assert MR.nms(err, [1.0, 2.0], 0.5)[2].tolist() == [1, 1]
    # strict, and the diagonal is not read
    err = np.array([[NAN, 0.5], [0.5, NAN]], F32)
    assert MR.nms(err, [2.0, 1.0], 0.5)[1].tolist() == [2] and MR.nms(err, [2.0, 1.0], np.nextafter(F32(0.5), F32(1)))[1].tolist() == [1]
    assert MR.nms(np.zeros((5, 5), F32), [1.0, 5.0, 5.0, 2.0, NAN], 1e-9)[0].tolist() == [1, -1, -1, -1, -1]
    assert MR.nms(np.full((3, 3), inf, F32), [1.0, 2.0, 3.0], inf)[0].tolist() == [2, 1, 0]


def test_instance_recall_is_not_recall():
    r = posematch.instance_recall(torch.tensor([0, 2, 3], dtype=torch.int32), 4)
    assert r.dtype == torch.float32 and r.tolist() == [0.0, 0.5, 0.75]
    assert torch.isnan(posematch.instance_recall(torch.tensor([0, 0]), 0)).all()
    r = posematch.instance_recall(torch.tensor([[1, 2], [0, 0]]), torch.tensor([[2], [0]]))
    assert r[0].tolist() == [0.5, 1.0] and torch.isnan(r[1]).all()
    assert "poseerr.recall" in posematch.instance_recall.__doc__
    for text in (posematch.__doc__, posematch.match_poses.__doc__):
        assert "bop_toolkit" in text  # the recipe is advertised as the package's own wherever it is offered


# ------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("seed", [0, 1])
def test_pair_restatement_against_float64(seed):
    g = np.random.default_rng(seed)
    A, Bn, V = 4, 3, 40
    pts = g.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    b = np.stack([VR.pose((g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(5, 8)), axis=g.normal(size=3), angle=g.uniform(0, 3)) for _ in range(Bn)])
    a = np.stack([VR.pose(b[k % Bn][:, 3].astype(F64) + g.normal(size=3) * 0.2, axis=g.normal(size=3), angle=g.uniform(0, 3)) for k in range(A)])
    syms = poseerr.symmetry_transforms(discrete=[np.concatenate([VR.rotation((0, 0, 1), math.pi), [[0.1], [0.0], [0.0]]], axis=1)])
    inv_unit = F32(0.5)
    got = MR.pair_errors(pts, a, b, syms, (600.0, 590.0, 320.0, 240.0), inv_unit)

    def h(M):
        return np.concatenate([np.asarray(M, F64), np.broadcast_to([0.0, 0.0, 0.0, 1.0], M.shape[:-2] + (1, 4))], axis=-2)
    X = np.concatenate([pts.astype(F64), np.ones((V, 1))], axis=1).T
    e = (h(a) @ X)[:, None, None, :3]                                      # (A,1,1,3,V)
    gg = (h(b)[:, None] @ h(syms)[None] @ X)[None, :, :, :3]               # (1,B,S,3,V)
    dist = np.linalg.norm(e - gg, axis=3)                                  # (A,B,S,V)
    mssd, add = dist.max(axis=3).min(axis=2), dist[:, :, 0].mean(axis=2)
    rows = np.concatenate([a.astype(F64), PR.sym_gt(b, syms).astype(F64).reshape(-1, 3, 4)])
    Bd = float((np.abs(rows[:, :, :3]) @ np.abs(pts.astype(F64)).T + np.abs(rows[:, :, 3:])).max())
    assert got["mssd"].shape == (A, Bn) and np.abs(got["mssd"].astype(F64) - mssd).max() <= PR.mssd_bound(Bd)
    got_add = PR.add_of(got["add_sum"], inv_unit, V).astype(F64)
    assert np.abs(got_add - add).max() <= PR.add_bound(Bd, float(inv_unit), float(add.max()))
    assert mssd.min() > 1e3 * PR.mssd_bound(Bd)  # the bound binds
    # and the layout: entry (i, j) is pair (a[i], b[j])
    one = PR.point_errors(pts, a[2:3], b[1:2], syms, (600.0, 590.0, 320.0, 240.0), inv_unit)
    assert all(got[k][2, 1] == one[k][0] for k in MR.PAIR_FIELDS)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    pts = torch.zeros(8, 3)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    K = (60.0, 60.0, 32.0, 24.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_errors(pts, R, t, R, t, K)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_errors(dict(vertices=pts.numpy()), R, t, R, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pair_errors(pts, R, t, R, t, syms=poseerr.symmetry_transforms())
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.nms_poses(pts, R, t, torch.zeros(2), 0.1)
    with pytest.raises(ValueError, match="R_a"):
        posematch.pair_errors(pts, R[0], t, R, t)
    with pytest.raises(ValueError, match="t_a"):
        posematch.pair_errors(pts, R, t[:1], R, t)
    with pytest.raises(ValueError, match="R_b"):
        posematch.pair_errors(pts, R, t, R.double(), t)
    with pytest.raises(ValueError, match="t_b"):
        posematch.pair_errors(pts, R, t, R, t.reshape(3, 2))
    with pytest.raises(ValueError, match="R_a"):
        posematch.pair_errors(pts, R[:0], t[:0], R, t)
    with pytest.raises(ValueError, match="R_b"):
        posematch.pair_errors(pts, R, t, R.repeat(513, 1, 1), t.repeat(513, 1))
    with pytest.raises(ValueError, match="points"):
        posematch.pair_errors(torch.zeros(8, 2), R, t, R, t)
    with pytest.raises(ValueError, match="syms"):
        posematch.pair_errors(pts, R, t, R, t, syms=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="K must"):
        posematch.pair_errors(pts, R, t, R, t, K=(1.0, 2.0))
    with pytest.raises(ValueError, match="unit"):
        posematch.pair_errors(pts, R, t, R, t, unit=0.0)
    big_R, big_t = R.repeat(512, 1, 1), t.repeat(512, 1)
    with pytest.raises(ValueError, match="A B S = 1024 x 1024 x 5"):  # the cap, before anything is launched
        posematch.pair_errors(pts, big_R, big_t, big_R, big_t, syms=torch.zeros(5, 3, 4))
    err, s = torch.zeros(3, 4), torch.zeros(3)
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.match_poses(err, s, [0.1])
    with pytest.raises(RuntimeError, match="HIP device"):
        posematch.pose_nms(torch.zeros(3, 3), s, 0.1)
    with pytest.raises(ValueError, match="err"):
        posematch.match_poses(torch.zeros(3), s, [0.1])
    with pytest.raises(ValueError, match="err"):
        posematch.match_poses(err.double(), s, [0.1])
    with pytest.raises(ValueError, match="err"):
        posematch.pose_nms(torch.zeros(3, 4), s, 0.1)  # not square
    with pytest.raises(ValueError, match="scores"):
        posematch.match_poses(err, torch.zeros(4), [0.1])
    with pytest.raises(ValueError, match="valid"):
        posematch.match_poses(err, s, [0.1], valid=torch.ones(4))
    with pytest.raises(ValueError, match="thresholds"):
        posematch.match_poses(err, s, [0.1] * 65)
    with pytest.raises(ValueError, match="max_ests"):
        posematch.match_poses(err, s, [0.1], max_ests=-1)
    with pytest.raises(ValueError, match="1024"):
        posematch.pose_nms(torch.zeros(1025, 1025), torch.zeros(1025), 0.1)
    with pytest.raises(ValueError, match="n_matched"):
        posematch.instance_recall([1, 2], 3)


def test_kernel_resources():
    """no kernel of posematch.hip uses scratch or spills a vector register, and each keeps within its built
    VGPR count rounded up to the next step of 8 (built: pair_errors 76 with the pixel half, all pairs <PIX, DIAG> = <1, 0> and the
    diagonal <1, 1> that sam6d_pose_point_errors runs, and 64 without it, pair_errors_finish 18, pm_order 4, pm_match 88, pm_nms_mask 12,
    pm_nms_scan 26).  Read from the code object's metadata: the compiler's figures."""
    from tests._util import kernel_resources
    limits = dict(pair_errors_kernelILb1ELb0E=80, pair_errors_kernelILb1ELb1E=80, pair_errors_kernelILb0ELb0E=64, pair_errors_finish_kernel=24,
                  pm_order_kernel=8, pm_match_kernel=88, pm_nms_mask_kernel=16, pm_nms_scan_kernel=32)
    found = kernel_resources(b"pair_errors_kernel", name_regex=r"(pair_errors_kernelILb[01]ELb[01]E|[a-z_]+_kernel)")
    print("\n[posematch] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
