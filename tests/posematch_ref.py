"""Numpy restatement of csrc/posematch.hip (sam6d_hip.posematch), code of its own.  The pair errors are tests/poseerr_ref.py's
point_errors on the expanded pair list -- imported, not copied: the recipe has one restatement.  Matching and suppression are plain
loops over the recipe at the top of posematch.hip.  The recipes are the package's own (BOP's match_poses in kind); nothing here is
bop_toolkit's code or checked against it.

    order     by descending score, equal scores (-0 equals +0) the lower index first, a NaN score after every number
    matching  per threshold, walking the first max_ests of the order (all when max_ests is 0): estimate i takes the valid free target
              j with the smallest err[i][j] < thr (strict, false for a NaN), the lowest j among equal errors
    nms       walking the order: i is kept unless a pose r kept before it has err[r][i] < thresh; suppressed_by[i] = the first such r
"""
import numpy as np

from tests import poseerr_ref as PR

F32 = np.float32
PAIR_FIELDS = ("mssd", "mspd", "mssd_sym", "mspd_sym", "n_skipped", "add_sum")


def expand(a, b):
    """(A,3,4), (B,3,4) -> the A B pairs in row-major order: est = a[i] repeated, gt = b tiled"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.repeat(a, len(b), axis=0), np.tile(b, (len(a), 1, 1))


def pair_errors(points, a, b, syms, intr, inv_unit=1.0, chunk=256):
    """sam6d_pose_pair_errors -> dict of (A,B) arrays, poseerr_ref.point_errors on the expanded pairs"""
    est, gt = expand(a, b)
    parts = [PR.point_errors(points, est[k:k + chunk], gt[k:k + chunk], syms, intr, inv_unit) for k in range(0, len(est), chunk)]
    return {k: np.concatenate([p[k] for p in parts]).reshape(len(a), len(b)) for k in PAIR_FIELDS}


def order(scores):
    """the estimates' order: a loop that picks, again and again, the best of those left"""
    s = np.asarray(scores, F32).tolist()  # (Python floats hold every float32 and compare as they do; a loop over them is quick)
    left, out = list(range(len(s))), []
    while left:
        best = left[0]
        for i in left[1:]:
            if s[best] != s[best] and s[i] == s[i]:
                best = i
            elif s[i] > s[best]:  # (false for a NaN and for -0 against +0: the earlier index stays)
                best = i
        left.remove(best)
        out.append(best)
    return out


def match(err, scores, thresholds, valid=None, max_ests=0):
    """sam6d_pose_match -> est_match (T,A), gt_match (T,B), n_matched (T) int32"""
    err = np.asarray(err, F32)
    A, B = err.shape
    err = err.tolist()
    thr = np.asarray(thresholds, F32).reshape(-1).tolist()
    valid = np.ones(B, bool) if valid is None else np.asarray(valid, bool)
    walk = order(scores)
    if max_ests > 0:
        walk = walk[:max_ests]
    est_match, gt_match = np.full((len(thr), A), -1, np.int32), np.full((len(thr), B), -1, np.int32)
    for k, limit in enumerate(thr):
        free = [j for j in range(B) if valid[j]]  # ascending, so the first of equal errors is the lowest j
        for i in walk:
            best, row = -1, err[i]
            for j in free:
                if row[j] < limit and (best < 0 or row[j] < row[best]):
                    best = j
            if best >= 0:
                est_match[k, i], gt_match[k, best] = best, i
                free.remove(best)
    return est_match, gt_match, (est_match >= 0).sum(axis=1).astype(np.int32)


def nms(err, scores, thresh):
    """sam6d_pose_nms -> keep_idx (N) int64 padded with -1, count (1) int32, suppressed_by (N) int32"""
    err = np.asarray(err, F32).tolist()
    N, thresh = len(err), float(F32(thresh))
    kept, by = [], np.zeros(N, np.int32)
    for i in order(scores):
        by[i] = i
        for r in kept:
            if err[r][i] < thresh:
                by[i] = r
                break
        if by[i] == i:
            kept.append(i)
    keep_idx = np.full(N, -1, np.int64)
    keep_idx[:len(kept)] = kept
    return keep_idx, np.array([len(kept)], np.int32), by
