"""All-pairs pose errors on the device, and what is built on an error matrix: the matching of estimates to ground-truth instances
and the removal of duplicate poses.  sam6d_hip.poseerr scores pose PAIRS (estimate n against ground truth n); with several proposals
per instance, as SAM's over-segmentation gives them, somebody has to decide which ground truth an estimate belongs to and which
estimates are the same instance, and both need the error of every pose against every other pose of the same object.

The reference has none of this: it writes all its poses with their scores (PEM/run_inference_custom_pytorch.py:460-471) and leaves
matching and scoring to bop_toolkit.  pair_errors is poseerr.pose_errors for every (i, j), bit for bit (csrc/posematch.hip over the
per-point step of csrc/poseerr_point.h).  match_poses is BOP's match_poses IN KIND -- greedy, by descending score, each estimate
taking the nearest free target under the threshold -- and pose_nms is a greedy suppression; both recipes are the package's own,
written out at the top of csrc/posematch.hip and restated in tests/posematch_ref.py, and every comparison with that restatement is
bit for bit.  Nothing here is pinned against bop_toolkit itself, which the suite does not have.

pair_vsd is the third BOP error as a matrix: poseerr.vsd's counts for every (i, j), bit for bit, from one render per pose
(csrc/vsdpairs.hip, restated in tests/vsdpairs_ref.py), and vsd_matches runs match_poses on it once per tolerance -- with
instance_recall that is AR_VSD, beside the AR_MSSD and AR_MSPD that pair_errors' matrices give.

pair_adi is ADD-S / ADI as a matrix: poseerr.adi's integer for every (i, j), bit for bit (csrc/pairadi.hip over the walk of
csrc/nearest.hip, restated in tests/pair_adi_ref.py), and with a cap the pairs whose tile bounds already put them above it are
answered +inf without their V x V search.  nms_poses_adi removes duplicate poses by it: ADI sees through a symmetry that nobody
annotated, which MSSD without syms does not.  ADI is evaluated over the vertices, and is not pinned against bop_toolkit either.

Poses of different objects are separate calls, one mesh each (INTEGRATION.md has the loop over template_ids).  Left to the caller:
symmetry-aware ADI, several meshes in one call, BOP's file formats and threshold lists.

Imports poseerr, verify, runtime, _lib, torch and math only; the library is loaded at the first launch, not at import.  There is no
CPU route: a CPU tensor raises RuntimeError.
"""
import math

import torch

from . import _lib, verify
from .poseerr import ADD_SCALE, MAX_POINTS, PoseErrors, _errors, _intrinsics, _inv_unit, _points, _same_device, _syms  # noqa: F401
from .poseerr import MAX_TAUS, _adi_of, _c_floats, _tolerances, morton_order, vsd_from_counts
from .runtime import _empty, _p, _s, on_tensor_device
from .verify import NEAR, _tensor

MAX_POSES = 1024             # A, B, S of pair_errors and match_poses, N of pose_nms
MAX_TRIPLES = 1 << 22        # A B S: a workspace of 8 bytes per triple, 32 MiB at most
MAX_THRESHOLDS = 64
MAX_VSD_WORDS = 1 << 28      # pair_vsd: the window words of all A + B views, a z-buffer of 2 GiB at most
NO_MSPD = 1                  # sam6d_pose_pair_errors flags bit 0
MAX_ADI_WORKGROUPS = 1 << 22 # pair_adi: A B ceil(V / 1024), the workgroups of one launch
ADI_NMS_MARGIN = 2.0 ** -20  # nms_poses_adi: cap = thresh * (1 + margin)


class PairErrors(PoseErrors):
    """What pair_errors returns; every tensor is on the device and (A,B): row i the pose a[i], column j the pose b[j].  mssd, add f32
    in the unit of t, mssd_sym i32, add_sum i64 the integer ADD is formed from; with K also mspd f32 in pixels, mspd_sym i32 and
    n_skipped i32, else None.  The fields are poseerr.PoseErrors' for est = a[i], gt = b[j]."""


class PoseMatches:
    """What match_poses returns.  est_match (T,A) i32 the target of estimate i under threshold k or -1, gt_match (T,B) i32 the
    estimate that took target j or -1, n_matched (T) i32, all on the device; n_targets a Python int, the targets that could be taken
    (valid ones)."""

    def __init__(self, est_match, gt_match, n_matched, n_targets):
        self.est_match, self.gt_match, self.n_matched, self.n_targets = est_match, gt_match, n_matched, n_targets


class PoseNms:
    """What pose_nms returns, all on the device.  keep_idx (N) i64 the kept poses by descending score, then -1; count (1) i32 how many;
    suppressed_by (N) i32 the first kept pose in order that suppresses i, i itself when it is kept.  kept() reads count back (4
    bytes) and returns keep_idx[:count]."""

    def __init__(self, keep_idx, count, suppressed_by):
        self.keep_idx, self.count, self.suppressed_by = keep_idx, count, suppressed_by

    def kept(self):
        return self.keep_idx[:int(self.count)]


# ------------------------------------------------------------------------------------------------------------ pair errors
def _poses(name, what, R, t, least=1):
    if not torch.is_tensor(R) or R.dim() != 3:
        raise ValueError("%s: R_%s must be an (N,3,3) float32 tensor" % (name, what))
    N = int(R.shape[0])
    R, t = _tensor(R, name, "R_" + what, torch.float32, (N, 3, 3)), _tensor(t, name, "t_" + what, torch.float32, (N, 3))
    if not least <= N <= MAX_POSES:
        raise ValueError("%s: R_%s: %s = %d is not in %d .. %d" % (name, what, what.upper(), N, least, MAX_POSES))
    return R, t


@on_tensor_device
def _pair_errors(points, a, b, syms, intr, inv_unit):
    A, B = int(a.shape[0]), int(b.shape[0])
    return _errors(PairErrors, "sam6d_pose_pair_errors", points, (A, B), (_p(a), A, _p(b), B), syms, intr, inv_unit,
                   (0 if intr is not None else NO_MSPD,))


def pair_errors(mesh_or_points, R_a, t_a, R_b, t_b, K=None, syms=None, scale=1.0, unit=None):
    """MSSD, MSPD and ADD of every pose a[i] against every pose b[j] of one object, over the model's vertices: for every (i, j), bit
    for bit, what poseerr.pose_errors gives for est = a[i], gt = b[j].

    mesh_or_points, syms, scale and unit as poseerr.pose_errors has them.  R_a (A,3,3), t_a (A,3), R_b (B,3,3), t_b (B,3) f32 HIP
    tensors; A, B and the number of symmetries S at most 1024 each, and A B S at most 2^22.  K: one 3 x 3 matrix or (fx, fy, cx, cy);
    None leaves MSPD out: the projections are not computed and mspd, mspd_sym, n_skipped are None.
    -> PairErrors, every field (A,B).  The symmetries are applied to b: where a symmetry other than the first attains the minimum,
    mssd[i][j] and mssd[j][i] of a set against itself can differ in the last bits.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "pair_errors"
    R_a, t_a = _poses(name, "a", R_a, t_a)
    R_b, t_b = _poses(name, "b", R_b, t_b)
    points = _points(name, mesh_or_points, R_a)
    intr = None if K is None else _intrinsics(name, K)
    inv_unit = _inv_unit(name, unit)
    syms = _syms(name, syms, points, MAX_POSES)
    A, B, S = int(R_a.shape[0]), int(R_b.shape[0]), int(syms.shape[0])
    if A * B * S > MAX_TRIPLES:
        raise ValueError("%s: A B S = %d x %d x %d = %d is above the cap of %d: split a or b" % (name, A, B, S, A * B * S, MAX_TRIPLES))
    _same_device(name, points, (("R_a", R_a), ("t_a", t_a), ("R_b", R_b), ("t_b", t_b), ("syms", syms)))
    return _pair_errors(points, verify.pose_views(R_a, t_a, scale), verify.pose_views(R_b, t_b, scale), syms, intr, inv_unit)


# ------------------------------------------------------------------------------------------------------------ matching
def _device_only(name, *tensors):
    """after the shapes and dtypes: the host-side shortcuts (no targets, no poses) refuse a CPU tensor as a launch would"""
    if any(torch.is_tensor(x) and not x.is_cuda for x in tensors):
        raise RuntimeError("%s: needs HIP device tensors (this build has no CPU path)" % name)


def _matrix(name, err, square=False):
    err = _tensor(err, name, "err", torch.float32, (None, None))
    if square and int(err.shape[0]) != int(err.shape[1]):
        raise ValueError("%s: err must have shape (N,N), got %s" % (name, tuple(err.shape)))
    return err


@on_tensor_device
def _match(err, scores, thr, valid, max_ests):
    A, B, T = int(err.shape[0]), int(err.shape[1]), int(thr.shape[0])
    need = int(_lib.load().sam6d_pose_match_workspace_bytes(A))
    ws = _empty((need // 4,), err, torch.int32)
    est_match, gt_match, n_matched = (_empty(s, err, torch.int32) for s in ((T, A), (T, B), (T,)))
    _lib.call("sam6d_pose_match", _p(err), A, B, _p(scores), _p(thr), T, None if valid is None else valid.data_ptr(), max_ests, _p(est_match),
              _p(gt_match), _p(n_matched), _p(ws), need, _s())
    return est_match, gt_match, n_matched


def match_poses(err, scores, thresholds, valid=None, max_ests=0):
    """Greedy matching of A estimates to B ground-truth instances of one object from their error matrix, for each threshold on its
    own: BOP's match_poses in kind, the package's own recipe (csrc/posematch.hip RECIPE b), not pinned against bop_toolkit.

    err (A,B) f32 HIP tensor (pair_errors' mssd, mspd or add); scores (A) f32 HIP tensor; thresholds: 1 .. 64 numbers (a sequence or a
    tensor), in err's unit; valid (B) bool HIP tensor, the targets that may be taken (None: all); max_ests > 0: only the max_ests
    best-scored estimates take part (BOP: the number of instances of the object in the image).
    The estimates go by descending score, equal scores the lower index first, a NaN score last.  In that order estimate i takes the
    free valid target j with the smallest err[i][j] < threshold (strict; never a NaN), the lowest j among equal errors.
    -> PoseMatches: est_match (T,A), gt_match (T,B), n_matched (T) i32 and n_targets.  B = 0, A = 0 or no valid target: everything is
    -1 / 0, by torch fills without a launch.  One read-back of 8 bytes when valid is given.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "match_poses"
    err = _matrix(name, err)
    A, B = int(err.shape[0]), int(err.shape[1])
    scores = _tensor(scores, name, "scores", torch.float32, (A,))
    if not (A <= MAX_POSES and B <= MAX_POSES):
        raise ValueError("%s: err: A, B = %d, %d: each must be at most %d" % (name, A, B, MAX_POSES))
    thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
    T = int(thr.shape[0])
    if not 1 <= T <= MAX_THRESHOLDS:
        raise ValueError("%s: thresholds: T = %d is not in 1 .. %d" % (name, T, MAX_THRESHOLDS))
    max_ests = int(max_ests)
    if max_ests < 0:
        raise ValueError("%s: max_ests = %d is negative" % (name, max_ests))
    n_targets = B
    if valid is not None:
        valid = _tensor(valid, name, "valid", torch.bool, (B,))
    _device_only(name, err, scores, valid)
    thr = thr.to(err.device).contiguous()
    _same_device(name, err, (("scores", scores),) + ((("valid", valid),) if valid is not None else ()))
    if valid is not None:
        n_targets = int(valid.sum())
    if A == 0 or n_targets == 0:
        return PoseMatches(torch.full((T, A), -1, dtype=torch.int32, device=err.device), torch.full((T, B), -1, dtype=torch.int32, device=err.device),
                           torch.zeros((T,), dtype=torch.int32, device=err.device), n_targets)
    return PoseMatches(*_match(err, scores, thr, valid, max_ests), n_targets)


def instance_recall(n_matched, n_targets):
    """The recall over the INSTANCES: n_matched / n_targets as f32, NaN where n_targets is 0.  n_matched a tensor (match_poses'
    (T), or sums of it over images and objects), n_targets a number or a tensor that broadcasts.  A plain torch op.
    This is not poseerr.recall: that is the fraction of pose PAIRS under a threshold, where the caller already knows which ground
    truth belongs to which estimate; this divides the matched instances by the instances there are, as every BOP recall does."""
    if not torch.is_tensor(n_matched):
        raise ValueError("instance_recall: n_matched must be a tensor")
    n = torch.as_tensor(n_targets, device=n_matched.device).to(torch.float32)
    return torch.where(n > 0, n_matched.to(torch.float32) / n, torch.full_like(n, float("nan")))


# ------------------------------------------------------------------------------------------------------------ suppression
@on_tensor_device
def _nms(err, scores, thresh):
    N = int(err.shape[0])
    need = int(_lib.load().sam6d_pose_nms_workspace_bytes(N))
    ws = _empty((need // 8,), err, torch.int64)
    keep_idx, count, by = _empty((N,), err, torch.int64), _empty((1,), err, torch.int32), _empty((N,), err, torch.int32)
    _lib.call("sam6d_pose_nms", _p(err), _p(scores), N, thresh, keep_idx.data_ptr(), _p(count), _p(by), ws.data_ptr(), need, _s())
    return PoseNms(keep_idx, count, by)


def pose_nms(err, scores, thresh):
    """Greedy removal of duplicate poses of one object from their (N,N) error matrix (csrc/posematch.hip RECIPE c; the package's own
    recipe).  err (N,N) f32 HIP tensor, err[r][i] the error of pose i against pose r; it need not be symmetric and its diagonal is not
    read.  scores (N) f32 HIP tensor; the order is match_poses'.  Walking it, pose i is kept unless a pose r kept before it has
    err[r][i] < thresh (strict).  A pose that only a suppressed pose would suppress is kept.
    -> PoseNms: keep_idx (N) i64, count (1) i32, suppressed_by (N) i32.  N = 0: empty tensors, no launch.  N at most 1024.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "pose_nms"
    err = _matrix(name, err, square=True)
    N = int(err.shape[0])
    scores = _tensor(scores, name, "scores", torch.float32, (N,))
    if N > MAX_POSES:
        raise ValueError("%s: err: N = %d is above %d" % (name, N, MAX_POSES))
    _device_only(name, err, scores)
    _same_device(name, err, (("scores", scores),))
    if N == 0:
        return PoseNms(torch.empty((0,), dtype=torch.int64, device=err.device), torch.zeros((1,), dtype=torch.int32, device=err.device),
                       torch.empty((0,), dtype=torch.int32, device=err.device))
    return _nms(err, scores, float(thresh))


def nms_poses(mesh_or_points, R, t, scores, thresh, syms=None, scale=1.0):
    """pose_nms on the MSSD of the poses against themselves: pair_errors(mesh, R, t, R, t, syms=syms, scale=scale).mssd, so thresh is
    a length in the unit of t (a fraction of the model's diameter is a good one).  Arguments as pair_errors and pose_nms have them.
    -> (PoseNms, the (N,N) mssd matrix)."""
    mssd = pair_errors(mesh_or_points, R, t, R, t, K=None, syms=syms, scale=scale).mssd
    return pose_nms(mssd, scores, thresh), mssd


# ------------------------------------------------------------------------------------------------------------ ADI as a matrix
class PairAdi:
    """What pair_adi returns; every tensor is on the device and (A,B): row i the pose a[i], column j the pose b[j].  adi f32 in the
    unit of t and adi_sum i64 the integer it is formed from, poseerr.AdiErrors' fields for est = a[i], gt = b[j]; lower_sum i64 the
    tile bounds' sum that never exceeds adi_sum (None without a cap); skipped bool: the pair is above the cap by its lower_sum, its
    adi is +inf and its adi_sum -1."""

    def __init__(self, adi, adi_sum, lower_sum, skipped):
        self.adi, self.adi_sum, self.lower_sum, self.skipped = adi, adi_sum, lower_sum, skipped


def _cap_sum(name, cap, inv_unit, V):
    """the cap as the integer the kernels compare lower_sum with: floor(cap * inv_unit * 2^30 * V) in float64, at most 2^63 - 1"""
    cap = float(cap)
    if not (cap >= 0.0 and math.isfinite(cap)):
        raise ValueError("%s: cap = %r is not a finite number >= 0" % (name, cap))
    x = ((cap * inv_unit) * ADD_SCALE) * V
    return (1 << 63) - 1 if x >= 2.0 ** 63 else int(math.floor(x))


@on_tensor_device
def _pair_adi(points, a, b, inv_unit, cap_sum, sort, prune):
    V, A, B = int(points.shape[0]), int(a.shape[0]), int(b.shape[0])
    if sort:
        points = points[morton_order(points)].contiguous()
    need = int(_lib.load().sam6d_pose_pair_adi_workspace_bytes(V, A, B))
    ws = _empty((need // 8,), points, torch.int64)
    adi_sum, skipped = _empty((A, B), points, torch.int64), _empty((A, B), points, torch.bool)
    lower_sum = _empty((A, B), points, torch.int64) if cap_sum >= 0 else None
    _lib.call("sam6d_pose_pair_adi", _p(points), V, _p(a), A, _p(b), B, inv_unit, 0 if prune else 1, cap_sum, adi_sum.data_ptr(),
              None if lower_sum is None else lower_sum.data_ptr(), skipped.data_ptr(), ws.data_ptr(), need, _s())
    adi = torch.where(skipped, torch.full_like(adi_sum, float("inf"), dtype=torch.float32), _adi_of(adi_sum, inv_unit, V))
    return PairAdi(adi, adi_sum, lower_sum, skipped)


def pair_adi(mesh_or_points, R_a, t_a, R_b, t_b, scale=1.0, unit=None, cap=None, sort=True, prune=True):
    """ADD-S / ADI of every pose a[i] against every pose b[j] of one object, over the model's vertices: for every (i, j) that is
    computed, bit for bit, what poseerr.adi gives for est = a[i], gt = b[j].  The roles are not symmetric (the nearest vertex is
    searched under b[j]), so pair_adi(.., a, b) is not the transpose of pair_adi(.., b, a).  No symmetry transforms are needed or
    applied; nothing is pinned against bop_toolkit.

    mesh_or_points, scale, unit, sort and prune as poseerr.adi has them; R_a (A,3,3), t_a (A,3), R_b (B,3,3), t_b (B,3) f32 HIP
    tensors, A and B 0 .. 1024 each, V 1 .. 2^20, and A B ceil(V / 1024) at most 2^22 (the workgroups of one launch: split a or b, or
    pass fewer vertices).  An empty side gives empty tensors without a launch.
    cap: a distance in the unit of t, or None.  With a cap, every pair gets lower_sum, the sum of the terms of each vertex's
    distance to the nearest tile box of b[j]: V / 256 box tests per vertex where the search costs V distances.  lower_sum <=
    adi_sum holds exactly (csrc/pairadi.hip has the proof), so a pair whose lower_sum is above floor(cap * (1 / unit) * 2^30 * V) has
    an ADI above the cap: it is skipped, its search is never started, skipped is True, adi +inf and adi_sum -1.  Every other pair is
    computed in full, also where its ADI turns out above the cap.  Use it where only errors below a threshold matter: for
    match_poses under the ADD(-S) protocol pass cap = the largest threshold * (1 + 2^-20) (nms_poses_adi derives the margin), and
    the matching is the uncapped matrix's.  For a dense mesh pass a subset of the vertices (ops.furthest_point_sampling): the cost of
    a computed pair grows with V^2.
    Neither sort nor prune changes a bit of any output; lower_sum belongs to the tiles of the order the search runs in (sorted or
    as given).  There is no read-back.
    -> PairAdi: adi (A,B) f32, adi_sum (A,B) i64, lower_sum (A,B) i64 or None, skipped (A,B) bool.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument, and so does a cap that is negative or
    not finite."""
    name = "pair_adi"
    R_a, t_a = _poses(name, "a", R_a, t_a, least=0)
    R_b, t_b = _poses(name, "b", R_b, t_b, least=0)
    points = _points(name, mesh_or_points, R_a)
    inv_unit = _inv_unit(name, unit)
    V, A, B = int(points.shape[0]), int(R_a.shape[0]), int(R_b.shape[0])
    cap_sum = -1 if cap is None else _cap_sum(name, cap, inv_unit, V)
    groups = A * B * ((V + 1023) // 1024)
    if groups > MAX_ADI_WORKGROUPS:
        raise ValueError("%s: A B ceil(V / 1024) = %d x %d x %d = %d is above the cap of %d workgroups a launch: split a or b, or pass fewer "
                         "vertices" % (name, A, B, (V + 1023) // 1024, groups, MAX_ADI_WORKGROUPS))
    _device_only(name, points, R_a, t_a, R_b, t_b)
    _same_device(name, points, (("R_a", R_a), ("t_a", t_a), ("R_b", R_b), ("t_b", t_b)))
    if A == 0 or B == 0:
        dev = points.device
        return PairAdi(torch.empty((A, B), dtype=torch.float32, device=dev), torch.empty((A, B), dtype=torch.int64, device=dev),
                       None if cap is None else torch.empty((A, B), dtype=torch.int64, device=dev), torch.empty((A, B), dtype=torch.bool, device=dev))
    return _pair_adi(points, verify.pose_views(R_a, t_a, scale), verify.pose_views(R_b, t_b, scale), inv_unit, cap_sum, bool(sort), bool(prune))


def nms_poses_adi(mesh_or_points, R, t, scores, thresh, scale=1.0, unit=None):
    """pose_nms on the ADI of the poses against themselves, capped just above thresh: duplicate poses of an object whose symmetries
    nobody annotated (a CAD file without models_info.json) are the same pose under ADI, where nms_poses without syms keeps both.
    thresh is a length in the unit of t, at least 0 (a fraction of the model's diameter is a good one); the other arguments as
    pair_adi and pose_nms have them.  -> (PoseNms, the (N,N) adi matrix, +inf where a pair was skipped).

    What is kept is what pose_nms keeps on the uncapped matrix.  The cap is thresh * (1 + 2^-20).  A skipped pair has adi_sum >=
    cap_sum + 1, and cap_sum + 1 is above the float64 product cap * inv_unit * 2^30 * V that floor() cut, which is off from the real
    product by a few units of 2^-53 relative.  The adi that pair_adi would report is fl32 of the float64 quotient adi_sum / 2^30 /
    inv_unit / V, again a few 2^-53 off: it is at least cap * (1 - 2^-50) > thresh, and rounding to float32 (2^-24) is monotone, so
    the reported adi is not below fl32(thresh), the number pose_nms compares with.  pose_nms asks err < thresh, strictly: +inf in the
    place of such an entry never changes an answer."""
    name = "nms_poses_adi"
    thresh = float(thresh)
    if not (thresh >= 0.0 and math.isfinite(thresh)):
        raise ValueError("%s: thresh = %r is not a finite number >= 0" % (name, thresh))
    adi = pair_adi(mesh_or_points, R, t, R, t, scale=scale, unit=unit, cap=thresh * (1.0 + ADI_NMS_MARGIN)).adi
    return pose_nms(adi, scores, thresh), adi


# ------------------------------------------------------------------------------------------------------------ VSD as a matrix
class PairVsd:
    """What pair_vsd returns; every tensor is on the device.  vsd (A,B,T) f32 and counts (A,B,4+T) i32 = n_union, n_inter, n_visib_est,
    n_visib_gt, cost_0 .. cost_{T-1}: row i the estimate a[i], column j the ground truth b[j].  n_render_a, n_visible_a (A) and
    n_render_b, n_visible_b (B) i32: per pose, the pixels its render covers and those of them that the depth image does not occlude."""

    def __init__(self, vsd, counts, n_render_a, n_visible_a, n_render_b, n_visible_b):
        self.vsd, self.counts = vsd, counts
        self.n_render_a, self.n_visible_a, self.n_render_b, self.n_visible_b = n_render_a, n_visible_a, n_render_b, n_visible_b


@on_tensor_device
def _pair_vsd(vertices, faces, view, A, intr, H, W, near, depth, delta, taus, inv_norm):
    B, T = int(view.shape[0]) - A, len(taus)
    # every view's own window; sam6d_pose_windows takes 1024 views a call
    box = torch.cat([verify._windows(vertices, faces, v, intr, H, W, near)[0] for v in (view[:A], view[A:])], dim=0).contiguous()
    offset, total = verify.window_offsets(box)
    total = int(total)  # the one read-back: 8 bytes, to size the workspace
    if total > MAX_VSD_WORDS:
        raise ValueError("pair_vsd: the windows of the %d + %d poses have %d words, above the cap of %d: split a or b" % (A, B, total, MAX_VSD_WORDS))
    need = int(_lib.load().sam6d_pose_pair_vsd_workspace_bytes(total, A, B))
    ws = _empty((need // 8,), vertices, torch.int64)
    counts, view_counts = _empty((A, B, 4 + T), vertices, torch.int32), _empty((A + B, 2), vertices, torch.int32)
    _lib.call("sam6d_pose_pair_vsd", _p(vertices), int(vertices.shape[0]), _p(faces), int(faces.shape[0]), _p(view), A, B, *intr, H, W, near, 0,
              _p(box), offset.data_ptr(), total, _p(depth), delta, _c_floats(taus), T, inv_norm, _p(counts), _p(view_counts), ws.data_ptr(),
              need, _s())
    return counts, view_counts


def pair_vsd(mesh, R_a, t_a, R_b, t_b, K, depth, delta, taus, diameter=None, scale=1.0, near=NEAR):
    """BOP's Visible Surface Discrepancy of every estimate a[i] against every ground truth b[j] of one object, for every tolerance in
    taus: for every (i, j), bit for bit, the counts poseerr.vsd gives for est = a[i], gt = b[j].

    a is the estimate and b the ground truth, and the roles are NOT symmetric: the ground truth's visibility is decided by the depth
    image alone, the estimate's also by the ground truth (BOP's `bop19` mode), so pair_vsd(.., a, b) is not the transpose of
    pair_vsd(.., b, a).
    mesh, K, depth, delta, taus, diameter, scale and near as poseerr.vsd has them.  R_a (A,3,3), t_a (A,3), R_b (B,3,3), t_b (B,3) f32
    HIP tensors, A and B at most 1024 each; the windows of all A + B poses together at most 2^28 pixels (a z-buffer of 2 GiB).
    Every pose is rendered once, into its own window; a pair costs a walk over the rectangle its two windows share and nothing at all
    when they do not meet (csrc/vsdpairs.hip has the recipe and why it gives poseerr.vsd's integers).
    -> PairVsd: vsd (A,B,T) f32 = (cost + n_union - n_inter) / n_union, 1 where nothing is visible; counts (A,B,4+T) i32; and per pose
    n_render_a, n_visible_a (A), n_render_b, n_visible_b (B) i32.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "pair_vsd"
    R_a, t_a = _poses(name, "a", R_a, t_a)
    R_b, t_b = _poses(name, "b", R_b, t_b)
    vertices, faces, R_a, t_a, depth, _, intr, H, W = verify._pose_args(name, mesh, R_a, t_a, K, depth, None, near)
    _same_device(name, vertices, (("R_b", R_b), ("t_b", t_b)))
    delta, taus, inv_norm = _tolerances(name, delta, taus, diameter)
    A = int(R_a.shape[0])
    view = torch.cat([verify.pose_views(R_a, t_a, scale), verify.pose_views(R_b, t_b, scale)], dim=0).contiguous()
    counts, per_view = _pair_vsd(vertices, faces, view, A, intr, H, W, float(near), depth, delta, taus, inv_norm)
    return PairVsd(vsd_from_counts(counts), counts, per_view[:A, 0], per_view[:A, 1], per_view[A:, 0], per_view[A:, 1])


def vsd_matches(vsd, scores, thresholds, valid=None, max_ests=0):
    """match_poses on a VSD matrix, once per misalignment tolerance: vsd (A,B,T) f32 HIP tensor (pair_vsd's), T 1 .. 16; scores,
    thresholds (BOP: 0.05 .. 0.5, the correctness thresholds on the error), valid and max_ests as match_poses has them.
    -> n_matched (T,K) i32 on the device, row k from match_poses(vsd[:, :, k], ..) with K the number of thresholds, and n_targets.
    instance_recall(n_matched, n_targets) is BOP's recall per (tau, threshold) and its mean over both axes AR_VSD.  A host loop of at
    most 16 launches; no kernel of its own.

    valid is where BOP's rule "targets at least 10 % visible" goes: pair_vsd's n_visible_b / n_render_b >= 0.1.  That ratio is BOP's
    visib_fract IN KIND: the package's rasteriser, and the silhouette inside the image as the denominator; it is not pinned against
    bop_toolkit.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "vsd_matches"
    vsd = _tensor(vsd, name, "vsd", torch.float32, (None, None, None))
    T = int(vsd.shape[2])
    if not 1 <= T <= MAX_TAUS:
        raise ValueError("%s: vsd: T = %d is not in 1 .. %d" % (name, T, MAX_TAUS))
    found = [match_poses(vsd[:, :, k].contiguous(), scores, thresholds, valid, max_ests) for k in range(T)]
    return torch.stack([m.n_matched for m in found], dim=0), found[0].n_targets
