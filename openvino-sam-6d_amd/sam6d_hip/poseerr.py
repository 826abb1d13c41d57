"""Scoring poses against ground truth on the device: the BOP pose errors MSSD, MSPD and VSD (Hodan et al., "BOP Challenge 2020 on
6D Object Localization") and ADD (Hinterstoisser et al. 2012), batched over N pose pairs.  The reference has no evaluation code -- it
writes its poses (PEM/run_inference_custom_pytorch.py:460-471) and leaves the scoring to bop_toolkit -- so the definitions are the
published ones, restated by the package: the recipe is at the top of csrc/poseerr.hip and restated in tests/poseerr_ref.py, and every
comparison with that restatement is bit for bit.  Nothing here is pinned against bop_toolkit itself.  VSD renders with the package's
own rasteriser (sam6d_hip.verify's raster pass), so it is BOP's in kind and not pixel for pixel.

The two quantities that need a search over all pairs of vertices are here too (csrc/nearest.hip, restated in tests/nearest_ref.py):
ADD-S / ADI without symmetries (adi; Hinterstoisser et al. 2012, Hodan et al. 2016) and the model diameter as bop_toolkit defines it,
the largest distance between two vertices (model_diameter, models_info).  Both are exact searches that skip tiles of points whose
bounding box cannot change the result; the bound holds in fp32 without a margin, so the pruned and the full search give the same bits.
ADI is evaluated over the vertices, as pose_errors is.

Left to the caller: symmetry-aware ADI, the index of the nearest vertex and of the diametral pair, ADI over surface samples, the
`tlinear` cost, other visibility modes, several meshes in one call, BOP's file formats, and the BOP threshold lists (recall and auc
take any).  The matching of estimates to ground-truth instances, which every function here takes as given, is sam6d_hip.posematch's.

Imports verify, runtime, _lib, torch and numpy only.  There is no CPU route: a CPU tensor raises RuntimeError.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, verify
from .runtime import _empty, _p, _s, on_tensor_device
from .verify import NEAR, _tensor

MAX_POINTS = 1 << 20
MAX_POSES = 1024
MAX_SYMS = 1024
MAX_PAIRS = 512     # vsd: 2 N views in one raster pass
MAX_TAUS = 16
ADD_SCALE = 2.0 ** 30
VSD_COLUMNS = ("n_union", "n_inter", "n_visib_est", "n_visib_gt")  # then cost_0 .. cost_{T-1}


class PoseErrors:
    """What pose_errors returns; every tensor is on the device.  mssd, mspd, add (N) f32 (mssd and add in the unit of t, mspd in
    pixels), mssd_sym, mspd_sym (N) i32 the symmetry that attains the minimum (the lowest on a tie), n_skipped (N) i32 the points
    that lie behind the camera under the estimate or the ground truth (symmetry 0) and take no part in mspd, add_sum (N) i64 the
    integer ADD is formed from."""

    def __init__(self, mssd, mspd, add, mssd_sym, mspd_sym, n_skipped, add_sum):
        self.mssd, self.mspd, self.add, self.mssd_sym, self.mspd_sym = mssd, mspd, add, mssd_sym, mspd_sym
        self.n_skipped, self.add_sum = n_skipped, add_sum


# ------------------------------------------------------------------------------------------------------------ symmetries
def _rotation(axis, angle):
    """Rodrigues' formula in float64"""
    a = np.asarray(axis, np.float64).reshape(3)
    norm = math.sqrt(float(a @ a))
    if not (norm > 0.0 and math.isfinite(norm)):
        raise ValueError("symmetry_transforms: continuous: axis %s has no direction" % (a.tolist(),))
    a = a / norm
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transforms(discrete=(), continuous=(), max_step=0.01):
    """The symmetry transforms of a model from its models_info.json entry, BOP's published construction (bop_toolkit's
    get_symmetry_transformations, restated): discrete = models_info's `symmetries_discrete` (each 16 numbers, a row-major 4 x 4
    matrix; a (4,4) or (3,4) array is taken too), continuous = its `symmetries_continuous` (each a dict with `axis` and `offset`).
    The identity is put before the discrete transforms; every continuous symmetry is sampled in ceil(pi / max_step) equal rotation
    steps about its axis through its offset (R_i, t_i = offset - R_i offset), and every discrete transform D is composed with every
    sample C as C o D.  Host numpy float64 -> (S,3,4) float32, the identity first.  More than 1024 transforms is refused."""
    name = "symmetry_transforms"
    if not (float(max_step) > 0.0 and math.isfinite(float(max_step))):
        raise ValueError("%s: max_step = %r is not a finite number > 0" % (name, max_step))
    disc = [np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)]
    for d in discrete:
        m = np.asarray(d, np.float64)
        if m.size == 16:
            m = m.reshape(4, 4)[:3]
        elif m.shape != (3, 4):
            raise ValueError("%s: discrete: a transform must have 16 numbers or shape (3,4), got shape %s" % (name, m.shape))
        disc.append(m.copy())
    steps = int(math.ceil(math.pi / float(max_step)))
    cont = []
    for c in continuous:
        if not (isinstance(c, dict) and "axis" in c and "offset" in c):
            raise ValueError("%s: continuous: each symmetry must be a dict with axis and offset" % name)
        off = np.asarray(c["offset"], np.float64).reshape(3, 1)
        for i in range(steps):
            R = _rotation(c["axis"], i * (2.0 * math.pi / steps))
            cont.append(np.concatenate([R, off - R @ off], axis=1))
    S = len(disc) * max(len(cont), 1)
    if S > MAX_SYMS:
        raise ValueError("%s: %d transforms (%d discrete with the identity x %d continuous samples) is above %d: raise max_step"
                         % (name, S, len(disc), len(cont), MAX_SYMS))
    out = []
    for d in disc:
        if not cont:
            out.append(d)
        for c in cont:
            out.append(np.concatenate([c[:, :3] @ d[:, :3], c[:, :3] @ d[:, 3:] + c[:, 3:]], axis=1))
    return np.stack(out).astype(np.float32)


def recall(err, thresholds):
    """The fraction of poses whose error is below each threshold: err (N) tensor, thresholds a sequence or tensor (K) -> (K) f32 on
    err's device.  A plain torch op; the BOP threshold lists (and the unit they are in) are the caller's."""
    if not torch.is_tensor(err) or err.dim() != 1 or err.numel() < 1:
        raise ValueError("recall: err must be an (N) tensor with N >= 1")
    thr = torch.as_tensor(thresholds, dtype=err.dtype, device=err.device).reshape(-1)
    return (err[None, :] < thr[:, None]).to(torch.float32).mean(dim=1)


def auc(err, max_err):
    """The area under the recall-over-threshold curve on [0, max_err], as a fraction of max_err (YCB-V's AUC of ADD(-S) with
    max_err = 0.1 m): err (N) tensor -> a 0-dim f64 tensor on err's device, mean(clamp(max_err - err, min=0)) / max_err.  A NaN error
    counts as a miss.  A plain torch op."""
    if not torch.is_tensor(err) or err.dim() != 1 or err.numel() < 1:
        raise ValueError("auc: err must be an (N) tensor with N >= 1")
    max_err = float(max_err)
    if not (max_err > 0.0 and math.isfinite(max_err)):
        raise ValueError("auc: max_err = %r is not a finite number > 0" % max_err)
    return torch.nan_to_num(torch.clamp(max_err - err.to(torch.float64), min=0.0), nan=0.0).mean() / max_err


# ------------------------------------------------------------------------------------------------------------ point errors
def _points(name, mesh_or_points, like):
    """(V,3) f32 contiguous: a tensor, a mesh dict (numpy or tensors; uploaded beside `like` when it is not a tensor) or a
    (vertices, faces) pair"""
    x = mesh_or_points
    if isinstance(x, dict):
        x = x["vertices"]
        if not torch.is_tensor(x):
            if not (torch.is_tensor(like) and like.is_cuda):
                raise RuntimeError("%s: needs HIP device tensors (this build has no CPU path)" % name)
            x = torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(like.device)
    elif isinstance(x, (tuple, list)) and len(x) == 2:
        x = x[0]
    x = _tensor(x, name, "points", torch.float32, (None, 3))
    if not 1 <= int(x.shape[0]) <= MAX_POINTS:
        raise ValueError("%s: points: V = %d is not in 1 .. %d" % (name, int(x.shape[0]), MAX_POINTS))
    return x


def _intrinsics(name, K):
    try:
        return verify._intrinsics(K)
    except ValueError as e:
        raise ValueError(str(e).replace("render_compare", name)) from None


def _pair(name, R_est, t_est, R_gt, t_gt, limit):
    if not torch.is_tensor(R_est) or R_est.dim() != 3:
        raise ValueError("%s: R_est must be an (N,3,3) float32 tensor" % name)
    N = int(R_est.shape[0])
    R_est, t_est = _tensor(R_est, name, "R_est", torch.float32, (N, 3, 3)), _tensor(t_est, name, "t_est", torch.float32, (N, 3))
    R_gt, t_gt = _tensor(R_gt, name, "R_gt", torch.float32, (N, 3, 3)), _tensor(t_gt, name, "t_gt", torch.float32, (N, 3))
    if not 1 <= N <= limit:
        raise ValueError("%s: N = %d is not in 1 .. %d" % (name, N, limit))
    return N, R_est, t_est, R_gt, t_gt


def _same_device(name, first, rest):
    for what, x in rest:
        if x.device != first.device:
            if not (x.is_cuda and first.is_cuda):
                raise RuntimeError("%s: needs HIP device tensors (%s is on %s, the model on %s; this build has no CPU path)"
                                   % (name, what, x.device, first.device))
            raise ValueError("%s: %s is on %s and the model on %s" % (name, what, x.device, first.device))


def _inv_unit(name, unit):
    """1 / unit as the float32 the kernels count in (None: 1)"""
    unit = 1.0 if unit is None else float(unit)
    if not (unit > 0.0 and math.isfinite(unit)):
        raise ValueError("%s: unit = %r is not a finite number > 0" % (name, unit))
    inv_unit = float(np.float32(1.0 / unit))
    if not (inv_unit > 0.0 and math.isfinite(inv_unit)):
        raise ValueError("%s: unit = %r: 1 / unit is not a finite float32 > 0" % (name, unit))
    return inv_unit


def _syms(name, syms, points, limit=MAX_SYMS):
    """(S,3,4) f32 beside the points: None is the identity alone, a host array is uploaded"""
    if syms is None:
        syms = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None].astype(np.float32)
    host = None if torch.is_tensor(syms) else np.asarray(syms)
    syms = _tensor(syms if host is None else torch.from_numpy(np.ascontiguousarray(host)), name, "syms", torch.float32, (None, 3, 4))
    if not 1 <= int(syms.shape[0]) <= limit:
        raise ValueError("%s: syms: S = %d is not in 1 .. %d" % (name, int(syms.shape[0]), limit))
    if host is not None:
        if not points.is_cuda:
            raise RuntimeError("%s: needs HIP device tensors (this build has no CPU path)" % name)
        syms = syms.to(points.device)
    return syms


def _errors(cls, entry, points, shape, poses, syms, intr, inv_unit, flags=()):
    """One call of sam6d_pose_point_errors or sam6d_pose_pair_errors -> cls: the outputs have `shape` ((N) or (A,B)), `poses` are the
    entry's pose arguments.  intr None (the pair entry alone): no mspd, mspd_sym, n_skipped"""
    V, S = int(points.shape[0]), int(syms.shape[0])
    need = int(getattr(_lib.load(), entry + "_workspace_bytes")(*shape, S))
    ws = _empty((need // 8,), points, torch.int64)
    mssd, mssd_sym = _empty(shape, points), _empty(shape, points, torch.int32)
    add_sum = _empty(shape, points, torch.int64)
    mspd = mspd_sym = skipped = None
    if intr is not None:
        mspd, mspd_sym, skipped = _empty(shape, points), _empty(shape, points, torch.int32), _empty(shape, points, torch.int32)
    _lib.call(entry, _p(points), V, *poses, _p(syms), S, *(intr or (0.0, 0.0, 0.0, 0.0)), inv_unit, *flags, _p(mssd), _p(mspd), _p(mssd_sym),
              _p(mspd_sym), _p(skipped), add_sum.data_ptr(), ws.data_ptr(), need, _s())
    add = (add_sum.to(torch.float64) / ADD_SCALE / inv_unit / V).to(torch.float32)
    return cls(mssd, mspd, add, mssd_sym, mspd_sym, skipped, add_sum)


@on_tensor_device
def _point_errors(points, est, gt, syms, intr, inv_unit):
    N = int(est.shape[0])
    return _errors(PoseErrors, "sam6d_pose_point_errors", points, (N,), (_p(est), _p(gt), N), syms, intr, inv_unit)


def pose_errors(mesh_or_points, R_est, t_est, R_gt, t_gt, K, syms=None, scale=1.0, unit=None):
    """MSSD, MSPD and ADD of N estimated poses against their ground truths, over the model's vertices.

    mesh_or_points: (V,3) f32 HIP tensor of model vertices in CAD units, a mesh dict as onboard.load_mesh returns, or a
    (vertices, faces) pair.  R_est, R_gt (N,3,3), t_est, t_gt (N,3) f32 HIP tensors.  K: one 3 x 3 matrix or (fx, fy, cx, cy).
    syms: (S,3,4) f32 symmetry transforms in CAD units (symmetry_transforms; numpy or a HIP tensor), None for the identity alone.
    scale: CAD units into the unit of t (0.001 for a millimetre model under metre poses), as verify.pose_views.  unit: the length ADD's
    integer sum counts in, in the unit of t (the model's diameter is a good one; None: 1); a point farther than 4096 units from its
    ground truth counts as 4096.

    -> PoseErrors.  mssd = min over symmetries of the max over vertices of |est x - gt S x|, mspd the same with the pixel distance of
    the two projections, add = the mean of |est x - gt x| (symmetry 0 alone).  A vertex behind the camera under either pose takes no
    part in mspd and is counted in n_skipped (for symmetry 0): check that it is 0 before trusting mspd.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "pose_errors"
    N, R_est, t_est, R_gt, t_gt = _pair(name, R_est, t_est, R_gt, t_gt, MAX_POSES)
    points = _points(name, mesh_or_points, R_est)
    intr = _intrinsics(name, K)
    inv_unit = _inv_unit(name, unit)
    syms = _syms(name, syms, points)
    _same_device(name, points, (("R_est", R_est), ("t_est", t_est), ("R_gt", R_gt), ("t_gt", t_gt), ("syms", syms)))
    return _point_errors(points, verify.pose_views(R_est, t_est, scale), verify.pose_views(R_gt, t_gt, scale), syms, intr, inv_unit)


# ------------------------------------------------------------------------------------------------------------ ADI, the diameter
class AdiErrors:
    """What adi returns; both tensors are on the device.  adi (N) f32 in the unit of t, adi_sum (N) i64 the integer it is formed
    from."""

    def __init__(self, adi, adi_sum):
        self.adi, self.adi_sum = adi, adi_sum


def _spread10(q):
    """the 10 low bits of an i64 tensor to every third bit"""
    q = (q | (q << 16)) & 0x30000FF
    q = (q | (q << 8)) & 0x300F00F
    q = (q | (q << 4)) & 0x30C30C3
    return (q | (q << 2)) & 0x9249249


def morton_order(points):
    """(V,3) f32 -> (V) i64, the points' order along a Morton curve: 10 bits per axis over the bounding box (one step for all three
    axes, the longest side's, so that the cells are cubes), interleaved, a stable argsort.  Plain torch ops.  Consecutive points are
    then neighbours in space, so the kernels' tiles of 256 are compact and their boxes prune; the order is plumbing, no result depends
    on it.  A coordinate that is not finite counts as 0."""
    x = torch.nan_to_num(points, nan=0.0, posinf=0.0, neginf=0.0)
    lo = x.min(dim=0).values
    span = (x.max(dim=0).values - lo).max().clamp_min(1e-30)
    q = ((x - lo) / span * 1023.0).clamp(0.0, 1023.0).to(torch.int64)
    return torch.argsort(_spread10(q[:, 0]) | (_spread10(q[:, 1]) << 1) | (_spread10(q[:, 2]) << 2), stable=True)


def _adi_of(adi_sum, inv_unit, V):
    """adi from its integer sum, the one copy of the expression (adi here, posematch.pair_adi): f32 in the unit of t"""
    return (adi_sum.to(torch.float64) / ADD_SCALE / inv_unit / V).to(torch.float32)


@on_tensor_device
def _adi(points, est, gt, inv_unit, sort, prune):
    V, N = int(points.shape[0]), int(est.shape[0])
    if sort:
        points = points[morton_order(points)].contiguous()
    need = int(_lib.load().sam6d_pose_adi_workspace_bytes(V, N))
    ws = _empty((need // 8,), points, torch.int64)
    adi_sum = _empty((N,), points, torch.int64)
    _lib.call("sam6d_pose_adi", _p(points), V, _p(est), _p(gt), N, inv_unit, 0 if prune else 1, adi_sum.data_ptr(), ws.data_ptr(), need, _s())
    return AdiErrors(_adi_of(adi_sum, inv_unit, V), adi_sum)


def adi(mesh_or_points, R_est, t_est, R_gt, t_gt, scale=1.0, unit=None, sort=True, prune=True):
    """ADD-S / ADI of N estimated poses against their ground truths, over the model's vertices: the mean over the vertices of the
    distance from a vertex under the estimate to the NEAREST vertex under the ground truth, the error for an object whose symmetries
    make ADD meaningless.  No symmetry transforms are applied.

    mesh_or_points, R_est, t_est, R_gt, t_gt, scale and unit as pose_errors has them (there is no K); a nearest distance above 4096
    units counts as 4096, and so does a vertex with no nearest distance (a NaN in the pose).  sort: order the vertices along a Morton
    curve first (morton_order), so that the search's tiles are compact; prune: skip the tiles whose box cannot hold a nearer vertex.
    Neither changes a bit of the result; prune=False is the full V x V walk.
    -> AdiErrors: adi (N) f32 in the unit of t, adi_sum (N) i64.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "adi"
    N, R_est, t_est, R_gt, t_gt = _pair(name, R_est, t_est, R_gt, t_gt, MAX_POSES)
    points = _points(name, mesh_or_points, R_est)
    inv_unit = _inv_unit(name, unit)
    _same_device(name, points, (("R_est", R_est), ("t_est", t_est), ("R_gt", R_gt), ("t_gt", t_gt)))
    return _adi(points, verify.pose_views(R_est, t_est, scale), verify.pose_views(R_gt, t_gt, scale), inv_unit, bool(sort), bool(prune))


@on_tensor_device
def _diameter(points, sort, prune):
    if sort:
        points = points[morton_order(points)].contiguous()
    V = int(points.shape[0])
    seeds = torch.cat([points.argmin(dim=0), points.argmax(dim=0)]).to(torch.int32)  # the extreme vertex of each axis, both ends
    need = int(_lib.load().sam6d_points_diameter_workspace_bytes(V))
    ws = _empty((need // 8,), points, torch.int64)
    out = _empty((1,), points)
    _lib.call("sam6d_points_diameter", _p(points), V, _p(seeds), int(seeds.numel()), 0 if prune else 1, _p(out), ws.data_ptr(), need, _s())
    return out.reshape(())


def _model_points(name, mesh_or_points):
    """_points for the calls without a pose: a numpy mesh goes to the current HIP device"""
    like = torch.empty(0, device="cuda") if torch.cuda.is_available() else None
    return _points(name, mesh_or_points, like)


def model_diameter(mesh_or_points, sort=True, prune=True):
    """The model's diameter as bop_toolkit defines it, the largest distance between two of its vertices, by an exact search over all
    pairs: mesh_or_points as pose_errors has it -> a 0-dim f32 tensor on the device, in CAD units.  NaN where a coordinate is not
    finite.  sort and prune as adi has them: neither changes a bit of the result.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    return _diameter(_model_points("model_diameter", mesh_or_points), bool(sort), bool(prune))


def _extent(points):
    """(V,3) -> (6) min_x, min_y, min_z, size_x, size_y, size_z; plain torch ops"""
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    return torch.cat([lo, hi - lo])


INFO_FIELDS = ("diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z")


def models_info(mesh_or_points):
    """The geometric fields of a BOP models_info.json entry for a model that has none (a CAD file onboard.load_mesh read): diameter
    (model_diameter) and min_x, min_y, min_z, size_x, size_y, size_z (the bounding box; plain torch ops), a dict of Python floats in
    CAD units.  One read-back of 28 bytes.  Symmetries are not detected."""
    points = _model_points("models_info", mesh_or_points)
    row = torch.cat([_diameter(points, True, True).reshape(1), _extent(points)]).cpu()
    return dict(zip(INFO_FIELDS, (float(v) for v in row)))


# ------------------------------------------------------------------------------------------------------------ VSD
def union_boxes(box_a, box_b):
    """(N,4) i32 [x0, y0, x1, y1] inclusive boxes -> the smallest box that holds both; an empty box (x1 < x0 or y1 < y0) is neutral,
    two empty ones give [0, 0, -1, -1]"""
    big = torch.iinfo(torch.int32).max
    ea = ((box_a[:, 2] < box_a[:, 0]) | (box_a[:, 3] < box_a[:, 1]))[:, None]
    eb = ((box_b[:, 2] < box_b[:, 0]) | (box_b[:, 3] < box_b[:, 1]))[:, None]
    lo = torch.minimum(torch.where(ea, big, box_a[:, :2]), torch.where(eb, big, box_b[:, :2]))
    hi = torch.maximum(torch.where(ea, -1, box_a[:, 2:]), torch.where(eb, -1, box_b[:, 2:]))
    lo = torch.where(ea & eb, 0, lo)
    return torch.cat([lo, hi], dim=1).to(torch.int32).contiguous()


@on_tensor_device
def _vsd(vertices, faces, view, intr, H, W, near, depth, delta, taus, inv_norm):
    N, T = int(view.shape[0]) // 2, len(taus)
    box, _ = verify._windows(vertices, faces, view, intr, H, W, near)
    both = union_boxes(box[:N], box[N:])
    box = torch.cat([both, both], dim=0).contiguous()
    offset, total = verify.window_offsets(box)
    total = int(total)  # the one read-back: 8 bytes, to size the workspace
    need = int(_lib.load().sam6d_pose_vsd_workspace_bytes(total, N))
    ws = _empty((need // 8,), vertices, torch.int64)
    counts = _empty((N, 4 + T), vertices, torch.int32)
    _lib.call("sam6d_pose_vsd", _p(vertices), int(vertices.shape[0]), _p(faces), int(faces.shape[0]), _p(view), N, *intr, H, W, near, 0,
              _p(box), offset.data_ptr(), total, _p(depth), delta, _c_floats(taus), T, inv_norm, _p(counts), ws.data_ptr(), need, _s())
    return counts


def _c_floats(values):
    """the host array of floats an entry reads its taus from"""
    return (ctypes.c_float * len(values))(*values)


def vsd_from_counts(counts):
    """counts (..., 4+T) i32 of sam6d_pose_vsd or sam6d_pose_pair_vsd ((N, 4+T) or (A, B, 4+T)) -> vsd (..., T) f32 =
    (cost_k + n_union - n_inter) / n_union, 1 where n_union is 0"""
    union = counts[..., 0:1]
    num = (counts[..., 4:] + (union - counts[..., 1:2])).to(torch.float32)
    return torch.where(union > 0, num / union.to(torch.float32), torch.ones_like(num))


def _tolerances(name, delta, taus, diameter):
    """delta, taus and diameter of vsd and posematch.pair_vsd, checked -> delta, the list of taus, inv_norm"""
    delta = float(delta)
    if not (delta >= 0.0 and math.isfinite(delta)):
        raise ValueError("%s: delta = %r is not a finite number >= 0" % (name, delta))
    taus = [float(v) for v in np.asarray(taus.cpu() if torch.is_tensor(taus) else taus, np.float64).reshape(-1)]
    if not 1 <= len(taus) <= MAX_TAUS:
        raise ValueError("%s: taus: T = %d is not in 1 .. %d" % (name, len(taus), MAX_TAUS))
    if not all(v >= 0.0 and math.isfinite(v) for v in taus):
        raise ValueError("%s: taus = %r: every one must be a finite number >= 0" % (name, taus))
    inv_norm = 1.0
    if diameter is not None:
        if not (float(diameter) > 0.0 and math.isfinite(float(diameter))):
            raise ValueError("%s: diameter = %r is not a finite number > 0" % (name, diameter))
        inv_norm = float(np.float32(1.0 / float(diameter)))
    return delta, taus, inv_norm


def vsd(mesh, R_est, t_est, R_gt, t_gt, K, depth, delta, taus, diameter=None, scale=1.0, near=NEAR):
    """BOP's Visible Surface Discrepancy of N estimated poses against their ground truths, for every misalignment tolerance in taus.

    mesh, K, depth, scale and near as verify.render_compare has them; R_est, R_gt (N,3,3), t_est, t_gt (N,3) f32 HIP tensors, N at most
    512.  delta: the visibility tolerance in the unit of t (BOP: 15 mm).  taus: 1 .. 16 numbers >= 0; with diameter (in the unit of t)
    they are fractions of it (BOP: 0.05 .. 0.5), without in the unit of t.

    Both poses of a pair are rendered into one window (the union of their boxes); per pixel the distances from the camera centre of
    the two renders and of the depth image decide what is visible (BOP's `bop19` mode: a pixel without a depth reading is visible) and
    the `step` cost counts the pixels visible in both whose distances differ by tau or more.
    -> vsd (N,T) f32 = (cost + n_union - n_inter) / n_union, 1 where nothing is visible, and counts (N, 4+T) i32 = n_union, n_inter,
    n_visib_est, n_visib_gt, cost_0 .. cost_{T-1}.
    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "vsd"
    vertices, faces, R_est, t_est, depth, _, intr, H, W = verify._pose_args(name, mesh, R_est, t_est, K, depth, None, near)
    N, R_est, t_est, R_gt, t_gt = _pair(name, R_est, t_est, R_gt, t_gt, MAX_PAIRS)
    _same_device(name, vertices, (("R_gt", R_gt), ("t_gt", t_gt)))
    delta, taus, inv_norm = _tolerances(name, delta, taus, diameter)
    view = torch.cat([verify.pose_views(R_est, t_est, scale), verify.pose_views(R_gt, t_gt, scale)], dim=0).contiguous()
    counts = _vsd(vertices, faces, view, intr, H, W, float(near), depth, delta, taus, inv_norm)
    return vsd_from_counts(counts), counts
