"""Checking poses against the depth image the scene was measured with: the CAD model rendered at each pose, compared with the
observed depth pixel by pixel.  The reference has no such check -- it multiplies the detection score by the PEM score
(PEM/run_inference_custom_pytorch.py:460-471) and draws the top pose as a box and 512 points (:480-482) -- so the classes, the
tolerance and the ratios are the package's own.  The geometry is the template renderer's (csrc/raster.hip through raster.h): a pixel's
coverage and depth are what onboard.render_views gives for the same view, bit for bit.  Each pose is rendered into a window of its
own, so the memory is the sum of the windows (8 bytes per pixel) and not poses x image; the recipe is at the top of csrc/verify.hip
and restated in tests/verify_ref.py.

No combined score and no thresholds are built in: render_compare returns counts and ratios, and the caller decides.

Imports runtime, _lib, torch and numpy only.  There is no CPU route: a CPU tensor raises RuntimeError.
"""
import math

import numpy as np
import torch

from . import _lib
from .runtime import _empty, _p, _s, on_tensor_device

MAX_SIZE = 2048    # H, W
MAX_POSES = 1024
MAX_FACES = 1 << 24
NEAR = 1.0e-3      # in the unit of t, as onboard.NEAR
TOL = 0.01         # in the unit of t: one centimetre under PEM's metre poses
COLUMNS = ("n_render", "n_inlier", "n_occluded", "n_behind", "n_unknown", "n_mask", "n_inter", "n_dropped")


class PoseCheck:
    """What render_compare returns; every tensor is on the device.
    counts (N,8) i32 in the order of COLUMNS, boxes (N,4) i32 [x0, y0, x1, y1] inclusive ([0, 0, -1, -1]: nothing rendered),
    inlier_ratio, behind_ratio, occluded_ratio, unknown_ratio (N) f32, mask_iou (N) f32 or None, ids (H,W) i32 and depth (H,W) f32
    or None."""

    def __init__(self, counts, boxes, mask_iou, ids, depth):
        self.counts, self.boxes, self.mask_iou, self.ids, self.depth = counts, boxes, mask_iou, ids, depth
        n = counts[:, 0].to(torch.float32)
        some = counts[:, 0] > 0

        def ratio(col):
            return torch.where(some, counts[:, col].to(torch.float32) / n, torch.zeros_like(n))

        self.inlier_ratio, self.occluded_ratio, self.behind_ratio, self.unknown_ratio = ratio(1), ratio(2), ratio(3), ratio(4)

    def __getattr__(self, name):  # n_render ... n_dropped: the columns of counts
        if name in COLUMNS:
            return self.counts[:, COLUMNS.index(name)]
        raise AttributeError(name)


def _tensor(x, name, what, dtype, shape):
    """a contiguous tensor of this dtype and shape (None in `shape`: any length); the device is checked by the launch"""
    if not torch.is_tensor(x):
        raise ValueError("%s: %s must be a torch tensor, got %s" % (name, what, type(x).__name__))
    if x.dtype != dtype:
        raise ValueError("%s: %s must be %s, got %s" % (name, what, dtype, x.dtype))
    if x.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(x.shape, shape)):
        raise ValueError("%s: %s must have shape %s, got %s" % (name, what, tuple("*" if s is None else s for s in shape), tuple(x.shape)))
    return x.contiguous()


def pose_views(R, t, scale=1.0):
    """The (N,3,4) f32 object-to-camera matrices of N poses on the device: M[:, :, :3] = R * fl32(scale), M[:, :, 3] = t.  R (N,3,3)
    and t (N,3) f32 tensors (PEM's pred_R and pred_t); scale turns CAD units into the unit of t: 0.001 for a millimetre model under
    PEM's metre poses."""
    if not torch.is_tensor(R) or R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.dtype != torch.float32:
        raise ValueError("pose_views: R must be an (N,3,3) float32 tensor")
    N = int(R.shape[0])
    if not torch.is_tensor(t) or tuple(t.shape) != (N, 3) or t.dtype != torch.float32:
        raise ValueError("pose_views: t must be an (%d,3) float32 tensor" % N)
    if t.device != R.device:
        raise ValueError("pose_views: R is on %s and t on %s" % (R.device, t.device))
    return torch.cat([R * float(np.float32(scale)), t.reshape(N, 3, 1)], dim=2).contiguous()


def _intrinsics(K):
    """(fx, fy, cx, cy) from one 3 x 3 matrix or from the four numbers"""
    k = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    k = np.asarray(k, np.float64)
    if k.shape == (1, 3, 3):
        k = k[0]
    if k.shape == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if k.shape == (4,):
        return tuple(float(v) for v in k)
    raise ValueError("render_compare: K must be one 3 x 3 matrix or (fx, fy, cx, cy), got shape %s" % (k.shape,))


@on_tensor_device
def _windows(vertices, faces, view, intr, H, W, near):
    N = int(view.shape[0])
    box, dropped = _empty((N, 4), vertices, torch.int32), _empty((N,), vertices, torch.int32)
    _lib.call("sam6d_pose_windows", _p(vertices), int(vertices.shape[0]), _p(faces), int(faces.shape[0]), _p(view), N, *intr, H, W, near,
              _p(box), _p(dropped), _s())
    return box, dropped


def pose_windows(vertices, faces, view, intrinsics, size, near=NEAR):
    """sam6d_pose_windows: vertices (V,3) f32, faces (F,3) i32, view (N,3,4) f32 HIP tensors, intrinsics (fx, fy, cx, cy), size (H, W)
    -> box (N,4) i32 [x0, y0, x1, y1] inclusive ([0, 0, -1, -1] for a pose that covers nothing), n_dropped (N) i32."""
    name = "pose_windows"
    vertices, faces = _tensor(vertices, name, "vertices", torch.float32, (None, 3)), _tensor(faces, name, "faces", torch.int32, (None, 3))
    view = _tensor(view, name, "view", torch.float32, (None, 3, 4))
    H, W = _size(name, size, int(view.shape[0]), int(faces.shape[0]), int(vertices.shape[0]))
    return _windows(vertices, faces, view, tuple(float(v) for v in intrinsics), H, W, float(near))


def _size(name, size, N, F, V):
    H, W = int(size[0]), int(size[1])
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError("%s: H x W = %d x %d is not in 1 .. %d" % (name, H, W, MAX_SIZE))
    if not 1 <= N <= MAX_POSES:
        raise ValueError("%s: N = %d is not in 1 .. %d" % (name, N, MAX_POSES))
    if not 1 <= F <= MAX_FACES or V < 1:
        raise ValueError("%s: a mesh of %d vertices and %d faces (F must be in 1 .. %d)" % (name, V, F, MAX_FACES))
    return H, W


def window_offsets(box):
    """box (N,4) i32 [x0, y0, x1, y1] inclusive -> offset (N+1) i64 on the device: the first z-buffer word of each pose's window, and
    in offset[N] the words of all windows together (still on the device: reading it back is the caller's)"""
    N = int(box.shape[0])
    bw = (box[:, 2] - box[:, 0] + 1).clamp_(min=0).to(torch.int64)
    bh = (box[:, 3] - box[:, 1] + 1).clamp_(min=0).to(torch.int64)
    offset = torch.zeros((N + 1,), dtype=torch.int64, device=box.device)
    torch.cumsum(bw * bh, dim=0, out=offset[1:])
    return offset, offset[N]


@on_tensor_device
def _verify(vertices, faces, view, intr, H, W, near, wave_area, box, depth, masks, tau, want_map):
    N = int(view.shape[0])
    offset, total = window_offsets(box)
    total = int(total)  # the one read-back: 8 bytes, to size the workspace
    need = int(_lib.load().sam6d_pose_verify_workspace_bytes(total, H, W))
    ws = _empty((need // 8,), vertices, torch.int64)
    counts = _empty((N, 8), vertices, torch.int32)
    ids = _empty((H, W), vertices, torch.int32) if want_map else None
    out = _empty((H, W), vertices) if want_map else None
    _lib.call("sam6d_pose_verify", _p(vertices), int(vertices.shape[0]), _p(faces), int(faces.shape[0]), _p(view), N, *intr, H, W, near,
              wave_area, _p(box), offset.data_ptr(), total, _p(depth), masks.data_ptr() if masks is not None else None, tau, _p(counts),
              _p(ids), _p(out), ws.data_ptr(), need, _s())
    return counts, ids, out


def _pose_args(name, mesh, R, t, K, depth, masks, near):
    """The arguments render_compare and refine.refine_poses share, checked and made contiguous
    -> vertices, faces, R, t, depth, masks, intr, H, W.  A wrong shape or dtype raises ValueError naming the argument."""
    if isinstance(mesh, dict):
        from .onboard import _mesh_tensors
        v = mesh["vertices"]
        dev = v.device if torch.is_tensor(v) else (R.device if torch.is_tensor(R) else None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError("%s: needs HIP device tensors (this build has no CPU path)" % name)
        vertices, faces = _mesh_tensors(mesh, dev)[:2]
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        vertices, faces = mesh
    else:
        raise ValueError("%s: mesh must be a dict with vertices and faces or a (vertices, faces) pair" % name)
    vertices, faces = _tensor(vertices, name, "vertices", torch.float32, (None, 3)), _tensor(faces, name, "faces", torch.int32, (None, 3))
    if not torch.is_tensor(R) or R.dim() != 3:
        raise ValueError("%s: R must be an (N,3,3) float32 tensor" % name)
    N = int(R.shape[0])
    R, t = _tensor(R, name, "R", torch.float32, (N, 3, 3)), _tensor(t, name, "t", torch.float32, (N, 3))
    depth = _tensor(depth, name, "depth", torch.float32, (None, None))
    H, W = _size(name, depth.shape, N, int(faces.shape[0]), int(vertices.shape[0]))
    if masks is not None:
        if not torch.is_tensor(masks) or masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError("%s: masks must be an (N,H,W) uint8 or bool tensor" % name)
        masks = _tensor(masks, name, "masks", masks.dtype, (N, H, W))
    intr = _intrinsics(K)
    if not float(near) > 0.0:
        raise ValueError("%s: near = %r is not positive" % (name, near))
    for what, x in (("faces", faces), ("R", R), ("t", t), ("depth", depth), ("masks", masks)):
        if x is not None and x.device != vertices.device:
            if not (x.is_cuda and vertices.is_cuda):
                raise RuntimeError("%s: needs HIP device tensors (%s is on %s, vertices on %s; this build has no CPU path)"
                                   % (name, what, x.device, vertices.device))
            raise ValueError("%s: %s is on %s and vertices on %s" % (name, what, x.device, vertices.device))
    return vertices, faces, R, t, depth, masks, intr, H, W


def render_compare(mesh, R, t, K, depth, masks=None, tol=TOL, scale=1.0, near=NEAR, wave_area=0, want_map=True):
    """Renders the model at each of N poses and compares every rendered pixel with the observed depth.

    mesh: what onboard.load_mesh returns (a dict with vertices and faces, numpy or tensors; uploaded when it is not on the device), or
    a (vertices (V,3) f32, faces (F,3) i32) pair of HIP tensors.  R (N,3,3), t (N,3) f32 HIP tensors: the poses (pose_views).  K: one
    3 x 3 matrix or (fx, fy, cx, cy).  depth (H,W) f32 HIP tensor in the unit of t (metres, as get_test_data forms it: depth *
    depth_scale / 1000).  masks (N,H,W) u8 or bool HIP tensor, mask n beside pose n, or None.  tol: the depth tolerance in the unit of
    t.  scale: CAD units into the unit of t (0.001 for a millimetre model).  near: faces with a vertex nearer than this are dropped
    whole and counted (there is no clipper).  wave_area: as onboard.render_views.  want_map: also composite all poses into ids / depth.

    -> PoseCheck.  Per pose, over the pixels its render covers (n_render):
      inlier_ratio    the observed depth is within tol of the rendered one: the surface is where the pose says
      behind_ratio    the observed depth is farther by more than tol: the camera sees THROUGH where the model should be -- evidence
                      against the pose
      occluded_ratio  the observed depth is nearer by more than tol: something stands in front -- an occluder, or a pose too deep
      unknown_ratio   the sensor has no depth there (0, negative or NaN)
      mask_iou        n_inter / (n_render + n_mask - n_inter) of the render against masks[n]; None without masks
    each float32 true division, 0 where the denominator is 0; counts holds the integers, boxes the windows, and ids / depth the
    instance map (the nearest pose per pixel, on a tie the lower index; -1 / 0 = background).  Nothing is thresholded or combined
    into one score here: which ratios matter, and how much, is the caller's decision.

    A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "render_compare"
    vertices, faces, R, t, depth, masks, intr, H, W = _pose_args(name, mesh, R, t, K, depth, masks, near)
    N = int(R.shape[0])
    tol = float(tol)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError("%s: tol = %r is not a finite number >= 0" % (name, tol))
    if int(wave_area) < 0:
        raise ValueError("%s: wave_area = %d is negative" % (name, int(wave_area)))
    view = pose_views(R, t, scale)
    box, dropped = _windows(vertices, faces, view, intr, H, W, float(near))
    counts, ids, out = _verify(vertices, faces, view, intr, H, W, float(near), int(wave_area), box, depth, masks, tol, bool(want_map))
    counts[:, 7] = dropped  # the windows' count: the same number, and also there when no pose has a window
    iou = None
    if masks is not None:
        union = counts[:, 0] + counts[:, 5] - counts[:, 6]
        zero = torch.zeros((N,), dtype=torch.float32, device=counts.device)
        iou = torch.where(union > 0, counts[:, 6].to(torch.float32) / union.to(torch.float32), zero)
    return PoseCheck(counts, box, iou, ids, out)
