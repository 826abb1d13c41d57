"""Refining poses against the depth image the scene was measured with: projective point-to-plane Gauss-Newton steps on the device,
batched over all poses.  The reference has no refinement -- its poses leave PEM's weighted SVD as they are
(PEM/run_inference_custom_pytorch.py:460-471) -- so the method, its gates and its status codes are the package's own, and it is
opt-in: nothing else in the package calls it.  The geometry is verify's: each pose is rendered into a window of its own with the
raster pass of verify.render_compare, every rendered pixel with an observed depth within `gate` of the rendered one is a pair, the
pairs' normal equations are summed as integers and solved per pose in float64.  The recipe is at the top of csrc/refine.hip and
restated in tests/refine_ref.py; the result is a function of the inputs alone.

The windows are those of the initial poses, grown by `margin` pixels, and stay fixed: what moves out of its window is not seen.

Imports verify, runtime, _lib, torch and numpy only.  There is no CPU route: a CPU tensor raises RuntimeError.
"""
import math

import numpy as np
import torch

from . import _lib, verify
from .runtime import _empty, _p, _s, on_tensor_device

STATUS = ("stepped", "too few pairs", "singular", "step refused", "no window")
FRACTION_BITS = 30  # the sums are integers in units of 2^-30 (csrc/refine.hip)


class PoseRefinement:
    """What refine_poses returns; every tensor is on the device.
    R (N,3,3), t (N,3) f32: the refined poses (the float64 state rounded once).  n_pairs (N) i32, rms (N) f32 and status (N) i32: the
    pairs of the last iteration, the root mean square of their point-to-plane residuals in the unit of t BEFORE that iteration's step,
    and its status code (an index into STATUS; with any but 0 that iteration left the pose as it was).  history (N, iters, 2) f32:
    n_pairs and rms of every iteration.  boxes (N,4) i32: the windows.  The squared residuals are summed in units of 2^-30 model radii
    squared, so a residual below 2^-15.5 radii adds nothing: on noise-free depth rms can read 0 at convergence."""

    def __init__(self, R, t, n_pairs, rms, status, history, boxes):
        self.R, self.t, self.n_pairs, self.rms, self.status, self.history, self.boxes = R, t, n_pairs, rms, status, history, boxes


def mesh_radius2(vertices):
    """max over the vertices of (x x + y y) + z z in float32, one rounding per operation: a device scalar"""
    x, y, z = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    return ((x * x + y * y) + z * z).max()


def inv_unit(radius2, scale):
    """float32(1 / (sqrt(radius2) * |scale|)) with the arithmetic in float64: what refine_poses passes to the step"""
    return float(np.float32(1.0 / (math.sqrt(float(radius2)) * abs(float(np.float32(scale))))))


def grow_boxes(box, margin, H, W):
    """box (N,4) i32 [x0, y0, x1, y1] inclusive grown by `margin` on every side and clamped to the image; an empty box stays
    [0, 0, -1, -1]"""
    some = (box[:, 2] >= box[:, 0]) & (box[:, 3] >= box[:, 1])
    lo = (box[:, :2] - margin).clamp_(min=0)
    hi = torch.stack([(box[:, 2] + margin).clamp_(max=W - 1), (box[:, 3] + margin).clamp_(max=H - 1)], dim=1)
    empty = torch.tensor([0, 0, -1, -1], dtype=torch.int32, device=box.device)
    return torch.where(some[:, None], torch.cat([lo, hi], dim=1), empty).to(torch.int32).contiguous()


def rms_of(stats, unit):
    """(N) f32 from stats (N,4) i32: sqrt(sum e e * 2^-30 / pairs) * unit in float64, rounded once; 0 without pairs"""
    pairs = stats[:, 0].to(torch.float64)
    see = ((stats[:, 3].to(torch.int64) << 32) | (stats[:, 2].to(torch.int64) & 0xFFFFFFFF)).to(torch.float64) * 2.0 ** -FRACTION_BITS
    rms = torch.sqrt(see / pairs.clamp(min=1.0)) * unit
    return torch.where(stats[:, 0] > 0, rms, torch.zeros_like(rms)).to(torch.float32)


@on_tensor_device
def _refine(vertices, faces, R, t, intr, H, W, near, depth, masks, scale, iters, gate, margin, damping, min_pairs, max_step):
    N = int(R.shape[0])
    box, _ = verify._windows(vertices, faces, verify.pose_views(R, t, scale), intr, H, W, near)
    box = grow_boxes(box, margin, H, W)
    offset, total = verify.window_offsets(box)
    # the one read-back, two numbers in one copy: the window total (it sizes the workspace) and the mesh radius (the unit of length)
    both = torch.stack([total.to(torch.float64), mesh_radius2(vertices).to(torch.float64)]).cpu()
    total, radius2 = int(both[0]), float(both[1])
    if not (radius2 > 0.0 and math.isfinite(radius2)):
        raise ValueError("refine_poses: the mesh has no extent (max |vertex|^2 = %r)" % radius2)
    iu = inv_unit(radius2, scale)
    unit = 1.0 / iu
    need = int(_lib.load().sam6d_pose_refine_workspace_bytes(total, N))
    ws = _empty((need // 8,), vertices, torch.int64)
    state = torch.cat([R.reshape(N, 9), t], dim=1).to(torch.float64).contiguous()
    acc = _empty((N, 32), vertices, torch.int64)
    stats = _empty((N, 4), vertices, torch.int32)
    history = _empty((N, iters, 2), vertices)
    for it in range(iters):
        _lib.call("sam6d_pose_refine_step", _p(vertices), int(vertices.shape[0]), _p(faces), int(faces.shape[0]), scale, N, *intr, H, W, near,
                  0, _p(box), offset.data_ptr(), total, _p(depth), masks.data_ptr() if masks is not None else None, gate, iu, damping,
                  min_pairs, max_step, state.data_ptr(), acc.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, _s())
        history[:, it, 0] = stats[:, 0].to(torch.float32)
        history[:, it, 1] = rms_of(stats, unit)
    return PoseRefinement(state[:, :9].to(torch.float32).reshape(N, 3, 3), state[:, 9:].to(torch.float32).contiguous(), stats[:, 0].clone(),
                          history[:, iters - 1, 1].clone(), stats[:, 1].clone(), history, box)


def refine_poses(mesh, R, t, K, depth, masks=None, iters=5, gate=0.02, margin=8, damping=1e-6, min_pairs=32, max_step=None, scale=1.0,
                 near=verify.NEAR):
    """`iters` projective point-to-plane Gauss-Newton steps for each of N poses against the observed depth.

    mesh, R, t, K, depth, masks, scale, near: as verify.render_compare takes them, with its errors.  iters >= 1.  gate: a
    rendered pixel pairs with its observed depth when the two differ by at most this, in the unit of t (2 cm under PEM's metre poses);
    with masks, only where masks[n] is set.  margin: pixels by which the window of the initial pose is grown on every side; the window
    stays fixed.  damping: A_ii += damping * A_ii before the solve.  min_pairs: a pose with fewer pairs is left as it is (status 1).
    max_step: a step with sqrt(|omega|^2 + |v / radius|^2) above this is refused (status 3); None: no bound.

    -> PoseRefinement.  A pose whose status is not 0 in an iteration keeps its state in that iteration, bit for bit; the float64 state
    stays on the device between the iterations and the only read-back is one 16-byte copy before the first (the window total and the
    mesh radius).  A CPU tensor raises RuntimeError; a wrong shape or dtype ValueError naming the argument."""
    name = "refine_poses"
    vertices, faces, R, t, depth, masks, intr, H, W = verify._pose_args(name, mesh, R, t, K, depth, masks, near)
    checks = (("iters", iters, lambda v: int(v) == v and v >= 1, "an integer >= 1"),
              ("gate", gate, lambda v: v >= 0.0 and math.isfinite(v), "a finite number >= 0"),
              ("margin", margin, lambda v: int(v) == v and 0 <= v <= verify.MAX_SIZE, "an integer in 0 .. %d" % verify.MAX_SIZE),
              ("damping", damping, lambda v: v >= 0.0 and math.isfinite(v), "a finite number >= 0"),
              ("min_pairs", min_pairs, lambda v: int(v) == v and v >= 1, "an integer >= 1"),
              ("max_step", math.inf if max_step is None else max_step, lambda v: v > 0.0, "a number > 0 or None"),
              ("scale", scale, lambda v: v != 0.0 and math.isfinite(v), "a finite number != 0"))
    for what, value, good, text in checks:
        if not good(float(value)):
            raise ValueError("%s: %s = %r is not %s" % (name, what, value, text))
    return _refine(vertices, faces, R, t, intr, H, W, float(near), depth, masks, float(np.float32(scale)), int(iters),
                   float(gate), int(margin), float(damping), int(min_pairs), math.inf if max_step is None else float(max_step))
