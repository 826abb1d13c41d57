"""Drop-in for PEM/utils/draw_utils.py without cv2: the numpy helpers in numpy, the drawing on the device (sam6d_hip.visualize,
csrc/overlay.hip).  draw_3d_bbox and draw_3d_pts on single primitives are not provided: the library paints all instances in one call.
The line and disc shapes are the package's own, not cv2's (equal in kind only)."""
import numpy as np
import torch

from sam6d_hip import visualize as _vis


def calculate_2d_projections(coordinates_3d, intrinsics):
    """coordinates (3,N), intrinsics (3,3) -> (N,2) int32, truncated toward zero (PEM/utils/draw_utils.py:5-18)."""
    q = np.asarray(intrinsics) @ np.asarray(coordinates_3d)
    return (q[:2] / q[2]).T.astype(np.int32)


def get_3d_bbox(scale, shift=0):
    """The eight corners (3,8) of a box of size `scale` (3 values or one) centred at `shift` (PEM/utils/draw_utils.py:20-49)."""
    half = np.asarray(scale) / 2 * np.ones(3)
    return (_vis._BOX_SIGNS * half + shift).T


def draw_detections(image, pred_rots, pred_trans, model_points, intrinsics, color=(255, 0, 0)):
    """PEM/utils/draw_utils.py:75-97: numpy in, the numpy picture (H,W,3) u8 out (the right half of the library's canvas).  Uploads,
    calls sam6d_hip.visualize.draw_detections and downloads; raises RuntimeError on a machine without a HIP device."""
    if not torch.cuda.is_available():
        raise RuntimeError("draw_detections: needs a HIP device (this build has no CPU path)")
    dev = torch.device("cuda")
    img = _vis._to_device_image(np.asarray(image), dev)

    def put(x, shape):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(shape))).to(dev)

    canvas, _ = _vis.draw_detections(img, put(pred_rots, (-1, 3, 3)), put(pred_trans, (-1, 3)), np.asarray(model_points),
                                     put(intrinsics, (-1, 3, 3)), colors=color)
    W = img.shape[1]
    return canvas[:, W:].cpu().numpy()
