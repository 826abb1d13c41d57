"""Drop-in for ISM/utils/bbox_utils.py: compute_iou (:197-222) on the library, and CropResizePad (:89-126) as a thin wrapper of the
package's own plain-torch gather (sam6d_hip.dinov2.crop_resize_pad, the eager partner of sam6d_dino_crop_proposals; the GPU path of
model/dinov2.py does not come through here)."""
from sam6d_hip import dinov2 as _dinov2
from sam6d_hip import ism as _ism


def compute_iou(bb_a, bb_b):
    return _ism.compute_iou(bb_a, bb_b)


class CropResizePad:
    """CropResizePad(size)(images (N, C, H, W), boxes (N, 4) integer xyxy) -> (N, C, size, size); square targets only."""

    def __init__(self, target_size):
        side = target_size if isinstance(target_size, int) else tuple(target_size)
        if not isinstance(side, int):
            if len(side) != 2 or side[0] != side[1]:
                raise NotImplementedError("CropResizePad: only square targets are implemented, got %s" % (side,))
            side = int(side[0])
        self.target_size = (side, side)

    def __call__(self, images, boxes):
        return _dinov2.crop_resize_pad(images, boxes, self.target_size[0])
