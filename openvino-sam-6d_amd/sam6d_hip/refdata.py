"""ISM's reference data from a template set, on the device: the block of ISM/run_inference_custom.py:129-163, 226-234 (and, for BOP
templates, ISM/provider/bop.py:60-83 with ISM/model/detector.py:65-196) that turns T template views -- rgb (T,H,W,3|4) u8 and
mask (T,H,W) u8, as sam6d_hip.onboard.render_templates leaves them or load_templates reads them -- into the `ref_data` that the drop-in
Instance_Segmentation_Model scores against: PIL's getbbox per mask (template_boxes), CropResizePad(224) of every template and mask in
one launch (template_crops), ONE pass of the DINOv2 encoder for both descriptor kinds (descriptors; the reference runs it twice on
the same crops), the scaled template poses (reference_poses) and the four-key dictionary (build).

Two flavours of the crop values, as the reference has them: "custom" (run_inference_custom.py:138-155: rgb / 255 times mask / 255, NO
Normalize -- what the reference feeds the encoder for custom templates, kept as it is) and "bop" (bop.py:66-83: rgb / 255, T.Normalize
after the padding, no mask product, the mask being the alpha band).

Imports runtime, _lib, dinov2 (and through it encoder, ism, ops), torch and numpy; PIL only inside load_templates.  The device
functions have no CPU route (a CPU tensor raises); eager_template_crops is the plain-torch partner on any device.
"""
import glob
import os

import numpy as np
import torch

from . import _lib, dinov2
from .runtime import _empty, _p, _s, on_tensor_device

FLAVOURS = {"custom": 0, "bop": 1}   # SAM6D_TEMPLATE_CUSTOM / SAM6D_TEMPLATE_BOP of include/sam6d_hip.h
MAX_T = 65535                        # templates per launch; larger sets are sliced
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
POSE_SCALE = 0.4                     # run_inference_custom.py:228


def _flavour(flavour):
    if flavour not in FLAVOURS:
        raise ValueError("sam6d_hip.refdata: unknown flavour %r (known: %s)" % (flavour, sorted(FLAVOURS)))
    return FLAVOURS[flavour]


def _check_band(band, name="band"):
    if not torch.is_tensor(band) or band.dtype != torch.uint8 or band.dim() != 3:
        raise ValueError("sam6d_hip.refdata: %s must be a (T, H, W) uint8 tensor, got %s %s"
                         % (name, tuple(band.shape) if torch.is_tensor(band) else type(band).__name__, getattr(band, "dtype", "")))
    if band.shape[1] < 1 or band.shape[2] < 1:
        raise ValueError("sam6d_hip.refdata: %s has an empty image: %s" % (name, tuple(band.shape)))


def _check_rgb(rgb, mask):
    if not torch.is_tensor(rgb) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] not in (3, 4):
        raise ValueError("sam6d_hip.refdata: rgb must be a (T, H, W, 3 or 4) uint8 tensor, got %s %s"
                         % (tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__, getattr(rgb, "dtype", "")))
    if tuple(rgb.shape[:3]) != tuple(mask.shape):
        raise ValueError("sam6d_hip.refdata: rgb %s and mask %s differ in (T, H, W)" % (tuple(rgb.shape), tuple(mask.shape)))


def _band_layout(band):
    """(band, pixel stride, image stride) in bytes of a (T,H,W) u8 tensor whose pixels (y, x) lie y W + x pixel strides into their
    image -- a contiguous tensor or one band of an interleaved one, read in place; any other view is copied once."""
    T, H, W = band.shape
    s0, s1, s2 = band.stride()
    ps = s2 if W > 1 else (s1 if H > 1 else 1)
    if not 1 <= ps <= 64 or (H > 1 and W > 1 and s1 != W * ps):
        band = band.contiguous()
        return band, 1, H * W
    return band, ps, (s0 if T > 1 else 0)


def _rgb_layout(rgb):
    """The same for the colours (T,H,W,3|4): channels one byte apart, pixels y W + x pixel strides into their image."""
    T, H, W, C = rgb.shape
    s0, s1, s2, s3 = rgb.stride()
    ps = s2 if W > 1 else (s1 if H > 1 else C)
    if s3 != 1 or not 3 <= ps <= 64 or (H > 1 and W > 1 and s1 != W * ps):
        rgb = rgb.contiguous()
        return rgb, C, H * W * C
    return rgb, ps, (s0 if T > 1 else 0)


@on_tensor_device
def _template_boxes(band):
    T, H, W = band.shape
    band, ps, ims = _band_layout(band)
    boxes = _empty((T, 4), band, torch.int64)
    for i0 in range(0, T, MAX_T):
        _lib.call("sam6d_template_boxes", band.data_ptr() + i0 * ims, min(MAX_T, T - i0), H, W, ps, ims, boxes.data_ptr() + 32 * i0, _s())
    return boxes


def template_boxes(band):
    """`mask.getbbox()` of every template (run_inference_custom.py:136; bop.py:66 with the alpha band) on the device: band (T,H,W)
    uint8 HIP tensor, or a view with uniform strides such as rgba[..., 3] (read in place) -> boxes (T,4) int64 on the device,
    (left, upper, right + 1, lower + 1) over the pixels != 0 and (0,0,0,0) for a band without one (PIL returns None there).
    No read-back."""
    _check_band(band)
    return _template_boxes(band)


def _empty_rows(boxes):
    """Indices of the boxes without area, from ONE read-back."""
    b = boxes.cpu()
    return torch.nonzero((b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1]))[:, 0].tolist()


@on_tensor_device
def _template_crops(rgb, mask, boxes, code):
    T, H, W = mask.shape
    rgb, rps, rims = _rgb_layout(rgb)
    mask, mps, mims = _band_layout(mask)
    out = _empty((T, 3, dinov2.IMG, dinov2.IMG), mask)
    om = _empty((T, dinov2.IMG, dinov2.IMG), mask)
    for i0 in range(0, T, MAX_T):
        _lib.call("sam6d_template_crops", rgb.data_ptr() + i0 * rims, rps, rims, mask.data_ptr() + i0 * mims, mps, mims,
                  boxes.data_ptr() + 32 * i0, min(MAX_T, T - i0), H, W, code, _p(out, i0 * 3 * dinov2.IMG * dinov2.IMG),
                  _p(om, i0 * dinov2.IMG * dinov2.IMG), _s())
    return out, om


def template_crops(rgb, mask, boxes=None, flavour="custom", check=True):
    """The template crops of run_inference_custom.py:138-155 ("custom") or bop.py:68-83 ("bop") in one launch: rgb (T,H,W,3|4) uint8
    (of four channels the first three are read, in place), mask (T,H,W) uint8 (the alpha band for "bop": rgba[..., 3] works in
    place), boxes (T,4) integer xyxy with exclusive ends on the device, None = template_boxes(mask) -> (templates (T,3,224,224),
    masks224 (T,224,224)) float32.  check=True reads the boxes back once and raises ValueError naming the templates whose box is
    empty (the reference fails there: getbbox() is None); check=False reads nothing back, and an empty box gives an all-padding crop."""
    code = _flavour(flavour)
    _check_band(mask, "mask")
    _check_rgb(rgb, mask)
    T = mask.shape[0]
    if boxes is not None and (not torch.is_tensor(boxes) or tuple(boxes.shape) != (T, 4) or boxes.dtype.is_floating_point
                              or boxes.dtype == torch.bool):
        raise ValueError("sam6d_hip.refdata: boxes must be (T, 4) integers, got %s %s"
                         % (tuple(boxes.shape) if torch.is_tensor(boxes) else type(boxes).__name__, getattr(boxes, "dtype", "")))
    if not mask.is_cuda or not rgb.is_cuda:
        raise RuntimeError("template_crops: needs HIP device tensors (eager_template_crops is the plain-torch route)")
    boxes = _template_boxes(mask) if boxes is None else boxes.to(device=mask.device, dtype=torch.long).contiguous()
    if check:
        bad = _empty_rows(boxes)
        if bad:
            raise ValueError("sam6d_hip.refdata: templates %s have an empty box (no pixel of their mask is set)" % bad)
    return _template_crops(rgb.to(mask.device), mask, boxes, code)


def host_boxes(band):
    """template_boxes' rule in numpy on the host: band (T,H,W) -> (T,4) int64."""
    a = np.asarray(band.cpu() if torch.is_tensor(band) else band) != 0
    out = np.zeros((a.shape[0], 4), np.int64)
    for t in range(a.shape[0]):
        ys, xs = np.nonzero(a[t].any(axis=1))[0], np.nonzero(a[t].any(axis=0))[0]
        if len(ys):
            out[t] = (xs[0], ys[0], xs[-1] + 1, ys[-1] + 1)
    return out


def eager_template_crops(rgb, mask, boxes=None, flavour="custom"):
    """template_crops in plain torch on the tensors' device (any device): the reference's own operations -- u8 / 255 in float64
    rounded by .float(), the mask product or Normalize's sub / div -- around dinov2.crop_resize_pad, with boxes on the host
    (None = host_boxes(mask)).  The route for a CPU model and the A/B partner of the kernel.  An empty box raises ValueError."""
    code = _flavour(flavour)
    _check_band(mask, "mask")
    _check_rgb(rgb, mask)
    b = torch.from_numpy(host_boxes(mask)) if boxes is None else torch.as_tensor(boxes).detach().to("cpu")
    bad = _empty_rows(b)
    if bad:
        raise ValueError("sam6d_hip.refdata: templates %s have an empty box (no pixel of their mask is set)" % bad)
    image = (rgb[..., :3].to(torch.float64) / 255).float().permute(0, 3, 1, 2)
    m = (mask.to(torch.float64) / 255).float()
    if code == FLAVOURS["custom"]:
        templates = dinov2.crop_resize_pad(image * m[:, None], b)
    else:
        mean = torch.tensor(MEAN, dtype=torch.float32, device=rgb.device)[:, None, None]
        std = torch.tensor(STD, dtype=torch.float32, device=rgb.device)[:, None, None]
        templates = dinov2.crop_resize_pad(image, b).sub_(mean).div_(std)
    return templates, dinov2.crop_resize_pad(m[:, None], b)[:, 0]


def _per_object(T, n_objects):
    n_objects = int(n_objects)
    if n_objects < 1 or T % n_objects:
        raise ValueError("sam6d_hip.refdata: %d templates do not divide into n_objects = %d" % (T, n_objects))
    return n_objects, T // n_objects


@on_tensor_device
def _descriptors(rgb, mask, weights, flavour, n_objects, check):
    n_obj, per = _per_object(mask.shape[0], n_objects)
    templates, m224 = template_crops(rgb, mask, None, flavour, check)
    cls, patch = dinov2.descriptors(templates, m224, weights)
    return dict(descriptors=cls.reshape(n_obj, per, dinov2.D), appe_descriptors=patch.reshape(n_obj, per, dinov2.NP, dinov2.D))


def descriptors(rgb, mask, weights, flavour="custom", n_objects=1, options=None, check=True):
    """compute_features + compute_masked_patch_feature of run_inference_custom.py:158-163 (detector.py:65-196 for BOP) on the crops
    of template_crops, in ONE pass of the encoder (dinov2.descriptors).  rgb, mask as template_crops takes them, the T templates
    object by object; weights a dinov2.DinoWeights -> dict(descriptors (n_objects, T / n_objects, 1024), appe_descriptors
    (n_objects, T / n_objects, 256, 1024))."""
    _flavour(flavour)
    _check_band(mask, "mask")
    _check_rgb(rgb, mask)
    _per_object(mask.shape[0], n_objects)
    return _descriptors(rgb, mask, weights, flavour, n_objects, check, options=options)


def reference_poses(obj_poses, index=None):
    """run_inference_custom.py:227-230: the template poses (T,4,4) with their translation times 0.4, in float64, then cast to float32,
    then (optionally) the rows `index` (load_index_level_in_level2's choice).  The caller loads obj_poses_level*.npy; the package
    ships no pose file.  The input is not modified.  -> numpy float32."""
    pose = np.array(obj_poses, dtype=np.float64, copy=True)
    if pose.ndim != 3 or pose.shape[1:] != (4, 4):
        raise ValueError("sam6d_hip.refdata: obj_poses must be (T, 4, 4), got %s" % (pose.shape,))
    pose[:, :3, 3] *= POSE_SCALE
    pose = pose.astype(np.float32)
    return pose if index is None else pose[np.asarray(index)]


def build(rgb, mask, weights, obj_poses, model_points, flavour="custom", n_objects=1, pose_index=None, options=None, check=True):
    """The `ref_data` of run_inference_custom.py:157-163, 226-234 -- what `model.ref_data = ...` of the drop-in
    Instance_Segmentation_Model takes: descriptors and appe_descriptors (descriptors()), poses (T', 4, 4) = reference_poses(obj_poses,
    pose_index) and pointcloud (n_objects, n, 3), all on the templates' device.  model_points: (n, 3) or (n_objects, n, 3) in metres,
    e.g. onboard.model_points(mesh, 2048) (mesh.sample(2048) / 1000 of the reference)."""
    ref = descriptors(rgb, mask, weights, flavour, n_objects, options=options, check=check)
    dev = mask.device
    ref["poses"] = torch.from_numpy(reference_poses(obj_poses, pose_index)).to(dev)
    pts = torch.as_tensor(model_points).to(device=dev, dtype=torch.float32)
    if pts.dim() == 2:
        pts = pts.unsqueeze(0)
    if pts.dim() != 3 or pts.shape[0] != ref["descriptors"].shape[0] or pts.shape[2] != 3:
        raise ValueError("sam6d_hip.refdata: model_points must be (n, 3) or (n_objects, n, 3), got %s" % (tuple(pts.shape),))
    ref["pointcloud"] = pts.contiguous()
    return ref


def load_templates(directory, device="cuda"):
    """rgb_i.png / mask_i.png, i = 0 .. T - 1, of a template directory (run_inference_custom.py:130-135; what
    onboard.save_templates and the render script write) -> (rgb (T,H,W,3) u8, mask (T,H,W) u8) on `device`."""
    from PIL import Image
    T = len(glob.glob(os.path.join(directory, "rgb_*.png")))
    if T == 0:
        raise ValueError("sam6d_hip.refdata: no rgb_*.png in %s" % directory)
    rgb = np.stack([np.array(Image.open(os.path.join(directory, "rgb_%d.png" % i)).convert("RGB")) for i in range(T)])
    mask = np.stack([np.array(Image.open(os.path.join(directory, "mask_%d.png" % i)).convert("L")) for i in range(T)])
    return torch.from_numpy(rgb).to(device), torch.from_numpy(mask).to(device)
