"""The six input tensors of Net.forward built from device-resident data: the reference's get_test_data and get_templates
(PEM/run_inference_custom_pytorch.py:226-367) without their per-detection host loops or cv2.

File I/O (PNG, JSON), RLE decoding (ism.rle_to_mask) and the detection-score threshold stay with the caller; the PLY reader and the
surface samples behind `model_points` are in sam6d_hip.onboard.  By default the random choices are drawn on the host with exactly the reference's np.random calls in the reference's order,
so a seeded numpy state gives the reference's points; everything else runs in the library's kernels (proposal_geometry /
proposal_choose / proposal_rgb, template_geometry / template_inputs: the tensor-level builders below, over csrc/testdata.hip, next.hip
and rgbprep.hip; `test_data` and `templates` at the end put them together).

Opt-in, `rng=DeviceChoice(seed)`: the choices are drawn on the device as well (draw_choice over csrc/choice.hip), without the host
loop, the permutation of all n candidates per detection and the upload of the indices.  That draw is NOT numpy's stream: it has an
integer definition of its own (counter-based sort keys, restated in tests/choice_ref.py), so it matches the reference in distribution
only and never reproduces the reference's points -- which is why it is not the default.
"""
import numpy as np
import torch

from . import _lib, ism
from .ops import _chk
from .runtime import _empty, _p, _s, on_tensor_device


# ------------------------------------------------------------------------------------------------- the builders, tensor by tensor
@on_tensor_device
def radius_normalize(pts, dense_po):
    """ViTEncoder.forward's radius normalisation (PEM/model/feature_extraction.py:133-137):
    -> dense_pm (B,M,3), dense_po (B,N,3) both divided by (radius + 1e-6), radius (B,)."""
    pts = pts.contiguous()
    dense_po = dense_po.contiguous()
    _chk(pts, "pts", torch.float32, 3)
    _chk(dense_po, "dense_po", torch.float32, 3)
    B, N, _ = dense_po.shape
    M = pts.shape[1]
    radius = _empty((B,), pts)
    po = _empty((B, N, 3), pts)
    pm = _empty((B, M, 3), pts)
    _lib.call("sam6d_radius_normalize", _p(dense_po), _p(pts), B, N, M, _p(radius), _p(po), _p(pm), _s())
    return pm, po, radius


@on_tensor_device
def depth_to_cloud(depth, K, bbox=None):
    """get_point_cloud_from_depth (PEM/utils/data_utils.py:92-110) on a device depth map (H,W) f32 -> (h,w,3)."""
    depth = depth.contiguous()
    _chk(depth, "depth", torch.float32, 2)
    H, W = depth.shape
    r0, r1, c0, c1 = (0, H, 0, W) if bbox is None else [int(v) for v in bbox]
    out = _empty((r1 - r0, c1 - c0, 3), depth)
    _lib.call("sam6d_depth_to_cloud", _p(depth), H, W, r0, r1, c0, c1, float(K[0][0]), float(K[1][1]), float(K[0][2]),
              float(K[1][2]), _p(out), _s())
    return out


@on_tensor_device
def proposal_geometry(masks, depth, K, radius, cap=None):
    """The per-proposal geometry of get_test_data before the random choice (PEM/run_inference_custom_pytorch.py:316-337):
    masks (N,H,W) uint8/bool, depth (H,W) f32 metres, K 3x3, radius = max CAD point norm.
    -> dict(bbox (N,4) i32, count (N), choose (N,cap) i32, cloud (N,cap,3), n_keep (N), center (N,3)); proposals with count <= 32
    or n_keep < 4 are the ones the reference skips (:320-324, :334-335) -- the caller filters on those two vectors."""
    masks = masks.to(torch.uint8).contiguous()
    depth = depth.contiguous()
    _chk(masks, "masks", torch.uint8, 3)
    _chk(depth, "depth", torch.float32, 2)
    N, H, Wd = masks.shape
    bbox = _empty((N, 4), depth, torch.int32)
    count = _empty((N,), depth, torch.int32)
    _lib.call("sam6d_mask_bbox", _p(masks), _p(depth), N, H, Wd, _p(bbox), _p(count), _s())
    cap = int(cap) if cap is not None else min(H, Wd) ** 2  # the crop is a square of side <= min(H, W)
    choose = _empty((N, cap), depth, torch.int32)
    cloud = _empty((N, cap, 3), depth)
    n_valid = _empty((N,), depth, torch.int32)
    _lib.call("sam6d_crop_masked_points", _p(masks), _p(depth), N, H, Wd, _p(bbox), float(K[0][0]), float(K[1][1]), float(K[0][2]),
              float(K[1][2]), cap, _p(choose), _p(cloud), _p(n_valid), _s())
    n_keep = _empty((N,), depth, torch.int32)
    center = _empty((N, 3), depth)
    _lib.call("sam6d_radius_filter", N, cap, _p(n_valid), float(radius), _p(choose), _p(cloud), _p(n_keep), _p(center), _s())
    return dict(bbox=bbox, count=count, choose=choose, cloud=cloud, n_valid=n_valid, n_keep=n_keep, center=center, cap=cap)


def proposal_choose(geom, sel, img_size=224):
    """pts (N,ns,3) and rgb_choose (N,ns) i64 for the caller's random choice sel (N,ns) into the kept points of each proposal
    (PEM/run_inference_custom_pytorch.py:339-355, get_resize_rgb_choose PEM/utils/data_utils.py:113-123)."""
    sel = sel.to(torch.int32).contiguous()
    N, ns = sel.shape
    pts = _empty((N, ns, 3), geom["cloud"])
    rc = _empty((N, ns), geom["cloud"], torch.int64)
    _lib.call("sam6d_choose_points", N, geom["cap"], _p(geom["choose"]), _p(geom["cloud"]), _p(geom["bbox"]), _p(sel), ns, int(img_size),
              _p(pts), _p(rc), _s())
    return pts, rc


MAX_CHOICE = 8192  # draw_choice sorts the chosen (key, index) pairs of a row in 64 KB of LDS


@on_tensor_device
def _draw_choice(n, ns, seed, row0):
    n = n.contiguous()
    _chk(n, "n", torch.int32, 1)
    N = n.shape[0]
    sel = _empty((N, ns), n, torch.int32)
    _lib.call("sam6d_draw_choice", _p(n), N, ns, int(seed) & 0xFFFFFFFF, int(row0) & 0xFFFFFFFF, _p(sel), _s())
    return sel


def draw_choice(n, ns, seed, row0=0):
    """The random choice of get_test_data / _get_template (PEM/run_inference_custom_pytorch.py:337-340, :215-218) on the device, for
    all rows in one launch: n (N) i32 HIP tensor of candidate counts (geom["n_keep"] / geom["n_valid"]) -> sel (N,ns) i32 for
    proposal_choose / template_inputs.  Row i is row row0 + i of the stream `seed` (both modulo 2^32).  n[i] > ns: ns distinct indices
    below n[i], a uniform subset in a uniform order; 1 <= n[i] <= ns: ns indices with replacement; n[i] <= 0: zeros; counts above 2^24
    are taken as 2^24.  A function of (seed, row, n[i], ns) alone, defined in csrc/choice.hip and restated in tests/choice_ref.py --
    not numpy's stream.  ns outside 1 .. 8192 raises ValueError (whatever device n is on); runs under on_tensor_device."""
    ns = int(ns)
    if not 1 <= ns <= MAX_CHOICE:
        raise ValueError("draw_choice: ns = %d is not in 1 .. %d" % (ns, MAX_CHOICE))
    return _draw_choice(n, ns, seed, row0)


class DeviceChoice:
    """`rng=` of test_data / templates that draws the choices on the device (draw_choice): the stream `seed`, and `row`, the next
    unused row of it -- 0 at first, advanced by the number of rows of each call, so successive frames or objects drawn with one object
    never reuse a row."""
    __slots__ = ("seed", "row")

    def __init__(self, seed):
        self.seed = int(seed)
        self.row = 0

    def draw(self, n, ns):
        sel = draw_choice(n, ns, self.seed, self.row)
        self.row += int(n.shape[0])
        return sel


def _rgb_crop_resize(images, stride, C, masks, depth, mask_mode, bbox, img_size, return_uint8, check):
    """sam6d_rgb_crop_resize over bbox.shape[0] items of images (..., H, W, C) u8 (stride: 1 = one image per item, 0 = shared)."""
    bbox = bbox.contiguous()
    _chk(bbox, "bbox", torch.int32, 2)
    N = bbox.shape[0]
    H, Wd = images.shape[-3:-1] if C == 3 else images.shape[-2:]
    S = int(img_size)
    out = _empty((N, 3, S, S), images)
    u8 = _empty((N, S, S, 3), images, torch.uint8) if return_uint8 else None
    status = _empty((N,), images, torch.int32) if check else None
    _lib.call("sam6d_rgb_crop_resize", images.data_ptr(), stride * H * Wd * C, C, H, Wd, masks.data_ptr() if masks is not None else None,
              depth.data_ptr() if depth is not None else None, mask_mode, N, _p(bbox), S, _p(out), u8.data_ptr() if u8 is not None else None,
              _p(status), _s())
    if check and N and bool(status.any()):
        bad = [i for i, v in enumerate(status.cpu().tolist()) if v]
        raise RuntimeError("rgb crop: the bbox of item(s) %s is not inside the %dx%d image" % (bad[:8], H, Wd))
    return (out, u8) if return_uint8 else out


def _image_channels(img, name, lead):
    """3 for (..., H, W, 3), 1 for a grayscale (..., H, W) u8 stack with `lead` leading dimensions"""
    _chk(img, name, torch.uint8)
    if img.dim() == lead + 3 and img.shape[-1] == 3:
        return 3
    if img.dim() == lead + 2:
        return 1
    raise RuntimeError("%s must be %s(H, W, 3) or %s(H, W) uint8, got %s" % (name, "(T, " * lead, "(T, " * lead, tuple(img.shape)))


@on_tensor_device
def proposal_rgb(image, masks, depth, geom, img_size=224, rgb_mask_flag=True, return_uint8=False, check=True):
    """The rgb input of get_test_data (PEM/run_inference_custom_pytorch.py:344-350) for every proposal in one launch: the crop
    geom["bbox"] (from proposal_geometry, or any (N,4) i32 (y1, y2, x1, x2)) of image (H,W,3) u8 RGB or (H,W) grayscale (:293-294),
    channels reversed, times (mask > 0) & (depth > 0) (:318) when rgb_mask_flag, cv2.resize INTER_LINEAR to img_size, ToTensor +
    Normalize.  -> rgb (N,3,S,S) f32, and with return_uint8 also the resized crops (N,S,S,3) u8.  check: one read-back of a status
    vector, RuntimeError for a bbox outside the image (boxes from proposal_geometry always lie inside; inputs.test_data skips it)."""
    image = image.contiguous()
    masks = masks.to(torch.uint8).contiguous()
    depth = depth.contiguous()
    C = _image_channels(image, "image", 0)
    _chk(masks, "masks", torch.uint8, 3)
    _chk(depth, "depth", torch.float32, 2)
    if tuple(depth.shape) != tuple(masks.shape[1:]) or tuple(image.shape[:2]) != tuple(depth.shape):
        raise RuntimeError("image %s, masks %s and depth %s disagree on (H, W)" % (tuple(image.shape), tuple(masks.shape), tuple(depth.shape)))
    if geom["bbox"].shape[0] != masks.shape[0]:
        raise RuntimeError("geom has %d boxes for %d masks" % (geom["bbox"].shape[0], masks.shape[0]))
    if rgb_mask_flag:
        return _rgb_crop_resize(image, 0, C, masks, depth, 1, geom["bbox"], img_size, return_uint8, check)
    return _rgb_crop_resize(image, 0, C, None, None, 0, geom["bbox"], img_size, return_uint8, check)


@on_tensor_device
def template_geometry(masks, xyz_mm, cap=None):
    """The crop of each template before the random choice (_get_template, PEM/run_inference_custom_pytorch.py:199-214): masks (T,H,W)
    u8 (mask == 255 is the object, :201), xyz_mm (T,H,W,3) f32 millimetres.  -> dict(bbox (T,4) i32 = get_bbox(mask == 255),
    count (T) mask pixels, choose (T,cap) i32 raster-order mask pixels of the crop, cloud (T,cap,3) = their xyz / 1000, n_valid (T),
    cap).  cap defaults to min(H, W)^2, the largest crop; n_valid[t] is the len(choose) the caller draws from (0: the reference's
    get_bbox would fail on that template)."""
    masks = masks.to(torch.uint8).contiguous()
    xyz_mm = xyz_mm.contiguous()
    _chk(masks, "masks", torch.uint8, 3)
    _chk(xyz_mm, "xyz_mm", torch.float32, 4)
    T, H, Wd = masks.shape
    if tuple(xyz_mm.shape) != (T, H, Wd, 3):
        raise RuntimeError("xyz_mm must be (%d, %d, %d, 3), got %s" % (T, H, Wd, tuple(xyz_mm.shape)))
    bbox = _empty((T, 4), masks, torch.int32)
    count = _empty((T,), masks, torch.int32)
    _lib.call("sam6d_template_bbox", _p(masks), T, H, Wd, _p(bbox), _p(count), _s())
    cap = int(cap) if cap is not None else min(H, Wd) ** 2
    choose = _empty((T, cap), masks, torch.int32)
    cloud = _empty((T, cap, 3), masks)
    n_valid = _empty((T,), masks, torch.int32)
    _lib.call("sam6d_template_crop_points", _p(masks), _p(xyz_mm), T, H, Wd, _p(bbox), cap, _p(choose), _p(cloud), _p(n_valid), _s())
    return dict(bbox=bbox, count=count, choose=choose, cloud=cloud, n_valid=n_valid, cap=cap)


@on_tensor_device
def template_inputs(images, masks, xyz_mm, sel, img_size=224, rgb_mask_flag=True, geom=None):
    """rgb, rgb_choose, xyz of _get_template (PEM/run_inference_custom_pytorch.py:199-222) for T templates at once: images (T,H,W,3)
    u8 RGB (or (T,H,W) grayscale), masks (T,H,W) u8 (mask == 255 is the object), xyz_mm (T,H,W,3) f32 millimetres, sel (T,ns) the
    caller's random choice into each template's n_valid crop pixels (:215-218).  -> rgb (T,3,S,S) f32, rgb_choose (T,ns) i64, xyz
    (T,ns,3) f32 metres.  geom: template_geometry(masks, xyz_mm) when the caller already has it (it draws sel from n_valid)."""
    images = images.contiguous()
    C = _image_channels(images, "images", 1)
    if geom is None:
        geom = template_geometry(masks, xyz_mm)
    masks = masks.to(torch.uint8).contiguous()
    T, H, Wd = masks.shape
    if tuple(images.shape[:3]) != (T, H, Wd):
        raise RuntimeError("images %s do not match masks %s" % (tuple(images.shape), tuple(masks.shape)))
    if not torch.is_tensor(sel) or sel.dim() != 2 or sel.shape[0] != T:
        raise RuntimeError("sel must be a (%d, ns) tensor" % T)
    xyz, rgb_choose = proposal_choose(geom, sel.to(masks.device), img_size)
    if rgb_mask_flag:
        rgb = _rgb_crop_resize(images, 1, C, masks, None, 2, geom["bbox"], img_size, False, False)
    else:
        rgb = _rgb_crop_resize(images, 1, C, None, None, 0, geom["bbox"], img_size, False, False)
    return rgb, rgb_choose, xyz


# ------------------------------------------------------------------------------------------------- get_test_data / get_templates
def _cfg(cfg, name, default=None):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def _draw(rng, n, ns):
    # PEM/run_inference_custom_pytorch.py:337-340 and :215-218
    if n <= ns:
        return rng.choice(np.arange(n), ns)
    return rng.choice(np.arange(n), ns, replace=False)


def test_data(image, depth_m, K, masks, scores, model_points, cfg, rng=np.random):
    """get_test_data (PEM/run_inference_custom_pytorch.py:256-367) from device tensors: image (H,W,3) u8 RGB or (H,W) grayscale,
    depth_m (H,W) f32 metres, K 3x3 (host), masks (N,H,W) u8 of the detections above the score threshold (ism.rle_to_mask), scores (N)
    host floats, model_points (M,3) f32 host array (the trimesh sample / 1000).  cfg: img_size, n_sample_observed_point, rgb_mask_flag.
    -> (input_data, kept): input_data = dict(pts, rgb, rgb_choose, score, model, K) as the reference builds it, kept = the indices of
    the detections it keeps (mask & depth > 32 pixels and >= 4 points inside radius * 1.2, :319-335).
    One host read-back, of (count, n_keep), decides the skips and the choice sizes.
    rng: np.random (the default) or any object with its `choice`: the reference's host draw, one call per kept detection in order.
    A DeviceChoice: the choices of all N detections are drawn on the device from geom["n_keep"], rows rng.row .. rng.row + N - 1
    (skipped detections have their row drawn and dropped), before the read-back, which then only decides `kept`."""
    dev = masks.device
    img_size = int(_cfg(cfg, "img_size", 224))
    ns = int(_cfg(cfg, "n_sample_observed_point", 2048))
    model_points = np.asarray(model_points.cpu() if torch.is_tensor(model_points) else model_points, dtype=np.float32)
    radius = np.max(np.linalg.norm(model_points, axis=1))  # :300
    K = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)
    geom = proposal_geometry(masks, depth_m, K, radius)
    device_draw = isinstance(rng, DeviceChoice)
    if device_draw:
        sel = rng.draw(geom["n_keep"], ns)
    cn = torch.stack([geom["count"], geom["n_keep"]]).cpu().numpy()
    kept = [i for i in range(masks.shape[0]) if cn[0, i] > 32 and cn[1, i] >= 4]
    if not device_draw:
        sel = np.zeros((masks.shape[0], ns), np.int32)  # rows of skipped detections stay 0 and are dropped below
        for i in kept:
            sel[i] = _draw(rng, int(cn[1, i]), ns)
        sel = torch.from_numpy(sel).to(dev)
    idx = torch.tensor(kept, dtype=torch.int64, device=dev)
    pts, rgb_choose = proposal_choose(geom, sel, img_size)
    box = dict(bbox=ism.take_rows(geom["bbox"], idx))
    rgb = proposal_rgb(image, ism.take_rows(masks.to(torch.uint8), idx), depth_m, box, img_size, bool(_cfg(cfg, "rgb_mask_flag", True)),
                           check=False)
    pts, rgb_choose = ism.take_rows(pts, idx), ism.take_rows(rgb_choose, idx)
    n = len(kept)
    scores = np.asarray(scores.cpu() if torch.is_tensor(scores) else scores)
    input_data = dict(
        pts=pts,
        rgb=rgb,
        rgb_choose=rgb_choose,
        score=torch.tensor([float(scores[i]) for i in kept], dtype=torch.float32).to(dev),
        model=torch.from_numpy(model_points).unsqueeze(0).repeat(n, 1, 1).to(dev),
        K=torch.from_numpy(K.astype(np.float32)).unsqueeze(0).repeat(n, 1, 1).to(dev),
    )
    return input_data, kept


def templates(images, masks, xyz_mm, cfg, rng=np.random):
    """get_templates (PEM/run_inference_custom_pytorch.py:226-253) from device tensors: images (T,H,W,3) u8 RGB renders, masks (T,H,W)
    u8 (255 = object), xyz_mm (T,H,W,3) f32 millimetres, in the order the reference loads the views.  cfg: img_size,
    n_sample_template_point, rgb_mask_flag.  -> all_tem, all_tem_pts, all_tem_choose: lists of (1,3,S,S), (1,ns,3), (1,ns) i64, the
    form ViTEncoder.get_obj_feats takes.  One host read-back, of the per-template pixel counts.
    rng: as in test_data; a DeviceChoice draws the T choices on the device from geom["n_valid"], rows rng.row .. rng.row + T - 1,
    behind the same read-back (it still refuses a template without mask pixels before anything is drawn)."""
    img_size = int(_cfg(cfg, "img_size", 224))
    ns = int(_cfg(cfg, "n_sample_template_point", 5000))
    geom = template_geometry(masks, xyz_mm)
    n_valid = geom["n_valid"].cpu().numpy()
    if (n_valid == 0).any():
        raise RuntimeError("templates: template(s) %s have no mask pixel (mask == 255)" % np.nonzero(n_valid == 0)[0].tolist())
    if isinstance(rng, DeviceChoice):
        sel = rng.draw(geom["n_valid"], ns)
    else:
        sel = torch.from_numpy(np.stack([_draw(rng, int(n), ns) for n in n_valid]).astype(np.int32)).to(masks.device)
    rgb, rgb_choose, xyz = template_inputs(images, masks, xyz_mm, sel, img_size, bool(_cfg(cfg, "rgb_mask_flag", True)), geom=geom)
    T = rgb.shape[0]
    return [rgb[t:t + 1] for t in range(T)], [xyz[t:t + 1] for t in range(T)], [rgb_choose[t:t + 1] for t in range(T)]
