"""The result pictures of the reference's two inference scripts, built on the device: vis_ism.png (ISM/run_inference_custom.py:48-84,
`visualize`) and vis_pem.png (PEM/run_inference_custom.py:110-134, `visualize`, over PEM/utils/draw_utils.py:5-97) -- without cv2,
scikit-image and distinctipy.  The masks, poses and model points are on the device when the picture is wanted; only the finished
canvas comes back, and only when a PIL image or a PNG is asked for.

What is the reference's and what is the package's own.  The pictures are defined by the integer recipes at the top of
csrc/overlay.hip and checked bit for bit against their numpy restatements (tests/overlay_ref.py).  The reference's: the grey
conversion (OpenCV's published 8-bit fixed point, restated, not pinned against cv2), the blend and its truncation, the choice of the
detection, the paint order and shades of the box, the truncating projection, the box corners and the side-by-side layout.  The
package's own, equal in kind only: the edge of a mask (not skimage's canny), the shapes of a thick line and of a disc (not cv2.line /
cv2.circle), the palette (distinctipy draws its colours at random, so there is nothing to match) and the rule that a point at or behind
the camera plane is skipped and counted (the reference divides by zero).

A third picture is the package's own altogether: vis_pem_render paints the instance map of verify.render_compare -- the CAD model's
rendered silhouette at every pose -- beside the input (the recipe at the top of csrc/verify.hip, restated in tests/verify_ref.py).

Imports runtime, _lib, torch and numpy; PIL only where an image is returned or saved.  There is no CPU route.
"""
import numpy as np
import torch

from . import _lib
from .runtime import _empty, _p, _s, on_tensor_device

MAX_SIZE = 8192       # H, W of both entries
MAX_MASKS = 4096
MAX_INSTANCES = 65535
MAX_POINTS = 65536
MAX_THICKNESS = 15
MAX_RADIUS = 15
GOLDEN = 0.6180339887498949  # (sqrt(5) - 1) / 2

_BOX_SIGNS = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]])


# ------------------------------------------------------------------------------------------------------------ host side
def palette(n):
    """n colours (n,3) u8 of the package's own: the golden-ratio hue walk through HSV at full saturation and value.  Colour k has
    hue h = frac(k * (sqrt(5) - 1) / 2); with i = floor(6 h) and f = 6 h - i its (r, g, b) is (1, f, 0), (1 - f, 1, 0), (0, 1, f),
    (0, 1 - f, 1), (f, 0, 1), (1, 0, 1 - f) for i = 0 .. 5, and a channel is int(255 * value) as ISM/run_inference_custom.py:67-69
    converts.  Float64 on the host.  NOT distinctipy's colours: those are drawn at random, so there is nothing to match."""
    k = np.arange(int(n), dtype=np.float64)
    h = np.mod(k * GOLDEN, 1.0) * 6.0
    i = np.floor(h).astype(np.int64) % 6
    f = h - np.floor(h)
    one, zero = np.ones_like(f), np.zeros_like(f)
    table = np.stack([np.stack([one, f, zero], 1), np.stack([1 - f, one, zero], 1), np.stack([zero, one, f], 1),
                      np.stack([zero, 1 - f, one], 1), np.stack([f, zero, one], 1), np.stack([one, zero, 1 - f], 1)])  # (6,n,3)
    rgb = table[i, np.arange(int(n))] if int(n) else np.zeros((0, 3))
    return (255.0 * rgb).astype(np.int64).astype(np.uint8)


def blend_table(color, alpha=0.33):
    """(3,256) u8: channel c of a mask pixel whose grey value is v, by the reference's own expression assigned into a uint8 array
    (ISM/run_inference_custom.py:70-72): alpha * color[c] + (1 - alpha) * v in float64, truncated."""
    v = np.arange(256, dtype=np.uint8)
    out = np.zeros((3, 256), dtype=np.uint8)
    for c in range(3):
        out[c, :] = alpha * int(color[c]) + (1 - alpha) * v
    return out


def box_corners(model_points):
    """The eight corners of the model's box (PEM/utils/draw_utils.py:20-49, :79-81): extent = max - min and centre = mean over the
    points, corner = centre + sign * (extent / 2) with the signs in the reference's order: +++, ++-, -++, -+-, +-+, +--, --+, ---.
    model_points (P,3) numpy -> (8,3) in the points' dtype, on the host."""
    pts = np.asarray(model_points)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("box_corners: model_points must be (P,3) with P >= 1, got %s" % (pts.shape,))
    half = (np.max(pts, axis=0) - np.min(pts, axis=0)) / 2
    return _BOX_SIGNS.astype(half.dtype) * half + np.mean(pts, axis=0)


def _image(rgb, name):
    """(H, W, row_stride in bytes) of an (H,W,3) u8 HIP tensor whose pixels are packed (a crop view of a larger image is accepted)."""
    if not torch.is_tensor(rgb):
        raise ValueError("%s: rgb must be a torch tensor on a HIP device, got %s" % (name, type(rgb).__name__))
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("%s: rgb must be (H,W,3) uint8, got %s %s" % (name, tuple(rgb.shape), rgb.dtype))
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError("%s: H x W = %d x %d is not in 1 .. %d" % (name, H, W, MAX_SIZE))
    if rgb.stride(2) != 1 or rgb.stride(1) != 3 or (H > 1 and rgb.stride(0) < 3 * W):
        raise ValueError("%s: rgb is not contiguous within its rows (strides %s; a crop view of a contiguous image is accepted)"
                         % (name, tuple(rgb.stride())))
    return H, W, int(rgb.stride(0)) if H > 1 else 3 * W


def _device_tensor(x, name, what, dtype, shape):
    if not torch.is_tensor(x):
        raise ValueError("%s: %s must be a torch tensor on a HIP device, got %s" % (name, what, type(x).__name__))
    if x.dtype != dtype:
        raise ValueError("%s: %s must be %s, got %s" % (name, what, dtype, x.dtype))
    if tuple(x.shape) != tuple(shape):
        raise ValueError("%s: %s must have shape %s, got %s" % (name, what, tuple(shape), tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("%s: %s is not contiguous" % (name, what))
    return x


def _on_device(name, **tensors):
    """the last check before a launch: every tensor on one HIP device"""
    first = None
    for what, x in tensors.items():
        if not x.is_cuda:
            raise ValueError("%s: %s is on the CPU (there is no CPU route)" % (name, what))
        first = x if first is None else first
        if x.device != first.device:
            raise ValueError("%s: %s is on %s and %s on %s" % (name, next(iter(tensors)), first.device, what, x.device))


def _colors(colors, n, name):
    """(n,3) u8 numpy from one colour or one per item"""
    c = np.asarray(colors)
    if c.shape == (3,):
        c = np.broadcast_to(c, (n, 3))
    if c.shape != (n, 3):
        raise ValueError("%s: colors must be one (3,) colour or (%d,3), got %s" % (name, n, c.shape))
    if c.size and (c.min() < 0 or c.max() > 255 or np.any(c != np.floor(c))):
        raise ValueError("%s: colors must be integers in 0 .. 255" % name)
    return np.ascontiguousarray(c.astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------ mask overlay
@on_tensor_device
def _overlay_masks(rgb, H, W, stride, masks, lut, edge):
    canvas = _empty((H, 2 * W, 3), rgb, torch.uint8)
    M = int(masks.shape[0])
    _lib.call("sam6d_overlay_masks", rgb.data_ptr(), stride, H, W, masks.data_ptr() if M else None, M, lut.data_ptr() if M else None,
              int(bool(edge)), canvas.data_ptr(), _s())
    return canvas


def overlay_masks(rgb, masks, colors=None, alpha=0.33, edge=True):
    """sam6d_overlay_masks: the picture of ISM/run_inference_custom.py:48-84 for M masks.  rgb (H,W,3) u8 and masks (M,H,W) u8 or bool
    HIP tensors; the masks are drawn in the order given, later over earlier (M = 1 is the reference, M = 0 the grey picture).
    colors: one (3,) colour, (M,3), or None = palette(M).  -> canvas (H, 2W, 3) u8 on the device: rgb on the left, the picture on
    the right (:79-84).  The recipe is at the top of csrc/overlay.hip.  Anything but packed HIP tensors of these dtypes raises
    ValueError before a launch."""
    H, W, stride = _image(rgb, "overlay_masks")
    if not torch.is_tensor(masks) or masks.dim() != 3:
        raise ValueError("overlay_masks: masks must be an (M,H,W) torch tensor")
    if masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError("overlay_masks: masks must be uint8 or bool, got %s" % masks.dtype)
    M = int(masks.shape[0])
    if M > MAX_MASKS:
        raise ValueError("overlay_masks: M = %d is not in 0 .. %d" % (M, MAX_MASKS))
    _device_tensor(masks, "overlay_masks", "masks", masks.dtype, (M, H, W))
    cols = _colors(palette(M) if colors is None else colors, M, "overlay_masks")
    _on_device("overlay_masks", rgb=rgb, masks=masks)
    lut = np.stack([blend_table(c, alpha) for c in cols]) if M else np.zeros((0, 3, 256), np.uint8)
    return _overlay_masks(rgb, H, W, stride, masks, torch.from_numpy(lut).to(rgb.device), edge)


def _to_device_image(rgb, device=None):
    """A PIL image, numpy array or tensor (H,W,3) u8 as a contiguous HIP tensor"""
    if torch.is_tensor(rgb):
        if rgb.is_cuda:
            return rgb
        dev = device or torch.device("cuda")
        return rgb.contiguous().to(dev)
    arr = np.asarray(rgb)
    if not (arr.flags.c_contiguous and arr.flags.writeable):  # (a PIL image gives a read-only view)
        arr = np.array(arr, order="C")
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("rgb must be (H,W,3) uint8, got %s %s" % (arr.shape, arr.dtype))
    return torch.from_numpy(arr).to(device or torch.device("cuda"))


def _finish(canvas, save_path):
    """The canvas as a PIL image, written as PNG when asked (PIL only)."""
    from PIL import Image
    img = Image.fromarray(canvas.cpu().numpy(), "RGB")
    if save_path is not None:
        img.save(save_path)
    return img


def best_detection(scores):
    """The index ISM/run_inference_custom.py:55-59 picks: the first detection with the strictly highest score above 0.  None raises
    ValueError (the reference dies with a NameError there)."""
    best, best_score = None, 0.0
    for i, s in enumerate(scores):
        if best_score < float(s):
            best, best_score = i, float(s)
    if best is None:
        raise ValueError("vis_ism: no detection has a score above 0 (%d detections)" % len(scores))
    return best


def vis_ism(rgb, detections, save_path=None):
    """`visualize` of ISM/run_inference_custom.py:48-84: the best detection's mask over the grey image beside the input.  rgb: a PIL
    image, an (H,W,3) u8 array or a HIP tensor; detections: a `Detections` object (masks on the device, scores, object_ids) or the
    list of dicts of detection_ism.json (score, category_id, segmentation = RLE, decoded with ism.rle_to_mask).  The colour is
    palette(len(detections))[category_id - 1].  -> the (2W, H) PIL image, also written to save_path as PNG when given."""
    is_list = isinstance(detections, (list, tuple))
    if is_list:
        n = len(detections)
        best = best_detection([d["score"] for d in detections])
        category = int(detections[best]["category_id"])
    else:
        n = len(detections.scores)
        best = best_detection(torch.as_tensor(detections.scores).cpu().tolist())
        category = int(torch.as_tensor(detections.object_ids)[best]) + 1  # save_to_file's category_id (ISM/model/utils.py:160)
    if not 1 <= category <= n:
        raise ValueError("vis_ism: category_id = %d has no colour in a palette of %d detections" % (category, n))
    masks = None if is_list else torch.as_tensor(detections.masks)
    img = _to_device_image(rgb, masks.device if masks is not None and masks.is_cuda else None)
    if is_list:
        from . import ism
        mask = ism.rle_to_mask([detections[best]["segmentation"]], img.device)
    else:
        mask = masks[best:best + 1].to(img.device)
        mask = (mask if mask.dtype in (torch.uint8, torch.bool) else (mask > 0)).contiguous()
    canvas = overlay_masks(img, mask, colors=palette(n)[category - 1])
    return _finish(canvas, save_path)


# ------------------------------------------------------------------------------------------------------------ pose overlay
@on_tensor_device
def _draw_detections(rgb, H, W, stride, R, t, K, box, pts, colors, thickness, radius):
    N, P = int(R.shape[0]), int(pts.shape[0])
    need = int(_lib.load().sam6d_draw_detections_workspace_bytes(H, W))
    ws = _empty((need // 4,), rgb, torch.int32)
    canvas = _empty((H, 2 * W, 3), rgb, torch.uint8)
    n_skipped = _empty((N,), rgb, torch.int32)
    _lib.call("sam6d_draw_detections", rgb.data_ptr(), stride, H, W, _p(R) if N else None, _p(t) if N else None, _p(K) if N else None, N,
              _p(box), _p(pts) if P else None, P, colors.data_ptr() if N else None, thickness, radius, canvas.data_ptr(),
              _p(n_skipped) if N else None, ws.data_ptr(), need, _s())
    return canvas, n_skipped


def draw_primitives(rgb, R, t, K, box, pts, colors=(255, 0, 0), thickness=3, radius=1):
    """sam6d_draw_detections on given primitives: rgb (H,W,3) u8, R (N,3,3), t (N,3), K (N,3,3), box (8,3) and pts (P,3) f32 -- packed
    HIP tensors on one device; colors one (3,) colour or (N,3).  -> (canvas (H, 2W, 3) u8, n_skipped (N) i32) on the device.  The
    recipe is at the top of csrc/overlay.hip.  A CPU tensor, a non-contiguous one, a wrong dtype or shape, or a size outside the
    limits raises ValueError before a launch."""
    name = "draw_detections"
    H, W, stride = _image(rgb, name)
    if not torch.is_tensor(R) or R.dim() != 3:
        raise ValueError("%s: R must be an (N,3,3) torch tensor" % name)
    N = int(R.shape[0])
    if N > MAX_INSTANCES:
        raise ValueError("%s: N = %d is not in 0 .. %d" % (name, N, MAX_INSTANCES))
    _device_tensor(R, name, "R", torch.float32, (N, 3, 3))
    _device_tensor(t, name, "t", torch.float32, (N, 3))
    _device_tensor(K, name, "K", torch.float32, (N, 3, 3))
    _device_tensor(box, name, "box", torch.float32, (8, 3))
    if not torch.is_tensor(pts) or pts.dim() != 2:
        raise ValueError("%s: pts must be a (P,3) torch tensor" % name)
    P = int(pts.shape[0])
    if P > MAX_POINTS:
        raise ValueError("%s: P = %d is not in 0 .. %d" % (name, P, MAX_POINTS))
    _device_tensor(pts, name, "pts", torch.float32, (P, 3))
    thickness, radius = int(thickness), int(radius)
    if not 1 <= thickness <= MAX_THICKNESS:
        raise ValueError("%s: thickness = %d is not in 1 .. %d" % (name, thickness, MAX_THICKNESS))
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError("%s: radius = %d is not in 0 .. %d" % (name, radius, MAX_RADIUS))
    cols = _colors(colors, N, name)
    _on_device(name, rgb=rgb, R=R, t=t, K=K, box=box, pts=pts)
    cols = torch.from_numpy(cols).to(rgb.device)
    return _draw_detections(rgb, H, W, stride, R, t, K, box, pts, cols, thickness, radius)


def choose_points(model_points, n_points=512, rng=None, device=None):
    """The points draw_detections paints (PEM/utils/draw_utils.py:84-85): model_points[choice] as a (n_points,3) f32 HIP tensor.
    rng None: the reference's own call np.random.choice(np.arange(len(pts)), n_points) on numpy's global state, so a seeded state
    gives the reference's points; a numpy RandomState or Generator: its .choice; an inputs.DeviceChoice: drawn on the device (its own
    stream, equal in distribution only)."""
    from .inputs import DeviceChoice
    n_all = int(model_points.shape[0])
    if isinstance(rng, DeviceChoice):
        pts = torch.as_tensor(model_points).to(device=device, dtype=torch.float32)
        sel = rng.draw(torch.tensor([n_all], dtype=torch.int32, device=pts.device), int(n_points))
        return pts.index_select(0, sel[0].to(torch.int64)).contiguous()
    choose = (np.random if rng is None else rng).choice(np.arange(n_all), int(n_points))
    if torch.is_tensor(model_points):
        pts = model_points.to(device=device, dtype=torch.float32)
        return pts.index_select(0, torch.from_numpy(np.asarray(choose, dtype=np.int64)).to(pts.device)).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(model_points)[choose], dtype=np.float32)).to(device)


def draw_detections(rgb, R, t, model_points, K, colors=(255, 0, 0), n_points=512, rng=None, thickness=3, radius=1):
    """`draw_detections` of PEM/utils/draw_utils.py:75-97 on the device: the box of the model and n_points of its points at every
    pose, painted over rgb.  rgb (H,W,3) u8, R (N,3,3), t (N,3), K (N,3,3) f32 HIP tensors; model_points (P,3), numpy or a tensor, in
    the units of t.  The points are chosen as choose_points describes (rng).  colors: one colour or one per instance.
    -> (canvas (H, 2W, 3) u8: rgb on the left, the picture on the right; n_skipped (N) i32: primitives not drawn, see
    csrc/overlay.hip) on the device."""
    H, W, _ = _image(rgb, "draw_detections")
    if not torch.is_tensor(model_points):
        model_points = np.asarray(model_points)
    if len(model_points.shape) != 2 or model_points.shape[1] != 3 or model_points.shape[0] < 1:
        raise ValueError("draw_detections: model_points must be (P,3) with P >= 1, got %s" % (tuple(model_points.shape),))
    _on_device("draw_detections", rgb=rgb)
    host = model_points.detach().cpu().numpy() if torch.is_tensor(model_points) else model_points
    box = torch.from_numpy(np.ascontiguousarray(box_corners(host), dtype=np.float32)).to(rgb.device)
    n_points = int(n_points)
    pts = choose_points(model_points, n_points, rng, rgb.device) if n_points > 0 else torch.zeros((0, 3), device=rgb.device)
    return draw_primitives(rgb, R, t, K, box, pts, colors, thickness, radius)


def vis_pem(rgb, R, t, model_points, K, save_path=None):
    """`visualize` of PEM/run_inference_custom.py:110-134: draw_detections in (255, 0, 0) beside the input.  rgb a PIL image, array
    or HIP tensor; R (N,3,3), t (N,3), K (N,3,3) arrays or tensors (uploaded as f32 when they are not on the device); model_points
    (P,3).  -> the (2W, H) PIL image, also written to save_path as PNG when given."""
    dev = next((x.device for x in (rgb, R, t, K) if torch.is_tensor(x) and x.is_cuda), None)
    img = _to_device_image(rgb, dev)

    def put(x, shape):
        return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=img.device, dtype=torch.float32).reshape(shape).contiguous()

    R, K = put(R, (-1, 3, 3)), put(K, (-1, 3, 3))
    if K.shape[0] == 1 and R.shape[0] != 1:  # one camera for all instances
        K = K.expand(R.shape[0], 3, 3).contiguous()
    canvas, _ = draw_detections(img, R, put(t, (-1, 3)), model_points, K, colors=(255, 0, 0))
    return _finish(canvas, save_path)


# ------------------------------------------------------------------------------------------------------------ rendered silhouettes
MAX_RENDER_SIZE = 2048    # H, W of sam6d_overlay_instances
MAX_RENDER_INSTANCES = 1024


@on_tensor_device
def _overlay_instances(rgb, H, W, stride, ids, colors, alpha):
    canvas = _empty((H, 2 * W, 3), rgb, torch.uint8)
    _lib.call("sam6d_overlay_instances", rgb.data_ptr(), stride, H, W, _p(ids), colors.data_ptr(), int(colors.shape[0]), alpha,
              canvas.data_ptr(), _s())
    return canvas


def overlay_instances(rgb, ids, colors, alpha=128):
    """sam6d_overlay_instances: rgb (H,W,3) u8 and ids (H,W) i32 HIP tensors (verify.render_compare's instance map; an id outside
    [0, N) is background), colors (N,3), alpha an integer in 0 .. 256 -> canvas (H, 2W, 3) u8 on the device: rgb on the left; on the
    right every instance blended in its colour, its silhouette and the line to another instance in the colour unblended.  The recipe
    is at the top of csrc/verify.hip."""
    name = "overlay_instances"
    H, W, stride = _image(rgb, name)
    if not (H <= MAX_RENDER_SIZE and W <= MAX_RENDER_SIZE):
        raise ValueError("%s: H x W = %d x %d is not in 1 .. %d" % (name, H, W, MAX_RENDER_SIZE))
    _device_tensor(ids, name, "ids", torch.int32, (H, W))
    c = np.asarray(colors)
    if c.ndim != 2 or not 1 <= c.shape[0] <= MAX_RENDER_INSTANCES:
        raise ValueError("%s: colors must be (N,3) with N in 1 .. %d, got %s" % (name, MAX_RENDER_INSTANCES, c.shape))
    cols = _colors(c, c.shape[0], name)
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError("%s: alpha = %r is not an integer in 0 .. 256" % (name, alpha))
    _on_device(name, rgb=rgb, ids=ids)
    return _overlay_instances(rgb, H, W, stride, ids, torch.from_numpy(cols).to(rgb.device), int(alpha))


def vis_pem_render(rgb, ids, colors=None, alpha=0.5, save_path=None):
    """The picture vis_pem leaves out: the CAD model's rendered silhouette at every pose, beside the input.  rgb a PIL image, array or
    HIP tensor; ids (H,W) i32 HIP tensor, the instance map of verify.render_compare (-1 = background); colors (N,3) or None =
    palette(n) with n = the largest id + 1 (one read-back); alpha: the weight of the colour, rounded to 1 / 256.  -> the (2W, H) PIL
    image, also written to save_path as PNG when given.  The package's own picture: the reference draws a box and points
    (PEM/utils/draw_utils.py:75-97)."""
    if not torch.is_tensor(ids):
        raise ValueError("vis_pem_render: ids must be an (H,W) int32 torch tensor on a HIP device, got %s" % type(ids).__name__)
    img = _to_device_image(rgb, ids.device if ids.is_cuda else None)
    if colors is None:
        colors = palette(max(int(ids.max()) + 1, 1) if ids.numel() else 1)
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("vis_pem_render: alpha = %r is not in 0 .. 1" % (alpha,))
    canvas = overlay_instances(img, ids, colors, alpha=int(np.floor(float(alpha) * 256.0 + 0.5)))
    return _finish(canvas, save_path)
