"""Test-only numpy restatement of the reference's rgb preprocessing (PEM/run_inference_custom_pytorch.py:151-153, :207-212, :344-350):
cv2.resize(..., INTER_LINEAR) for CV_8UC3 as OpenCV 4.x computes it (imgproc/src/resize.cpp, 11-bit fixed point, the vectorised
vertical pass; a 2x crop takes the INTER_AREA fast path, an S x S crop is copied), ToTensor + Normalize, and _get_template /
get_test_data composed from it.  OpenCV itself is not needed: parity with it is checked only where cv2 imports
(tests/test_rgb_inputs.py).  Nothing in the package imports this module."""
import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _sat16(v):
    return np.clip(v, -32768, 32767)


def _coef(f):
    # saturate_cast<short>(float * 2048): cvRound = round half to even
    return _sat16(np.rint(f * np.float32(2048.0))).astype(np.int64)


def taps(src_len, S, clamp):
    """(s, w0, w1) per output index along one axis: fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), fx -= s; with clamp (x axis)
    s < 0 -> (0, 0) and s >= len - 1 -> (len - 1, 0)."""
    scale = 1.0 / (float(S) / float(src_len))
    f = ((np.arange(S, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= src_len - 1
        f[hi], s[hi] = 0, src_len - 1
    return s, _coef(np.float32(1.0) - f), _coef(f)


def resize_linear(src, S):
    """cv2.resize(src, (S, S), interpolation=cv2.INTER_LINEAR) of an (h, w, 3) uint8 image."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    h, w = src.shape[:2]
    if h == S and w == S:
        return src.copy()
    s = src.astype(np.int64)
    if h == 2 * S and w == 2 * S:  # INTER_AREA fast path
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = taps(w, S, True)
    nxt = np.where(a1 != 0, np.minimum(sx + 1, w - 1), sx)
    hx = s[:, sx] * a0[None, :, None] + np.where((a1 != 0)[None, :, None], s[:, nxt] * a1[None, :, None], 0)  # (h, S, 3)
    sy, b0, b1 = taps(h, S, False)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    t0 = (_sat16(hx[y0] >> 4) * b0[:, None, None]) >> 16
    t1 = (_sat16(hx[y1] >> 4) * b1[:, None, None]) >> 16
    return np.clip((_sat16(t0 + t1) + 2) >> 2, 0, 255).astype(np.uint8)


def bilinear_f64(src, S):
    """The same coordinate map in float64 with exact weights and no rounding (the yardstick for the fixed-point restatement)."""
    src = np.asarray(src, dtype=np.float64)
    h, w = src.shape[:2]

    def axis(n, clamp):
        f = (np.arange(S) + 0.5) * (n / S) - 0.5
        s = np.floor(f).astype(np.int64)
        f = f - s
        if clamp:
            f[s < 0], s[s < 0] = 0, 0
            f[s >= n - 1], s[s >= n - 1] = 0, n - 1
        return s, f

    sx, fx = axis(w, True)
    sy, fy = axis(h, False)
    x1 = np.minimum(sx + 1, w - 1)
    hx = src[:, sx] * (1 - fx)[None, :, None] + src[:, x1] * fx[None, :, None]
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    return hx[y0] * (1 - fy)[:, None, None] + hx[y1] * fy[:, None, None]


def to_tensor_normalize(u8):
    """transforms.ToTensor() + Normalize(MEAN, STD) on torch CPU, fp32: (H, W, 3) uint8 -> (3, H, W)."""
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]).div_(torch.as_tensor(STD, dtype=torch.float32)[:, None, None])


def crop_rgb(img, bbox, mask_crop, S, rgb_mask_flag=True):
    """img[y1:y2, x1:x2][:, :, ::-1] times the mask bit, resized: the uint8 crop (S, S, 3)."""
    y1, y2, x1, x2 = [int(v) for v in bbox]
    if img.ndim == 2:
        img = np.concatenate([img[:, :, None]] * 3, axis=2)
    rgb = img[y1:y2, x1:x2, :][:, :, ::-1]
    if rgb_mask_flag:
        rgb = rgb * (mask_crop[:, :, None] > 0).astype(np.uint8)
    return resize_linear(rgb, S)


def resize_rgb_choose(choose, bbox, S):
    # get_resize_rgb_choose (PEM/utils/data_utils.py:113-123)
    rmin, rmax, cmin, cmax = bbox
    ch, cw = rmax - rmin, cmax - cmin
    return (np.floor((choose // cw) * (S / ch)) * S + np.floor((choose % cw) * (S / cw))).astype(np.int64)


def _draw(n, ns):
    if n <= ns:
        return np.random.choice(np.arange(n), ns)
    return np.random.choice(np.arange(n), ns, replace=False)


def get_template(rgb, mask_png, xyz_mm, S=224, ns=5000, rgb_mask_flag=True):
    """_get_template (PEM/run_inference_custom_pytorch.py:199-222) on loaded arrays; draws from np.random's global state."""
    from oracle.pem_oracle import get_bbox
    xyz = xyz_mm.astype(np.float32) / 1000.0
    mask = mask_png.astype(np.uint8) == 255
    bbox = get_bbox(mask)
    y1, y2, x1, x2 = bbox
    mask = mask[y1:y2, x1:x2]
    u8 = crop_rgb(rgb, bbox, mask, S, rgb_mask_flag)
    choose = (mask > 0).astype(np.float32).flatten().nonzero()[0]
    choose = choose[_draw(len(choose), ns)]
    xyz = xyz[y1:y2, x1:x2, :].reshape((-1, 3))[choose, :]
    return u8, to_tensor_normalize(u8), resize_rgb_choose(choose, [y1, y2, x1, x2], S), xyz


def get_test_data(img, depth, K, masks, scores, model_points, S=224, ns=2048, rgb_mask_flag=True):
    """get_test_data (PEM/run_inference_custom_pytorch.py:256-367) after file loading: -> (dict of host tensors, kept, uint8 crops)."""
    from oracle.pem_oracle import proposal_geometry
    radius = np.max(np.linalg.norm(model_points, axis=1))
    out = dict(pts=[], rgb=[], rgb_choose=[], score=[])
    kept, crops = [], []
    for i in range(masks.shape[0]):
        o = proposal_geometry(masks[i], depth, K, radius)
        if o is None:
            continue
        choose, cloud = o["choose"], o["cloud"]
        idx = _draw(len(choose), ns)
        choose, cloud = choose[idx], cloud[idx]
        y1, y2, x1, x2 = o["bbox"]
        m = np.logical_and(masks[i] > 0, depth > 0)[y1:y2, x1:x2]
        u8 = crop_rgb(img, o["bbox"], m, S, rgb_mask_flag)
        crops.append(u8)
        out["pts"].append(torch.FloatTensor(cloud))
        out["rgb"].append(to_tensor_normalize(u8))
        out["rgb_choose"].append(torch.from_numpy(resize_rgb_choose(choose, o["bbox"], S)))
        out["score"].append(scores[i])
        kept.append(i)
    n = len(kept)
    data = dict(pts=torch.stack(out["pts"]), rgb=torch.stack(out["rgb"]), rgb_choose=torch.stack(out["rgb_choose"]),
                score=torch.FloatTensor(out["score"]), model=torch.FloatTensor(model_points).unsqueeze(0).repeat(n, 1, 1),
                K=torch.FloatTensor(K).unsqueeze(0).repeat(n, 1, 1))
    return data, kept, crops
