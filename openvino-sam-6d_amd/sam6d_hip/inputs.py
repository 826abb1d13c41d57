"""The six input tensors of Net.forward built from device-resident data: the reference's get_test_data and get_templates
(PEM/run_inference_custom_pytorch.py:226-367) without their per-detection host loops or cv2.

File I/O (PNG, JSON, PLY), RLE decoding (ism.rle_to_mask), trimesh surface sampling and the detection-score threshold stay with the
caller.  The random choices are drawn on the host with exactly the reference's np.random calls in the reference's order, so a seeded
numpy state gives the reference's points; everything else runs in the library's kernels (pem.proposal_geometry / proposal_choose /
proposal_rgb, pem.template_geometry / template_inputs).
"""
import numpy as np
import torch

from . import pem


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
    One host read-back, of (count, n_keep), decides the skips and the choice sizes."""
    from . import ism
    dev = masks.device
    img_size = int(_cfg(cfg, "img_size", 224))
    ns = int(_cfg(cfg, "n_sample_observed_point", 2048))
    model_points = np.asarray(model_points.cpu() if torch.is_tensor(model_points) else model_points, dtype=np.float32)
    radius = np.max(np.linalg.norm(model_points, axis=1))  # :300
    K = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)
    geom = pem.proposal_geometry(masks, depth_m, K, radius)
    cn = torch.stack([geom["count"], geom["n_keep"]]).cpu().numpy()
    kept = [i for i in range(masks.shape[0]) if cn[0, i] > 32 and cn[1, i] >= 4]
    sel = np.zeros((masks.shape[0], ns), np.int32)  # rows of skipped detections stay 0 and are dropped below
    for i in kept:
        sel[i] = _draw(rng, int(cn[1, i]), ns)
    idx = torch.tensor(kept, dtype=torch.int64, device=dev)
    pts, rgb_choose = pem.proposal_choose(geom, torch.from_numpy(sel).to(dev), img_size)
    box = dict(bbox=ism.take_rows(geom["bbox"], idx))
    rgb = pem.proposal_rgb(image, ism.take_rows(masks.to(torch.uint8), idx), depth_m, box, img_size, bool(_cfg(cfg, "rgb_mask_flag", True)),
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
    form ViTEncoder.get_obj_feats takes.  One host read-back, of the per-template pixel counts."""
    img_size = int(_cfg(cfg, "img_size", 224))
    ns = int(_cfg(cfg, "n_sample_template_point", 5000))
    geom = pem.template_geometry(masks, xyz_mm)
    n_valid = geom["n_valid"].cpu().numpy()
    if (n_valid == 0).any():
        raise RuntimeError("templates: template(s) %s have no mask pixel (mask == 255)" % np.nonzero(n_valid == 0)[0].tolist())
    sel = np.stack([_draw(rng, int(n), ns) for n in n_valid]).astype(np.int32)
    rgb, rgb_choose, xyz = pem.template_inputs(images, masks, xyz_mm, torch.from_numpy(sel).to(masks.device), img_size,
                                               bool(_cfg(cfg, "rgb_mask_flag", True)), geom=geom)
    T = rgb.shape[0]
    return [rgb[t:t + 1] for t in range(T)], [xyz[t:t + 1] for t in range(T)], [rgb_choose[t:t + 1] for t in range(T)]
