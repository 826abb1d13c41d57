"""The rgb input of Net.forward on the device (inputs.proposal_rgb / template_inputs) and the assembled inputs (sam6d_hip.inputs) against
the numpy restatement of the reference's preprocessing (tests/cv2_linear.py): resized crops byte for byte, normalised tensors and
every other input bitwise, and the (R, t, score) the network computes from either."""
import importlib

import numpy as np
import pytest
import torch

from tests import cv2_linear as CV
from sam6d_hip import inputs, synth

pytestmark = pytest.mark.gpu

H, W = 480, 640
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def _scene(seed, N):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (0.6 + 0.0004 * xx + 0.05 * g.random((H, W))).astype(np.float32)
    depth[g.random((H, W)) < 0.05] = 0  # zero-depth pixels inside the masks
    masks = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        cy, cx, r = g.integers(0, H), g.integers(0, W), g.integers(2, 160)
        m = ((xx - cx) ** 2 + (yy - cy) ** 2) < r * r
        m &= g.random((H, W)) > 0.15  # holes
        masks[i] = m * g.integers(1, 256)
    return img, depth, masks


def _want_u8(img, depth, masks, bbox, S, flag):
    out = []
    for i, b in enumerate(bbox):
        y1, y2, x1, x2 = b
        if y2 == y1 or x2 == x1:  # an empty crop (a skipped proposal): every pixel masked out
            out.append(np.zeros((S, S, 3), np.uint8))
            continue
        m = np.logical_and(masks[i] > 0, depth > 0)[y1:y2, x1:x2]
        out.append(CV.crop_rgb(img, b, m, S, flag))
    return np.stack(out)


def _check(dev, img, depth, masks, bbox, S=224, flag=True):
    geom = dict(bbox=torch.tensor(bbox, dtype=torch.int32, device=dev))
    rgb, u8 = inputs.proposal_rgb(torch.from_numpy(img).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(depth).to(dev), geom,
                                  S, flag, return_uint8=True)
    got = u8.cpu().numpy()
    want = _want_u8(img, depth, masks, bbox, S, flag)
    for i in range(len(bbox)):
        assert np.array_equal(got[i], want[i]), ("crop", i, bbox[i], int((got[i] != want[i]).sum()))
    norm = torch.stack([CV.to_tensor_normalize(c) for c in got])
    assert torch.equal(rgb.cpu(), norm)


SIDES = [448, 224, 480, 300, 130, 34, 2]


@pytest.mark.parametrize("side", SIDES)
def test_resize_sides_and_borders(dev, side):
    img, depth, masks = _scene(side, 6)
    c = (H - side) // 2
    bbox = [[0, side, 0, side], [H - side, H, W - side, W], [0, side, W - side, W], [H - side, H, 0, side], [c, c + side, 77, 77 + side],
            [c, c + side, 3, 3 + side]]
    _check(dev, img, depth, masks, bbox)


def test_resize_mask_flag_off_grayscale_and_rectangles(dev):
    img, depth, masks = _scene(11, 5)
    bbox = [[10, 130, 20, 420], [0, 480, 0, 640], [100, 101, 5, 6], [200, 232, 300, 301], [50, 50, 60, 80]]  # the last one empty
    _check(dev, img, depth, masks, bbox, flag=False)
    _check(dev, img, depth, masks, bbox)
    gray = np.ascontiguousarray(img[:, :, 1])
    _check(dev, gray, depth, masks, bbox)
    _check(dev, img, depth, masks, bbox, S=100)  # img_size not a multiple of 4: the scalar store path


@pytest.mark.parametrize("N", [1, 32])
def test_resize_proposals_from_geometry(dev, N):
    img, depth, masks = _scene(20 + N, N)
    geom = inputs.proposal_geometry(torch.from_numpy(masks).to(dev), torch.from_numpy(depth).to(dev), K, 0.1)
    _check(dev, img, depth, masks, geom["bbox"].cpu().tolist())


# ------------------------------------------------------------------------------------------------------- assembled inputs
CFG = dict(img_size=224, n_sample_observed_point=2048, n_sample_template_point=5000, rgb_mask_flag=True)


def _detections(seed):
    img, depth, masks = _scene(seed, 32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, (cy, cx, r) in enumerate(((240, 320, 60), (100, 150, 40), (400, 500, 70))):
        masks[i] = (((xx - cx) ** 2 + (yy - cy) ** 2) < r * r) * (i + 1)
    masks[3] = 0
    masks[3, 100:105, 100:106] = 1  # 30 pixels: skipped by the 32-pixel rule
    masks[7] = 0
    masks[7, 10:14, 10:20] = 1  # 44 pixels, but no 4 of them within radius * 1.2 of their mean: skipped by the 4-point rule
    masks[7, 400:402, 600:602] = 1
    depth[10:14, 10:20] = 40.0
    depth[400:402, 600:602] = 0.5
    scores = np.random.default_rng(seed).random(32)
    g = np.random.default_rng(seed + 1)
    model = ((g.random((1024, 3)) - 0.5) * 0.12).astype(np.float32)
    return img, depth, masks, scores, model


def _device_test_data(dev, img, depth, masks, scores, model, seed):
    np.random.seed(seed)
    return inputs.test_data(torch.from_numpy(img).to(dev), torch.from_numpy(depth).to(dev), K, torch.from_numpy(masks).to(dev), scores,
                            model, CFG)


def test_test_data_matches_reference_composition(dev):
    img, depth, masks, scores, model = _detections(5)
    got, kept = _device_test_data(dev, img, depth, masks, scores, model, 1234)
    np.random.seed(1234)
    want, wkept, _ = CV.get_test_data(img, depth, K, masks, scores, model)
    assert kept == wkept and 3 not in kept and 7 not in kept and len(kept) >= 16
    for k in ("pts", "rgb", "rgb_choose", "score", "model", "K"):
        assert got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k].cpu(), want[k]), k


def _templates(seed, T=42, h=120, w=160):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = g.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    masks = np.zeros((T, h, w), np.uint8)
    for t in range(T):
        r = 20 if t == 5 else g.integers(45, 60)  # template 5: < 5000 mask pixels (the with-replacement draw)
        cy, cx = g.integers(40, h - 40), g.integers(50, w - 50)
        m = ((xx - cx) ** 2 + (yy - cy) ** 2) < r * r
        masks[t] = np.where(m, 255, np.where(g.random((h, w)) < 0.02, 128, 0))  # stray non-255 values are not the object
    xyz = ((g.random((T, h, w, 3)) - 0.5) * 200.0).astype(np.float32)
    return imgs, masks, xyz


def _device_templates(dev, imgs, masks, xyz, seed):
    np.random.seed(seed)
    return inputs.templates(torch.from_numpy(imgs).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(xyz).to(dev), CFG)


def _host_templates(imgs, masks, xyz, seed):
    np.random.seed(seed)
    out = [CV.get_template(imgs[t], masks[t], xyz[t]) for t in range(imgs.shape[0])]
    return ([o[1].unsqueeze(0) for o in out], [torch.FloatTensor(o[3]).unsqueeze(0) for o in out],
            [torch.from_numpy(o[2]).long().unsqueeze(0) for o in out])


def test_templates_match_reference_composition(dev):
    imgs, masks, xyz = _templates(9)
    assert int((masks[5] == 255).sum()) < 5000 < int((masks[0] == 255).sum())
    got = _device_templates(dev, imgs, masks, xyz, 77)
    want = _host_templates(imgs, masks, xyz, 77)
    for a, b, what in zip(got, want, ("rgb", "pts", "choose")):
        assert len(a) == 42
        for t in range(42):
            assert a[t].shape == b[t].shape and a[t].dtype == b[t].dtype, (what, t)
            assert torch.equal(a[t].cpu(), b[t]), (what, t)


def test_forward_seam_device_vs_host_inputs(dev):
    """get_obj_feats + Net.forward on the device-built inputs and on the host-built ones: the same (R, t, score), bitwise."""
    torch.manual_seed(0)
    net = importlib.import_module("pose_estimation_model").Net(synth.default_model_cfg())
    net.load_state_dict(synth.make_pem_weights(1), strict=False)
    net = net.to(dev).eval()
    imgs, masks, xyz = _templates(13)
    img, depth, dmasks, scores, model = _detections(17)
    dev_tem = _device_templates(dev, imgs, masks, xyz, 3)
    host_tem = [[t.to(dev) for t in lst] for lst in _host_templates(imgs, masks, xyz, 3)]
    d, _ = _device_test_data(dev, img, depth, dmasks[:4], scores, model, 4)
    np.random.seed(4)
    h = {k: v.to(dev) for k, v in CV.get_test_data(img, depth, K, dmasks[:4], scores, model)[0].items()}
    B = d["pts"].shape[0]
    assert B >= 2
    rand = torch.rand(B, 18000, generator=torch.Generator().manual_seed(8)).to(dev)
    res = []
    for tem, data in ((dev_tem, d), (host_tem, h)):
        net.coarse_point_matching.hypothesis_rand = rand
        try:
            with torch.no_grad():
                po, fo = net.feature_extraction.get_obj_feats(*tem)[:2]
                res.append(net(data["pts"], data["rgb"], data["rgb_choose"], data["model"], po.repeat(B, 1, 1), fo.repeat(B, 1, 1)))
        finally:
            net.coarse_point_matching.hypothesis_rand = None
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_error_contract(dev):
    img, depth, masks = _scene(1, 2)
    geom = dict(bbox=torch.tensor([[0, 10, 0, 10], [0, 10, 0, 10]], dtype=torch.int32, device=dev))
    ti, tm, td = torch.from_numpy(img), torch.from_numpy(masks), torch.from_numpy(depth)
    with pytest.raises(RuntimeError):
        inputs.proposal_rgb(ti, tm, td, dict(bbox=geom["bbox"].cpu()))
    with pytest.raises(RuntimeError):
        inputs.proposal_rgb(ti.to(dev).float(), tm.to(dev), td.to(dev), geom)
    with pytest.raises(RuntimeError):
        inputs.proposal_rgb(ti.to(dev), tm.to(dev), td.to(dev).double(), geom)
    with pytest.raises(RuntimeError):
        inputs.proposal_rgb(ti.to(dev), tm.to(dev), td.to(dev), dict(bbox=geom["bbox"].float()))
    for bad in ([0, 10, 630, 641], [-1, 9, 0, 10], [470, 481, 0, 10], [20, 10, 0, 10]):
        b = torch.tensor([[0, 10, 0, 10], bad], dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError):
            inputs.proposal_rgb(ti.to(dev), tm.to(dev), td.to(dev), dict(bbox=b))
    imgs, tmasks, xyz = _templates(2, T=2)
    with pytest.raises(RuntimeError):
        inputs.template_inputs(torch.from_numpy(imgs), torch.from_numpy(tmasks), torch.from_numpy(xyz), torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        inputs.template_inputs(torch.from_numpy(imgs).to(dev), torch.from_numpy(tmasks).to(dev), torch.from_numpy(xyz).to(dev).double(),
                               torch.zeros(2, 8, dtype=torch.int32, device=dev))
