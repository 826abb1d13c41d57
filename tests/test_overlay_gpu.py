"""Result images on the device (sam6d_hip.visualize over csrc/overlay.hip) against the numpy restatements of the recipes
(tests/overlay_ref.py): every comparison is torch.equal, there is no tolerance anywhere.  The images are 61 x 83 and 37 x 53 (no
dimension a multiple of 4, 16 or 64), so every case runs in well under a second."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import overlay_ref as OR
from tests._util import PKG  # noqa: F401  (sys.path)
from sam6d_hip import _lib, inputs, visualize as V

pytestmark = pytest.mark.gpu

H, W = 61, 83
EYE = np.eye(3, dtype=np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _image(h=H, w=W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _equal(got, want, what):
    w = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    assert got.dtype == w.dtype and got.shape == w.shape, (what, got.dtype, got.shape, w.dtype, w.shape)
    assert torch.equal(got, w), (what, int((got != w).sum()))


# ------------------------------------------------------------------------------------------------------------ mask overlay
def _check_masks(dev, rgb, masks, colors, edge=True, alpha=0.33, rgb_dev=None):
    got = V.overlay_masks(_t(rgb, dev) if rgb_dev is None else rgb_dev, _t(masks, dev), colors=colors, alpha=alpha, edge=edge)
    cols = np.broadcast_to(np.asarray(colors), (len(masks), 3))
    lut = np.stack([V.blend_table(c, alpha) for c in cols]) if len(masks) else np.zeros((0, 3, 256), np.uint8)
    want = OR.overlay_masks(rgb, masks, lut, edge)
    _equal(got, want, "overlay_masks")
    return want


def _single_masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    cases = {}
    m = np.zeros((h, w), np.uint8)
    m[0:h, 3:w - 2] = 1
    m[5:h - 7, 0:w] = 1
    cases["touches all four borders"] = m
    m = np.zeros((h, w), np.uint8)
    m[h // 2, w // 3] = 1
    cases["one pixel"] = m
    cases["full image"] = np.ones((h, w), np.uint8)
    cases["empty"] = np.zeros((h, w), np.uint8)
    cases["checkerboard"] = ((yy + xx) % 2).astype(np.uint8)
    m = np.zeros((h, w), np.uint8)
    m[h - 1, :] = 1
    m[:, w - 1] = 1
    cases["last row and last column"] = m
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 255  # any non-zero byte is inside
    cases["the four corners"] = m
    return cases


@pytest.mark.parametrize("case", list(_single_masks(2, 2)))
@pytest.mark.parametrize("size", [(H, W), (37, 53)])
def test_mask_overlay_single(dev, case, size):
    rgb = _image(*size, seed=1)
    m = _single_masks(*size)[case]
    want = _check_masks(dev, rgb, m[None], (200, 90, 17))
    right = want[:, size[1]:]
    if case == "full image":  # no edge at all, by the border rule: every pixel is the blend
        assert np.array_equal(OR.mask_edge(m), np.zeros(size, bool))
    if case == "empty":
        g = OR.grey(rgb)
        assert np.array_equal(right, np.stack([g, g, g], -1).astype(np.uint8))


def test_mask_overlay_bool_masks_and_default_palette(dev):
    rgb = _image(seed=2)
    m = _single_masks(H, W)["touches all four borders"][None]
    got = V.overlay_masks(_t(rgb, dev), _t(m.astype(bool), dev))
    _equal(got, OR.overlay_masks(rgb, m, np.stack([V.blend_table(V.palette(1)[0])])), "bool masks")


def test_mask_overlay_three_overlapping(dev):
    """the last mask wins the blend, the edges come from any mask -- also from one that is covered"""
    rgb = _image(seed=3)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([(yy - 25) ** 2 + (xx - 30) ** 2 <= 18 ** 2, (yy - 30) ** 2 + (xx - 45) ** 2 <= 20 ** 2,
                      (abs(yy - 28) <= 9) & (abs(xx - 38) <= 30)]).astype(np.uint8)
    colors = [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    want = _check_masks(dev, rgb, masks, colors)[:, W:]
    lut2 = V.blend_table(colors[2])
    g = OR.grey(rgb)
    assert want[28, 38].tolist() == [lut2[c][g[28, 38]] for c in range(3)]  # inside all three: the last one's colour
    e0 = OR.mask_edge(masks[0]) & (masks[2] != 0) & ~OR.mask_edge(masks[2]) & ~OR.mask_edge(masks[1])
    assert e0.any() and (want[e0] == 255).all()  # the first mask's edge shows through the last mask
    _check_masks(dev, rgb, masks[::-1].copy(), colors)


def test_mask_overlay_no_masks_and_no_edge(dev):
    rgb = _image(seed=4)
    want = _check_masks(dev, rgb, np.zeros((0, H, W), np.uint8), np.zeros((0, 3), np.uint8))
    g = OR.grey(rgb)
    assert np.array_equal(want[:, W:], np.stack([g, g, g], -1).astype(np.uint8)) and np.array_equal(want[:, :W], rgb)
    m = np.stack([_single_masks(H, W)["touches all four borders"], _single_masks(H, W)["checkerboard"]])
    _check_masks(dev, rgb, m, [(10, 200, 30), (250, 250, 0)], edge=False)
    _check_masks(dev, rgb, m, [(10, 200, 30), (250, 250, 0)], alpha=0.5)


def test_crop_view_row_stride(dev):
    big = _image(70, 100, seed=5)
    view = _t(big, dev)[5:5 + H, 9:9 + W]
    assert view.stride(0) == 300 and not view.is_contiguous()
    crop = np.ascontiguousarray(big[5:5 + H, 9:9 + W])
    _check_masks(dev, crop, _single_masks(H, W)["touches all four borders"][None], (200, 90, 17), rgb_dev=view)
    box = _line_box((10, 20), (60, 41))
    _check_draw(dev, crop, EYE[None], np.zeros((1, 3), np.float32), EYE[None], box, np.zeros((0, 3), np.float32), (255, 0, 0), rgb_dev=view)


# ------------------------------------------------------------------------------------------------------------ pose overlay
def _check_draw(dev, rgb, R, t, K, box, pts, colors, thickness=3, radius=1, rgb_dev=None):
    R, t, K, box, pts = (np.ascontiguousarray(a, dtype=np.float32) for a in (R, t, K, box, pts))
    got, skipped = V.draw_primitives(_t(rgb, dev) if rgb_dev is None else rgb_dev, _t(R, dev), _t(t, dev), _t(K, dev), _t(box, dev),
                                     _t(pts.reshape(-1, 3), dev), colors, thickness, radius)
    want, want_skipped = OR.draw_detections(rgb, R, t, K, box, pts.reshape(-1, 3), colors, thickness, radius)
    _equal(skipped, want_skipped, "n_skipped")
    _equal(got, want, "canvas")
    return want, want_skipped


def _line_box(a, b, za=1.0, zb=1.0):
    """a box whose top corners all project to pixel a and whose ground corners to pixel b under K = I and the identity pose: the
    pillars are the line a -> b, the top and ground edges its end discs"""
    return np.array([[a[0] * za, a[1] * za, za]] * 4 + [[b[0] * zb, b[1] * zb, zb]] * 4, np.float32)


def _identity(n):
    return np.broadcast_to(EYE, (n, 3, 3)).copy(), np.zeros((n, 3), np.float32), np.broadcast_to(EYE, (n, 3, 3)).copy()


NO_PTS = np.zeros((0, 3), np.float32)
LINES = {
    "horizontal": ((10, 20), (60, 20)), "horizontal reversed": ((60, 33), (10, 33)), "vertical": ((30, 5), (30, 50)),
    "45 degrees": ((10, 10), (50, 50)), "135 degrees": ((70, 10), (30, 50)), "slope 1/7": ((5, 10), (75, 20)),
    "slope -1/7": ((75, 30), (5, 40)), "slope 7": ((20, 3), (27, 52)), "slope -7": ((60, 55), (67, 6)), "zero length": ((40, 30), (40, 30)),
    "clipped at both ends": ((-5, -5), (W + 4, H + 9)), "wholly outside, left": ((-50, -20), (-10, -30)),
    "wholly outside, right": ((W + 20, 70), (300, 90)), "just outside": ((W + 1, 10), (W + 1, 40)),
    "along the last row": ((3, H - 1), (W - 4, H - 1)), "ends at 8191": ((8191, 30), (40, 31)), "ends at -8192": ((-8192, -8192), (20, 20)),
}


@pytest.mark.parametrize("thickness", [1, 2, 3, 6, 15])
@pytest.mark.parametrize("name", list(LINES))
def test_single_lines(dev, name, thickness):
    a, b = LINES[name]
    R, t, K = _identity(1)
    want, skipped = _check_draw(dev, _image(seed=6), R, t, K, _line_box(a, b), NO_PTS, (250, 120, 40), thickness=thickness)
    assert skipped.tolist() == [0]
    if name.startswith("wholly outside"):
        assert np.array_equal(want[:, W:], want[:, :W])


def test_single_lines_on_the_small_image(dev):
    rgb = _image(37, 53, seed=7)
    R, t, K = _identity(4)
    boxes = [_line_box((2, 3), (50, 30)), _line_box((50, 3), (2, 33)), _line_box((-9, 18), (70, 18)), _line_box((26, -4), (26, 44))]
    for T in (1, 4):
        for box in boxes:
            _check_draw(dev, rgb, R[:1], t[:1], K[:1], box, NO_PTS, (9, 250, 99), thickness=T)


def test_skipped_endpoints_are_counted(dev):
    """8191 is kept and 8192 skipped; q2 = 0 and q2 < 0 are skipped: the count is the numpy projection's"""
    rgb = _image(seed=8)
    R, t, K = _identity(1)
    pts = np.array([[1, 1, 0], [1, 1, -1], [40, 30, 1], [8192, 3, 1], [3, 8192, 1], [3, -8193, 1], [np.nan, 1, 1], [-8192, 8191, 1]], np.float32)
    _, _, kept = OR.project(EYE, np.zeros(3), EYE, pts)
    assert kept.tolist() == [False, False, True, False, False, False, False, True]
    # the ground corners are skipped: four ground edges and four pillars are not drawn, the top discs are
    _, skipped = _check_draw(dev, rgb, R, t, K, _line_box((40, 31), (8192, 30)), pts, (250, 120, 40))
    assert skipped.tolist() == [8 + 6]
    _, skipped = _check_draw(dev, rgb, R, t, K, _line_box((40, 31), (8191, 30)), pts[:3], (250, 120, 40))
    assert skipped.tolist() == [2]
    for zb in (0.0, -1.0):  # a corner on and behind the camera plane
        box = _line_box((40, 31), (20, 10), zb=zb)
        if zb == 0.0:
            box[4:, :2] = (20, 10)
        _, skipped = _check_draw(dev, rgb, R, t, K, box, NO_PTS, (250, 120, 40))
        assert skipped.tolist() == [8]


def _pose(rng, center, z):
    A = rng.randn(3, 3)
    Q, _r = np.linalg.qr(A)
    return (Q * np.sign(np.linalg.det(Q))).astype(np.float32), np.array([center[0], center[1], z], np.float32)


CAM = np.array([[100.0, 0, 41.5], [0, 100.0, 30.5], [0, 0, 1]], np.float32)


def test_three_overlapping_boxes(dev):
    """instance order, then stage order inside an instance (a top edge over a pillar of the same box), then the points over all"""
    rng = np.random.RandomState(12)
    model = rng.uniform(-0.1, 0.1, size=(300, 3)).astype(np.float32) * np.array([1.0, 0.7, 0.5], np.float32)
    box = V.box_corners(model).astype(np.float32)
    poses = [_pose(rng, c, z) for c, z in (((-0.02, 0.0), 0.55), ((0.03, 0.02), 0.6), ((0.0, -0.03), 0.5))]
    R, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    K = np.broadcast_to(CAM, (3, 3, 3)).copy()
    colors = [(255, 0, 0), (0, 255, 0), (40, 80, 255)]
    rgb = _image(seed=9)
    want, skipped = _check_draw(dev, rgb, R, t, K, box, model[:64], colors)
    assert skipped.tolist() == [0, 0, 0]
    right = want[:, W:].reshape(-1, 3)
    seen = {tuple(c) for c in right.tolist()}
    for col in colors:  # all three shades of every instance survive somewhere
        for sh in OR.shades(col)[:3]:
            assert sh in seen, (col, sh)
    # the same scene drawn in the other order differs: instance order is what decides
    want_rev, _ = _check_draw(dev, rgb, R[::-1], t[::-1], K, box, model[:64], colors[::-1])
    assert not np.array_equal(want_rev, want)
    # a top edge crosses a pillar of the same box: one instance whose top edge (0,1) runs over its pillar (2,6)
    cross = np.array([[10, 30, 1], [70, 30, 1], [40, 5, 1], [41, 5, 1], [10, 31, 1], [70, 31, 1], [40, 55, 1], [41, 55, 1]], np.float32)
    Ri, ti, Ki = _identity(1)
    want, _ = _check_draw(dev, rgb, Ri, ti, Ki, cross, NO_PTS, (200, 100, 50))
    assert want[30, W + 40].tolist() == [200, 100, 50] and want[20, W + 40].tolist() == [120, 60, 30]


@pytest.mark.parametrize("radius", [0, 1, 3, 15])
def test_points(dev, radius):
    rng = np.random.RandomState(13)
    model = rng.uniform(-0.3, 0.3, size=(700, 3)).astype(np.float32)  # wider than the image: discs are clipped at every border
    R, t = _pose(rng, (0.0, 0.0), 0.7)
    box = V.box_corners(model).astype(np.float32)
    want, skipped = _check_draw(dev, _image(seed=10), R[None], t[None], CAM[None], box, model, (255, 255, 0), radius=radius)
    assert skipped.tolist() == [0]
    u, v, _ = OR.project(R, t, CAM, model)
    assert ((u < 0) | (u >= W) | (v < 0) | (v >= H)).any() and ((u >= 0) & (u < W) & (v >= 0) & (v < H)).sum() > 100


def test_nothing_to_draw(dev):
    rgb = _image(seed=11)
    R, t, K = _identity(2)
    want, _ = _check_draw(dev, rgb, R[:0], t[:0], K[:0], _line_box((1, 1), (5, 5)), NO_PTS, (255, 0, 0))
    assert np.array_equal(want[:, W:], rgb) and np.array_equal(want[:, :W], rgb)
    want, _ = _check_draw(dev, rgb, R[:0], t[:0], K[:0], _line_box((1, 1), (5, 5)), np.ones((5, 3), np.float32), (255, 0, 0))
    assert np.array_equal(want[:, W:], rgb)
    _check_draw(dev, rgb, R, t, K, _line_box((10, 10), (70, 50)), NO_PTS, [(255, 0, 0), (0, 0, 255)])  # P = 0


# ------------------------------------------------------------------------------------------------------------ the C entry itself
def _raw_draw(dev, rgb, box, pts, canvas, ws, ws_bytes, h=H, w=W, thickness=3, n=2):
    R, t, K = (_t(a, dev) for a in _identity(n))
    cols = _t(np.array([(255, 0, 0), (0, 200, 255)][:n], np.uint8), dev)
    skipped = torch.full((n,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sam6d_draw_detections(rgb.data_ptr(), 3 * W, h, w, R.data_ptr(), t.data_ptr(), K.data_ptr(), n, box.data_ptr(),
                                               pts.data_ptr(), pts.shape[0], cols.data_ptr(), thickness, 1, canvas.data_ptr(),
                                               skipped.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return rc, skipped


def test_every_byte_is_written_and_nothing_is_left_to_order(dev):
    rgb = _t(_image(seed=14), dev)
    box = _t(_line_box((-5, -5), (W + 4, H + 9)), dev)
    pts = _t(np.random.RandomState(15).uniform(0, 1, size=(700, 3)).astype(np.float32) * np.array([W, H, 0], np.float32) + np.array([0, 0, 1], np.float32), dev)
    need = _lib.load().sam6d_draw_detections_workspace_bytes(H, W)
    assert need == H * W * 4
    out = []
    for fill in (0x00, 0xAB):
        canvas = torch.full((H, 2 * W, 3), fill, dtype=torch.uint8, device=dev)
        ws = torch.full((need // 4 + 3,), fill * 0x01010101 & 0x7FFFFFFF, dtype=torch.int32, device=dev)
        rc, skipped = _raw_draw(dev, rgb, box, pts, canvas, ws, need)
        assert rc == 0 and skipped.tolist() == [0, 0]
        out.append(canvas)
    assert torch.equal(out[0], out[1])
    # the mask overlay writes every byte too
    m = _t(_single_masks(H, W)["checkerboard"][None], dev)
    a = V.overlay_masks(rgb, m, (1, 2, 3))
    b = V.overlay_masks(rgb, m, (1, 2, 3))
    assert torch.equal(a, b)


def test_refusals_leave_the_canvas_untouched(dev):
    lib = _lib.load()
    for h, w in ((0, 5), (5, 0), (8193, 5), (5, 8193), (-1, -1)):
        assert lib.sam6d_draw_detections_workspace_bytes(h, w) == 0
    assert lib.sam6d_draw_detections_workspace_bytes(8192, 8192) == 8192 * 8192 * 4
    rgb = _t(_image(seed=16), dev)
    box, pts = _t(_line_box((5, 5), (50, 50)), dev), _t(np.ones((4, 3), np.float32), dev)
    need = H * W * 4
    ws = torch.zeros((need // 4,), dtype=torch.int32, device=dev)
    for kw, ws_bytes in ((dict(), need - 4), (dict(thickness=16), need), (dict(thickness=0), need), (dict(h=8193), need), (dict(w=0), need)):
        canvas = torch.full((H, 2 * W, 3), 0x5A, dtype=torch.uint8, device=dev)
        rc, skipped = _raw_draw(dev, rgb, box, pts, canvas, ws, ws_bytes, **kw)
        assert rc != 0, kw
        assert bool((canvas == 0x5A).all()) and skipped.tolist() == [-7, -7], kw
    canvas = torch.full((H, 2 * W, 3), 0x5A, dtype=torch.uint8, device=dev)
    m = torch.ones((1, H, W), dtype=torch.uint8, device=dev)
    lut = torch.zeros((1, 3, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream
        for h, w, M, stride in ((8193, W, 1, 3 * W), (H, W, 4097, 3 * W), (H, W, -1, 3 * W), (H, W, 1, 3 * W - 1)):
            assert lib.sam6d_overlay_masks(rgb.data_ptr(), stride, h, w, m.data_ptr(), M, lut.data_ptr(), 1, canvas.data_ptr(), s) != 0
        torch.cuda.synchronize()
    assert bool((canvas == 0x5A).all())
    with pytest.raises(ValueError, match="not contiguous"):
        V.overlay_masks(rgb, torch.ones((1, W, H), dtype=torch.uint8, device=dev).transpose(1, 2))
    with pytest.raises(ValueError, match="must have shape"):
        V.overlay_masks(rgb, m[:, :-1])


# ------------------------------------------------------------------------------------------------------------ end to end
def _scene(dev):
    h, w = 48, 64
    rgb = _image(h, w, seed=20)
    yy, xx = np.mgrid[0:h, 0:w]
    masks = np.stack([(yy - 20) ** 2 + (xx - 20) ** 2 <= 100, (abs(yy - 30) < 10) & (abs(xx - 40) < 15), (yy > 40) & (xx > 50)]).astype(np.uint8)
    return h, w, rgb, masks


def test_vis_ism_end_to_end(dev, tmp_path):
    from PIL import Image
    from sam6d_hip import ism
    U = importlib.import_module("model.utils")
    h, w, rgb, masks = _scene(dev)
    scores = [0.4, 0.9, 0.9]
    object_ids = [2, 0, 1]
    det = U.Detections({"masks": _t(masks, dev), "boxes": torch.zeros((3, 4), device=dev), "scores": torch.tensor(scores, device=dev),
                        "object_ids": torch.tensor(object_ids, device=dev)})
    path = os.path.join(str(tmp_path), "vis_ism.png")
    img = V.vis_ism(Image.fromarray(rgb), det, save_path=path)
    assert img.size == (2 * w, h)
    canvas = V.overlay_masks(_t(rgb, dev), _t(masks[1:2], dev), colors=V.palette(3)[0])  # the first of the two best, category 1
    _equal(canvas, OR.overlay_masks(rgb, masks[1:2], np.stack([V.blend_table(V.palette(3)[0])])), "vis_ism canvas")
    assert np.array_equal(np.asarray(img), canvas.cpu().numpy())
    assert np.array_equal(np.asarray(img)[:, :w], rgb)
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), canvas.cpu().numpy())
    rles = ism.mask_to_rle(_t(masks, dev))
    dicts = [dict(score=s, category_id=o + 1, segmentation=r) for s, o, r in zip(scores, object_ids, rles)]
    img2 = V.vis_ism(rgb, dicts)
    assert np.array_equal(np.asarray(img2), np.asarray(img))
    with pytest.raises(ValueError, match="no detection"):
        V.vis_ism(rgb, [dict(d, score=0.0) for d in dicts])


def _pem_scene():
    rng = np.random.RandomState(21)
    model = (rng.uniform(-1, 1, size=(900, 3)) * (60, 40, 30)).astype(np.float32)  # millimetres
    K = np.array([[80.0, 0, 32.0], [0, 80.0, 24.0], [0, 0, 1]], np.float32)
    poses = [_pose(rng, (-40.0, 10.0), 420.0), _pose(rng, (60.0, -20.0), 500.0)]
    return model, np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]), np.broadcast_to(K, (2, 3, 3)).copy()


def test_vis_pem_end_to_end(dev, tmp_path):
    from PIL import Image
    h, w, rgb, _ = _scene(dev)
    model, R, t, K = _pem_scene()
    path = os.path.join(str(tmp_path), "vis_pem.png")
    np.random.seed(5)
    img = V.vis_pem(rgb, R, t, model, K, save_path=path)
    assert img.size == (2 * w, h)
    np.random.seed(5)
    choose = np.random.choice(np.arange(len(model)), 512)  # the reference's own call (draw_utils.py:84)
    want, _ = OR.draw_detections(rgb, R, t, K, V.box_corners(model).astype(np.float32), model[choose], (255, 0, 0))
    assert np.array_equal(np.asarray(img), want) and not np.array_equal(want[:, w:], rgb)
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), want)
    np.random.seed(5)
    canvas, skipped = V.draw_detections(_t(rgb, dev), _t(R, dev), _t(t, dev), _t(model, dev), _t(K, dev))
    _equal(canvas, want, "draw_detections with device model points")
    assert skipped.tolist() == [0, 0]
    # the choice drawn on the device: the picture of exactly those points
    canvas, _ = V.draw_detections(_t(rgb, dev), _t(R, dev), _t(t, dev), model, _t(K, dev), colors=[(255, 0, 0), (0, 255, 0)], n_points=100,
                                  rng=inputs.DeviceChoice(3))
    sel = inputs.draw_choice(torch.tensor([len(model)], dtype=torch.int32, device=dev), 100, 3)[0].cpu().numpy()
    want2, _ = OR.draw_detections(rgb, R, t, K, V.box_corners(model).astype(np.float32), model[sel], [(255, 0, 0), (0, 255, 0)])
    _equal(canvas, want2, "draw_detections with DeviceChoice")


def test_drop_in_draw_utils(dev):
    draw_utils = importlib.import_module("draw_utils")
    h, w, rgb, _ = _scene(dev)
    model, R, t, K = _pem_scene()
    np.random.seed(9)
    got = draw_utils.draw_detections(rgb, R.astype(np.float64), t.astype(np.float64), model, K, color=(0, 255, 0))
    np.random.seed(9)
    choose = np.random.choice(np.arange(len(model)), 512)
    want, _ = OR.draw_detections(rgb, R, t, K, V.box_corners(model).astype(np.float32), model[choose], (0, 255, 0))
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, want[:, w:])
