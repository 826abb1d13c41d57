"""Result images (sam6d_hip.visualize, csrc/overlay.hip): the host side and the numpy restatement of the recipes (tests/overlay_ref.py).
No GPU: the tables, the palette, the box corners, the refusals, the fp32 projection against the reference's float64 recipe and the
painter's own invariants against hand-made arrays."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import overlay_ref as OR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import visualize as V


def test_grey_values():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert OR.grey(px).tolist() == [[76, 150, 29, 255, 0]]


def test_blend_table_is_the_reference_expression():
    tab = V.blend_table((200, 200, 17), 0.33)
    assert tab.shape == (3, 256) and tab.dtype == np.uint8
    assert tab[0, :5].tolist() == [66, 66, 67, 68, 68] and tab[0, -3:].tolist() == [235, 236, 236]
    img = np.arange(256, dtype=np.uint8)
    for c, col in enumerate((200, 200, 17)):
        want = img.copy()
        sel = np.ones(256, bool)
        want[sel] = 0.33 * col + (1 - 0.33) * img[sel]  # ISM/run_inference_custom.py:70-72
        assert np.array_equal(tab[c], want)


def test_shades_are_integer_quotients():
    """the device's (c * 3) / 10 and (c * 6) / 10 are Python's int(c * 0.3) and int(c * 0.6) for every byte"""
    for c in range(256):
        assert int(c * 0.3) == (c * 3) // 10 and int(c * 0.6) == (c * 6) // 10, c


def test_dilation_is_scipys():
    e0 = np.zeros((5, 5), bool)
    e0[2, 2] = True
    got = ndimage.binary_dilation(e0, np.ones((2, 2)))
    want = np.zeros((5, 5), bool)
    want[1:3, 1:3] = True
    assert np.array_equal(got, want)
    # the recipe's OR over (y + dy, x + dx), dy, dx in {0, 1}, is that dilation on any input
    rng = np.random.RandomState(3)
    for shape in ((5, 5), (1, 7), (7, 1), (9, 6)):
        a = rng.rand(*shape) < 0.3
        pad = np.zeros((shape[0] + 1, shape[1] + 1), bool)
        pad[:-1, :-1] = a
        mine = pad[:-1, :-1] | pad[1:, :-1] | pad[:-1, 1:] | pad[1:, 1:]
        assert np.array_equal(mine, ndimage.binary_dilation(a, np.ones((2, 2))))


def test_edge0_ignores_the_image_border():
    assert not OR.edge0(np.ones((4, 6), bool)).any()
    m = np.zeros((4, 6), bool)
    m[0, 0] = True
    assert OR.edge0(m)[0, 0] and OR.edge0(m).sum() == 1
    m = np.ones((4, 6), bool)
    m[2, 3] = False
    want = np.zeros((4, 6), bool)
    want[1, 3] = want[3, 3] = want[2, 2] = want[2, 4] = True
    assert np.array_equal(OR.edge0(m), want)


def test_palette():
    p = V.palette(7)
    assert p.shape == (7, 3) and p.dtype == np.uint8
    assert p[0].tolist() == [255, 0, 0]
    assert (p.max(axis=1) == 255).all() and (p.min(axis=1) == 0).all()  # full value, full saturation
    assert len({tuple(c) for c in p.tolist()}) == 7
    assert np.array_equal(V.palette(3), p[:3]) and V.palette(0).shape == (0, 3)
    h = (1 * V.GOLDEN) % 1.0 * 6  # colour 1 by hand: hue 0.618 -> sector 3, (0, 1 - f, 1)
    assert int(h) == 3 and p[1].tolist() == [0, int(255 * (1 - (h - 3))), 255]


def test_box_corners():
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 0, 8], [2, 4, 8], [2, 4, 8]], np.float32)  # extent (2,4,8), mean (1,2,4)
    got = V.box_corners(pts)
    want = np.array([[2, 4, 8], [2, 4, 0], [0, 4, 8], [0, 4, 0], [2, 0, 8], [2, 0, 0], [0, 0, 8], [0, 0, 0]], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    shifted = pts + np.float32(0.5)
    shifted[4] = (4.5, 0.5, 0.5)  # the mean leaves the middle of the extent: the box is centred at the mean, as the reference's is
    c = V.box_corners(shifted)
    assert np.allclose(c.mean(axis=0), shifted.mean(axis=0)) and np.allclose(c.max(axis=0) - c.min(axis=0), (4, 4, 8))
    import draw_utils
    assert np.array_equal(draw_utils.get_3d_bbox(np.array([2.0, 4.0, 8.0]), np.array([1.0, 2.0, 4.0])), want.T)
    assert np.array_equal(draw_utils.get_3d_bbox(2.0), np.sign(want - [1, 2, 4]).T)  # a scalar scale: the cube of that side
    with pytest.raises(ValueError):
        V.box_corners(np.zeros((0, 3)))


def test_calculate_2d_projections_truncates():
    import draw_utils
    K = np.array([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1]])
    p = np.array([[1.9, -1.9], [0.3, -0.3], [2.0, 2.0]])  # (3, N): q = (4.8, 1.6, 2) and (-2.8, 0.4, 2)
    assert draw_utils.calculate_2d_projections(p, K).tolist() == [[2, 0], [-1, 0]]


def test_refusals_before_any_launch():
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    masks = torch.zeros((1, 4, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CPU"):
        V.overlay_masks(rgb, masks)
    with pytest.raises(ValueError, match="uint8"):
        V.overlay_masks(rgb.float(), masks)
    with pytest.raises(ValueError, match="torch tensor"):
        V.overlay_masks(np.zeros((4, 5, 3), np.uint8), masks)
    with pytest.raises(ValueError, match="not contiguous"):
        V.overlay_masks(torch.zeros((4, 3, 5), dtype=torch.uint8).permute(0, 2, 1), masks)
    with pytest.raises(ValueError, match="uint8 or bool"):
        V.overlay_masks(rgb, masks.float())
    with pytest.raises(ValueError, match="masks is not contiguous"):
        V.overlay_masks(rgb, torch.zeros((1, 5, 4), dtype=torch.uint8).permute(0, 2, 1))
    with pytest.raises(ValueError, match="R must be torch.float32"):
        V.draw_primitives(rgb, torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3), torch.eye(3)[None], torch.zeros(8, 3), torch.zeros(0, 3))
    with pytest.raises(ValueError, match="thickness = 16"):
        V.draw_primitives(rgb, torch.eye(3)[None], torch.zeros(1, 3), torch.eye(3)[None], torch.zeros(8, 3), torch.zeros(0, 3), thickness=16)
    eye = torch.eye(3)[None]
    with pytest.raises(ValueError, match="CPU"):
        V.draw_detections(rgb, eye, torch.zeros(1, 3), np.zeros((5, 3), np.float32), eye)
    with pytest.raises(ValueError, match="CPU"):
        V.draw_primitives(rgb, eye, torch.zeros(1, 3), eye, torch.zeros(8, 3), torch.zeros(0, 3))
    with pytest.raises(ValueError, match="no detection"):
        V.vis_ism(np.zeros((4, 5, 3), np.uint8), [dict(score=0.0, category_id=1, segmentation=None)])
    with pytest.raises(ValueError, match="no detection"):
        V.best_detection([])
    assert V.best_detection([0.2, 0.7, 0.7, 0.1]) == 1  # the first of the strictly highest
    with pytest.raises(ValueError, match="colors"):
        V._colors([[1, 2, 3]], 2, "x")
    with pytest.raises(ValueError, match="0 .. 255"):
        V._colors((256, 0, 0), 1, "x")


def test_draw_utils_needs_a_device(monkeypatch):
    import draw_utils
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        draw_utils.draw_detections(np.zeros((4, 5, 3), np.uint8), np.eye(3)[None], np.zeros((1, 3)), np.zeros((5, 3)), np.eye(3)[None])


def test_fp32_projection_matches_the_float64_recipe():
    """The reference's recipe in float64 (K @ (R @ p + t), divide, cast to int32; draw_utils.py:13-16, :89-94) against the recipe's
    fp32, on points selected WITH THE FLOAT64 RECIPE ALONE: both quotients inside a 640 x 480 image with a fractional part in
    [0.01, 0.99].  Below 1000 px half a dozen fp32 roundings stay under 2e-3, far inside the 0.01 guard, so the integers are equal."""
    rng = np.random.RandomState(11)
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
    n_drawn = n_kept = 0
    for _ in range(8):
        A = rng.randn(3, 3)
        Q, _r = np.linalg.qr(A)
        R = Q * np.sign(np.linalg.det(Q))
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
        p = rng.uniform(-0.08, 0.08, size=(500, 3))
        R32, t32, K32, p32 = (a.astype(np.float32) for a in (R, t, K, p))
        q = K32.astype(np.float64) @ (R32.astype(np.float64) @ p32.astype(np.float64).T + t32.astype(np.float64)[:, None])
        uv = q[:2] / q[2]
        frac = uv - np.floor(uv)
        keep = ((frac >= 0.01) & (frac <= 0.99)).all(axis=0) & (uv[0] >= 0) & (uv[0] < 640) & (uv[1] >= 0) & (uv[1] < 480)
        want = np.array(uv.T, dtype=np.int32)
        u, v, ok = OR.project(R32, t32, K32, p32)
        assert ok[keep].all()
        assert np.array_equal(u[keep], want[keep, 0]) and np.array_equal(v[keep], want[keep, 1])
        n_drawn += len(p)
        n_kept += int(keep.sum())
    assert 2 * n_kept >= n_drawn, (n_kept, n_drawn)


def test_projection_skips():
    eye = np.eye(3, dtype=np.float32)
    z = np.zeros(3, np.float32)
    p = np.array([[8191, 0, 1], [8192, 0, 1], [-8192, 5, 1], [-8193, 5, 1], [1, 1, 0], [1, 1, -1], [3.9, -3.9, 1], [np.nan, 0, 1]], np.float32)
    u, v, ok = OR.project(eye, z, eye, p)
    assert ok.tolist() == [True, False, True, False, False, False, True, False]
    assert (u[0], u[2], v[2]) == (8191, -8192, 5) and (u[6], v[6]) == (3, -3)  # truncation toward zero


def _line(ax, ay, bx, by, T, n=9):
    YY, XX = np.mgrid[0:n, 0:n].astype(np.int64)
    return OR.in_line(ax, ay, bx, by, T, XX, YY)


def test_painter_invariants_on_9x9():
    want = np.zeros((9, 9), bool)
    want[3:6, 2:7] = True  # three rows over the segment x = 2 .. 6
    want[3:6, 1] = want[3:6, 7] = True  # the caps: 4 |w|^2 <= 9 holds for w = (-1, 0) and (-1, +-1), not for (-2, 0)
    assert np.array_equal(_line(2, 4, 6, 4, 3), want)
    assert np.array_equal(_line(6, 4, 2, 4, 3), want)        # direction does not matter
    assert np.array_equal(_line(4, 2, 4, 6, 3), want.T)      # vertical
    one = np.zeros((9, 9), bool)
    one[4, 2:7] = True
    assert np.array_equal(_line(2, 4, 6, 4, 1), one)         # T = 1: the pixels of the segment
    YY, XX = np.mgrid[0:9, 0:9].astype(np.int64)
    plus = np.zeros((9, 9), bool)
    plus[4, 3:6] = plus[3:6, 4] = True
    assert np.array_equal(OR.in_disc(4, 4, 1, XX, YY), plus) and plus.sum() == 5
    assert OR.in_disc(4, 4, 0, XX, YY).sum() == 1
    assert np.array_equal(_line(4, 4, 4, 4, 2), plus)        # a zero-length edge is the disc of radius T / 2
    diag = _line(1, 1, 7, 7, 1)
    assert np.array_equal(diag, np.eye(9, dtype=bool) & (np.arange(9) >= 1)[:, None] & (np.arange(9) <= 7)[:, None])


def test_sequential_painter_order_and_counts():
    """later paint wins in the restatement: top over pillar over ground, points over all, instance 1 over instance 0"""
    rgb = np.full((9, 9, 3), 7, np.uint8)
    eye = np.eye(3, dtype=np.float32)
    box = np.array([[4, 4, 1]] * 8, np.float32)  # every corner projects to (4, 4): all twelve edges are the same disc
    R, t, K = eye[None], np.zeros((1, 3), np.float32), eye[None]
    canvas, skipped = OR.draw_detections(rgb, R, t, K, box, np.zeros((0, 3), np.float32), (250, 100, 10), thickness=2, radius=1)
    assert canvas.shape == (9, 18, 3) and np.array_equal(canvas[:, :9], rgb) and skipped.tolist() == [0]
    assert canvas[4, 9 + 4].tolist() == [250, 100, 10] and canvas[0, 9].tolist() == [7, 7, 7]
    box2 = box.copy()
    box2[:4, 2] = 0  # the top corners lie on the camera plane: pillars and top edges are skipped, the ground stays
    pts = np.array([[4, 4, 1], [0, 0, -1]], np.float32)
    canvas, skipped = OR.draw_detections(rgb, R, t, K, box2, pts[1:], (250, 100, 10), thickness=2, radius=1)
    assert skipped.tolist() == [9] and canvas[4, 9 + 4].tolist() == [75, 30, 3]
    canvas, skipped = OR.draw_detections(rgb, np.concatenate([R, R]), np.concatenate([t, t]), np.concatenate([K, K]), box2, pts,
                                         [(250, 100, 10), (0, 200, 0)], thickness=2, radius=0)
    assert skipped.tolist() == [9, 9] and canvas[4, 9 + 4].tolist() == [0, 200, 0] and canvas[4, 9 + 5].tolist() == [0, 60, 0]
    windowed, _ = OR.draw_detections(rgb, np.concatenate([R, R]), np.concatenate([t, t]), np.concatenate([K, K]), box2, pts,
                                     [(250, 100, 10), (0, 200, 0)], thickness=2, radius=0, window=True)
    assert np.array_equal(windowed, canvas)


def test_mask_overlay_restatement():
    rgb = np.zeros((7, 8, 3), np.uint8)
    rgb[..., 0] = 255
    mask = np.zeros((1, 7, 8), np.uint8)
    mask[0, 2:7, 2:8] = 1  # reaches the lower and the right border
    lut = np.stack([V.blend_table((200, 100, 0), 0.33)])
    out = OR.overlay_masks(rgb, mask, lut)
    assert out.shape == (7, 16, 3) and np.array_equal(out[:, :8], rgb)
    right = out[:, 8:]
    blend = [int(66 + 0.67 * 76), int(33 + 0.67 * 76), int(0.67 * 76)]
    assert right[0, 0].tolist() == [76, 76, 76] and right[0, 7].tolist() == [76, 76, 76]  # outside: grey
    assert right[1, 1].tolist() == [255, 255, 255]   # the dilation reaches up and to the left of edge0 (2, 2)
    assert right[2, 2].tolist() == [255, 255, 255] and right[3, 3].tolist() == blend   # ... and not down or to the right
    assert right[6, 7].tolist() == blend             # the image corner: the border alone makes no edge
    assert right[6, 1].tolist() == [255, 255, 255] and right[6, 2].tolist() == [255, 255, 255] and right[6, 3].tolist() == blend
    assert np.array_equal(OR.overlay_masks(rgb, mask[:0], lut[:0])[:, 8:], np.full((7, 8, 3), 76, np.uint8))
    assert np.array_equal(OR.overlay_masks(rgb, mask, lut, draw_edge=False)[2:, 10:], np.broadcast_to(np.uint8(blend), (5, 6, 3)))


def test_kernel_resources():
    """none of the three kernels uses scratch or spills, each keeps within its built VGPR count rounded up
    to the next step of 8 (built: overlay_masks 20, draw_paint 46, draw_resolve 11), and the only vector atomics of the file are the
    painter's 32-bit unsigned max and the skip counter's add."""
    from tests._util import kernel_resources
    limits = dict(overlay_masks_kernel=24, draw_paint_kernel=48, draw_resolve_kernel=16)
    found, atomics = kernel_resources(b"draw_paint_kernel", r"((?:overlay|draw)_[a-z_]+_kernel)", disassemble=True)
    print("\n[overlay] (VGPRs, scratch bytes, spilled): %s; atomics %s" % (found, sorted(atomics)))
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
    assert atomics == {"global_atomic_umax", "global_atomic_add"}, atomics
