"""The pose check on the device (sam6d_hip.verify and visualize.vis_pem_render over csrc/verify.hip) against its numpy restatement
(tests/verify_ref.py) and against the template renderer (onboard.render_views) for the same views.  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import raster_ref as RR
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, onboard, verify
from sam6d_hip import visualize as V

pytestmark = pytest.mark.gpu

F32 = np.float32
TAU = 2.0 ** -6  # with depths in [2, 4) every r + TAU and r - TAU is a float32, so o - r is TAU exactly
BIG = (96, 128)
BIG_INTR = (120.0, 120.0, 64.0, 48.0)
PIXEL = (1.0, 1.0, 0.0, 0.0)  # intrinsics under which a vertex (x z, y z, z) lands at pixel coordinates (x, y)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F32)[None]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "octahedron":
        return RR.octahedron()
    if name == "quad":  # two triangles in the plane z = 2 that cover any image of the tests
        return np.array([[-3, -3, 2], [3, -3, 2], [-3, 3, 2], [3, 3, 2]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    return RR.icosphere(int(name[-1]))


def _run(dev, v, f, view, obs, masks=None, tau=TAU, intr=VR.INTR, near=1e-3, wave_area=0, want_map=True):
    """render_compare for the view matrices `view` (scale 1: R * 1.0f is R)"""
    view = np.asarray(view, F32)
    return verify.render_compare((_t(v, dev), _t(f, dev)), _t(view[:, :, :3], dev), _t(view[:, :, 3], dev), intr, _t(obs, dev),
                                 masks=_t(masks, dev), tol=tau, near=near, wave_area=wave_area, want_map=want_map)


def _want(v, f, view, obs, masks=None, tau=TAU, intr=VR.INTR, near=1e-3):
    """the restatement of render_compare: box, counts (column 7 from the windows), ids, depth"""
    size = obs.shape
    box, dropped = VR.windows(v, f, view, intr, size, near)
    counts, ids, depth = VR.pose_verify(v, f, view, intr, size, near, box, obs, masks, tau)
    if VR.areas(box, size).sum() > 0:
        assert np.array_equal(counts[:, 7], dropped)
    counts[:, 7] = dropped
    return box, counts, ids, depth


def _same(dev, got, want, maps=True):
    box, counts, ids, depth = want
    assert got.boxes.dtype == torch.int32 and torch.equal(got.boxes, _t(box, dev)), (got.boxes.cpu().numpy(), box)
    assert got.counts.dtype == torch.int32 and torch.equal(got.counts, _t(counts, dev)), (got.counts.cpu().numpy(), counts)
    if maps:
        assert got.ids.dtype == torch.int32 and torch.equal(got.ids, _t(ids, dev)), int((got.ids != _t(ids, dev)).sum())
        assert got.depth.dtype == torch.float32 and torch.equal(got.depth, _t(depth, dev))
    for k, w in VR.ratios(counts).items():
        assert torch.equal(getattr(got, k), _t(w, dev)), k


# ------------------------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize("mesh", ["octahedron", "icosphere2"])
def test_windows(dev, mesh):
    v, f = _mesh(mesh)
    view = VR.five_poses()
    box, dropped = verify.pose_windows(_t(v, dev), _t(f, dev), _t(view, dev), VR.INTR, VR.SIZE)
    wbox, wdropped = VR.windows(v, f, view, VR.INTR, VR.SIZE)
    assert box.dtype == torch.int32 and torch.equal(box, _t(wbox, dev)), (box.cpu().numpy(), wbox)
    assert dropped.dtype == torch.int32 and torch.equal(dropped, _t(wdropped, dev))
    assert wbox[3].tolist() == wbox[4].tolist() == [0, 0, -1, -1] and wdropped[2] > 0 and wbox[2, 2] >= wbox[2, 0]
    assert wbox[1, 2:].tolist() == [63, 47] and wdropped[4] == len(f)


# ------------------------------------------------------------------------------------------------------------ the renderer's geometry
def _px(points, z=1.0):
    p = np.asarray(points, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(p),))
    return np.stack([p[:, 0] * z, p[:, 1] * z, z], axis=1).astype(F32)


A, B, C, D = (0.5, 0.5), (6.5, 0.5), (0.5, 6.5), (6.5, 6.5)
GEOMETRY = {
    "one triangle through centres": (_px([A, B, C]), [[0, 1, 2]], EYE, PIXEL, (8, 8)),
    "shared edge": (_px([A, B, C, D]), [[0, 1, 2], [1, 3, 2]], EYE, PIXEL, (8, 8)),
    "shared edge, other winding": (_px([A, B, C, D], 2.0), [[0, 2, 1], [1, 2, 3]], EYE, PIXEL, (8, 8)),
    "octahedron inside": (None, "octahedron", VR.five_poses()[0:1], VR.INTR, VR.SIZE),
    "icosphere inside": (None, "icosphere2", VR.five_poses()[0:1], VR.INTR, VR.SIZE),
    "icosphere at the border": (None, "icosphere2", VR.five_poses()[1:2], VR.INTR, VR.SIZE),
    "icosphere through the camera plane": (None, "icosphere2", VR.five_poses()[2:3], VR.INTR, VR.SIZE),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_same_geometry_as_the_template_renderer(dev, case):
    """N = 1: ids >= 0 and depth are mask == 255 and depth of onboard.render_views for the same view, device against device"""
    v, f, view, intr, size = GEOMETRY[case]
    if v is None:
        v, f = _mesh(f)
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    got = _run(dev, v, f, view, np.ones(size, F32), intr=intr)
    ref = onboard.render_views(_t(v, dev), _t(f, dev), None, None, _t(view, dev), _t(np.zeros((1, 3), F32), dev), intr, size)
    assert torch.equal(got.ids >= 0, ref["mask"][0] == 255) and torch.equal(got.depth, ref["depth"][0])
    assert int(got.counts[0, 0]) == int((ref["mask"] == 255).sum()) > 0 and int(got.counts[0, 7]) == int(ref["n_dropped"][0])
    assert {0} <= set(got.ids.unique().tolist()) <= {-1, 0}  # (the pose through the camera plane covers the whole image)


# ------------------------------------------------------------------------------------------------------------ counts
@functools.lru_cache(maxsize=None)
def _counts_scene():
    """icosphere(2) at the five poses; depth_obs from the restatement's own render of pose 0: the upper left quadrant of the image
    at + 2 tau (the model lies in front of what is seen: behind), the upper right at - 2 tau (occluded), the lower left zeroed, the
    lower right as rendered, and single pixels at exactly + tau and - tau (inliers), 0, a negative value and NaN"""
    v, f = _mesh("icosphere2")
    view = VR.five_poses()
    mask, depth = VR.render_depth(v, f, view[0], VR.INTR, VR.SIZE)
    assert mask[26, 36] and mask[27, 37] and mask[28, 38] and mask[29, 39] and mask[30, 40] and depth[mask].max() + 2 * TAU < 4.0
    obs = depth.copy()
    obs[:24, :32] += F32(2 * TAU)
    obs[:24, 32:] -= F32(2 * TAU)
    obs[24:, :32] = 0
    obs[26, 36] = depth[26, 36] + F32(TAU)
    obs[27, 37] = depth[27, 37] - F32(TAU)
    obs[28, 38] = 0
    obs[29, 39] = -1.0
    obs[30, 40] = np.nan
    assert obs[26, 36] - depth[26, 36] == F32(TAU) and depth[27, 37] - obs[27, 37] == F32(TAU)
    g = np.random.default_rng(11)
    masks = np.stack([np.roll(VR.render_depth(v, f, M, VR.INTR, VR.SIZE)[0], (2, -3), (0, 1)) for M in view]).astype(np.uint8) * 255
    masks[4] = g.integers(0, 2, VR.SIZE, dtype=np.uint8) * 7
    return v, f, view, obs, masks


@pytest.mark.parametrize("with_masks", [False, True])
def test_counts(dev, with_masks):
    v, f, view, obs, masks = _counts_scene()
    masks = masks if with_masks else None
    want = _want(v, f, view, obs, masks)
    got = _run(dev, v, f, view, obs, masks)
    _same(dev, got, want)
    c = want[1]
    assert (c[0, 1:5] > 0).all() and c[0, 1:5].sum() == c[0, 0] and c[0, 4] >= 3
    assert c[2, 7] > 0 and not c[3].any() and c[4, :5].sum() == 0
    if with_masks:
        assert torch.equal(got.mask_iou, _t(VR.mask_iou(c), dev)) and c[4, 5] > 1000 and c[0, 6] > 0 and float(got.mask_iou[3]) == 0.0
        assert torch.equal(got.n_mask, _t(c[:, 5], dev)) and torch.equal(got.n_inter, _t(c[:, 6], dev))
    else:
        assert got.mask_iou is None and not c[:, 5:7].any()
    again = _run(dev, v, f, view, obs, masks, want_map=False)
    assert again.ids is None and again.depth is None
    _same(dev, again, want, maps=False)


# ------------------------------------------------------------------------------------------------------------ composite
def test_composite_ties_and_rows_alone(dev):
    """two identical poses (the lower index owns every shared pixel) and a nearer one that overlaps them"""
    v, f = _mesh("icosphere2")
    view = np.stack([VR.pose((0.1, -0.05, 4.0)), VR.pose((0.1, -0.05, 4.0)), VR.pose((0.6, 0.2, 3.2))])
    obs = np.full(VR.SIZE, 3.5, F32)
    want = _want(v, f, view, obs)
    got = _run(dev, v, f, view, obs)
    _same(dev, got, want)
    ids = want[2]
    assert (ids == 0).sum() > 100 and (ids == 1).sum() == 0 and (ids == 2).sum() > 100 and np.array_equal(want[1][0], want[1][1])
    assert want[1][0, 0] > (ids == 0).sum()  # the nearer pose hides part of pose 0
    for n in range(3):
        alone = _run(dev, v, f, view[n:n + 1], obs)
        assert torch.equal(alone.counts[0], got.counts[n]) and torch.equal(alone.boxes[0], got.boxes[n]), n


# ------------------------------------------------------------------------------------------------------------ both raster paths
@functools.lru_cache(maxsize=None)
def _paths_scene(mesh):
    v, f = _mesh(mesh)
    if mesh == "quad":
        view = np.concatenate([EYE, EYE + np.array([[[0, 0, 0, 0.25], [0, 0, 0, 0], [0, 0, 0, 0.5]]], F32)])
    else:
        view = np.stack([VR.pose((0.1, -0.05, 4.0)), VR.pose((1.7, 1.2, 3.5)), VR.pose((-0.4, 0.3, 3.0), angle=2.0)])
    obs = np.full(BIG, 3.0, F32)
    obs[:, 64:] = 2.0
    return v, f, view, obs, _want(v, f, view, obs, intr=BIG_INTR)


@pytest.mark.parametrize("mesh", ["icosphere3", "quad"])
def test_thread_and_wave_paths_agree(dev, mesh):
    v, f, view, obs, want = _paths_scene(mesh)
    assert len(f) == (1280 if mesh == "icosphere3" else 2)
    for wave_area in (0, 1, 2 ** 31 - 1):  # the default; every face by the wave; every face by its lane
        _same(dev, _run(dev, v, f, view, obs, intr=BIG_INTR, wave_area=wave_area), want)
    if mesh == "quad":
        assert want[0].tolist() == [[0, 0, 127, 95]] * 2 and (want[2] == 0).all() and (want[1][:, 0] == 96 * 128).all()


# ------------------------------------------------------------------------------------------------------------ layout
LAYOUT = {
    "a zero-area window between two others": [0, 3, 1],
    "zero-area windows first and last": [4, 0, 3],
    "one pose": [1],
    "every pose off-screen": [3, 4, 3],
}


@pytest.mark.parametrize("case", sorted(LAYOUT))
def test_window_layout(dev, case):
    """odd image sizes, so that masks[n] starts at every alignment; total = 0 writes zeros and background"""
    v, f = _mesh("icosphere2")
    view = VR.five_poses()[LAYOUT[case]]
    size = (45, 61)
    g = np.random.default_rng(3)
    obs = np.full(size, 3.4, F32)
    masks = (g.random((len(view),) + size) < 0.4).astype(np.uint8)
    want = _want(v, f, view, obs, masks)
    if case == "every pose off-screen":
        assert not want[1][:, :7].any() and (want[2] == -1).all() and not want[3].any() and want[1][1, 7] == len(f)
    else:
        assert want[1][:, 0].sum() > 0 and (want[1][:, 5] > 0).all()
    _same(dev, _run(dev, v, f, view, obs, masks), want)
    _same(dev, _run(dev, v, f, view, obs, torch.from_numpy(masks).bool().numpy()), want)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_guard_values_and_refusals(dev):
    v, f = _mesh("icosphere2")
    view = VR.five_poses()
    H, W = VR.SIZE
    N, G = len(view), 64
    obs = np.full(VR.SIZE, 3.4, F32)
    wbox, wdropped = VR.windows(v, f, view, VR.INTR, VR.SIZE)
    wcounts, wids, wdepth = VR.pose_verify(v, f, view, VR.INTR, VR.SIZE, 1e-3, wbox, obs, None, TAU)
    d = dict(v=_t(v, dev), f=_t(f, dev), view=_t(view, dev), obs=_t(obs, dev))
    sizes = dict(box=(N * 4, torch.int32), dropped=(N, torch.int32), counts=(N * 8, torch.int32), ids=(H * W, torch.int32),
                 depth=(H * W, torch.float32))
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
    offset = np.concatenate([[0], np.cumsum(VR.areas(wbox, VR.SIZE))]).astype(np.int64)
    total = int(offset[-1])
    d_offset = _t(offset, dev)
    need = _lib.load().sam6d_pose_verify_workspace_bytes(total, H, W)
    assert need == 8 * (total + H * W)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def windows(N=N, H=H, vert=d["v"].data_ptr(), box=ptr["box"], near=1e-3, F=len(f)):
        _lib.call("sam6d_pose_windows", vert, len(v), d["f"].data_ptr(), F, d["view"].data_ptr(), N, *VR.INTR, H, W, near, box, ptr["dropped"],
                  stream)

    def check(N=N, H=H, tau=TAU, ws_ptr=ws.data_ptr() + 8 * G, ws_bytes=need, vert=d["v"].data_ptr(), counts=ptr["counts"], box=ptr["box"],
              offset=d_offset.data_ptr(), obs=d["obs"].data_ptr(), wave_area=0, total=total):
        _lib.call("sam6d_pose_verify", vert, len(v), d["f"].data_ptr(), len(f), d["view"].data_ptr(), N, *VR.INTR, H, W, 1e-3, wave_area, box,
                  offset, total, obs, None, tau, counts, ptr["ids"], ptr["depth"], ws_ptr, ws_bytes, stream)

    windows()
    check()
    want = dict(box=wbox, dropped=wdropped, counts=wcounts, ids=wids, depth=wdepth)
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all(), k
        assert np.array_equal(h[G:-G], np.asarray(want[k]).reshape(-1)), k
    hw = ws.cpu().numpy()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()
    before = {k: b.clone() for k, b in bufs.items()}
    ws_before = ws.clone()
    for kw, name in ((dict(vert=None), "null"), (dict(box=None), "null"), (dict(H=2049), "H x W"), (dict(N=0), "N = 0"), (dict(N=1025), "N = 1025"),
                     (dict(near=0.0), "near"), (dict(F=0), "F = 0")):
        with pytest.raises(RuntimeError, match=name):
            windows(**kw)
    for kw, name in ((dict(vert=None), "null"), (dict(counts=None), "null"), (dict(box=None), "null"), (dict(offset=None), "null"),
                     (dict(obs=None), "null"), (dict(ws_ptr=None), "null"), (dict(H=2049), "H x W"), (dict(N=0), "N = 0"),
                     (dict(N=1025), "N = 1025"), (dict(tau=-1.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=float("inf")), "tau"),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(ws_ptr=ws.data_ptr() + 8 * G + 4), "aligned"), (dict(wave_area=-1), "wave_area"),
                     (dict(total=-1), "total"), (dict(total=N * H * W + 1), "total")):
        with pytest.raises(RuntimeError, match=name):
            check(**kw)
    canvas = torch.full((16 * 48 * 3 + 2 * G,), 77, dtype=torch.uint8, device=dev)
    rgb, ids, cols = torch.zeros((16, 24, 3), dtype=torch.uint8, device=dev), torch.zeros((16, 24), dtype=torch.int32, device=dev), torch.zeros((2, 3), dtype=torch.uint8, device=dev)

    def paint(H=16, N=2, alpha=128, stride=72, rgb_ptr=rgb.data_ptr()):
        _lib.call("sam6d_overlay_instances", rgb_ptr, stride, H, 24, ids.data_ptr(), cols.data_ptr(), N, alpha, canvas.data_ptr() + G, stream)

    for kw, name in ((dict(H=0), "H x W"), (dict(N=0), "N = 0"), (dict(N=1025), "N = 1025"), (dict(alpha=257), "alpha"), (dict(alpha=-1), "alpha"),
                     (dict(stride=71), "row_stride"), (dict(rgb_ptr=None), "null")):
        with pytest.raises(RuntimeError, match=name):
            paint(**kw)
    assert (canvas == 77).all()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and torch.equal(ws, ws_before)  # a refused call writes nothing
    # boxes and offsets the host never sees: nothing outside the buffers is touched, whatever they hold
    wild = _t(np.array([[-5, -7, 5000, 4000], [60, 40, 70, 50], [10, 10, 5, 5], [0, 0, -1, -1], [0, 0, 63, 47]], np.int32), dev)
    check(box=wild.data_ptr())
    check(offset=_t(np.array([0, total, -40, 1 << 40, 7, total], np.int64), dev).data_ptr())
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all(), k
    hw = ws.cpu().numpy()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()


# ------------------------------------------------------------------------------------------------------------ the picture
@pytest.mark.parametrize("alpha", [0, 128, 256])
def test_overlay_instances(dev, alpha):
    """ids holding -1, N - 1 and values out of range; instances meeting along a line and at the image border (the border itself is
    no edge); rgb a crop view with row_stride > 3 W"""
    g = np.random.default_rng(8)
    H, W, N = 16, 24, 4
    wide = g.integers(0, 256, (H, W + 9, 3), dtype=np.uint8)
    ids = np.full((H, W), -1, np.int32)
    ids[:9, :10] = 0          # against the top and left borders
    ids[:9, 10:17] = N - 1    # meets instance 0 along a vertical line
    ids[9:, 4:12] = 2         # meets both along a horizontal line, runs to the bottom border
    ids[3, 20], ids[4, 20], ids[5, 21] = N, -7, 1 << 30  # out of range: background
    ids[12, 20] = 1           # a single pixel: all edge
    colors = g.integers(0, 256, (N, 3), dtype=np.uint8)
    d_wide = _t(wide, dev)
    rgb = d_wide[:, 5:5 + W]
    assert rgb.stride(0) == 3 * (W + 9) > 3 * W
    got = V.overlay_instances(rgb, _t(ids, dev), colors, alpha=alpha)
    want = VR.overlay_instances(wide[:, 5:5 + W], ids, colors, alpha)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, 2 * W, 3) and torch.equal(got, _t(want, dev))
    right = want[:, W:]
    assert np.array_equal(right[0, 0], ((wide[0, 5].astype(int) * (256 - alpha) + colors[0].astype(int) * alpha + 128) >> 8))  # a corner: no edge
    assert np.array_equal(right[4, 9], colors[0]) and np.array_equal(right[4, 10], colors[N - 1]) and np.array_equal(right[12, 20], colors[1])
    assert np.array_equal(right[3, 20], wide[3, 25]) and np.array_equal(right[5, 21], wide[5, 26])


# ------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _end_to_end_scene():
    """icosphere(3), squeezed into an ellipsoid, at 96 x 128: pose A, A moved by 3 tau towards the camera and away from it, A turned by 20 degrees"""
    v, f = _mesh("icosphere3")
    v = (v * np.array([1.0, 0.8, 0.6], F32)).astype(F32)  # an ellipsoid: turning it changes what the camera sees
    R = VR.rotation((1.0, 2.0, 3.0), 0.7)
    t = np.array([0.1, -0.05, 3.0])
    turned = VR.rotation((0.0, 1.0, 0.0), np.deg2rad(20.0)) @ R
    Rs = np.stack([R, R, R, turned]).astype(F32)
    ts = np.stack([t, t - [0, 0, 3 * TAU], t + [0, 0, 3 * TAU], t]).astype(F32)
    return v, f, Rs, ts


def test_end_to_end(dev, tmp_path):
    from PIL import Image
    v, f, Rs, ts = _end_to_end_scene()
    view = np.concatenate([Rs, ts[:, :, None]], axis=2)
    dv, df = _t(v, dev), _t(f, dev)
    ref = onboard.render_views(dv, df, None, None, _t(view[:1], dev), _t(np.zeros((1, 3), F32), dev), BIG_INTR, BIG)
    obs = ref["depth"][0]
    K = np.array([[BIG_INTR[0], 0, BIG_INTR[2]], [0, BIG_INTR[1], BIG_INTR[3]], [0, 0, 1]])
    got = verify.render_compare(dict(vertices=v, faces=f), _t(Rs, dev), _t(ts, dev), K, obs, tol=TAU)
    obs_h = obs.cpu().numpy()
    want = _want(v, f, view, obs_h, intr=BIG_INTR)
    _same(dev, got, want)
    counts = want[1]
    covered = obs_h > 0
    assert counts[0, 0] == covered.sum() == counts[0, 1] > 2000 and float(got.inlier_ratio[0]) == 1.0
    assert int(got.inlier_ratio.argmax()) == 0 and float(got.inlier_ratio[3]) < 1.0
    # the moved poses: no inlier on the pixels A also covers -- and A covers every pixel with an observed depth, so none at all
    # (nearer than the truth: the camera sees through it, behind; farther: the observed surface stands in front, occluded)
    assert counts[1, 1] == 0 and counts[2, 1] == 0 and counts[1, 3] > 2000 and counts[2, 2] > 2000
    assert counts[1, 3] + counts[1, 4] == counts[1, 0] and counts[2, 2] + counts[2, 4] == counts[2, 0]
    g = np.random.default_rng(1)
    rgb = g.integers(0, 256, BIG + (3,), dtype=np.uint8)
    path = str(tmp_path / "vis_pem_render.png")
    img = V.vis_pem_render(rgb, got.ids, alpha=0.5, save_path=path)
    assert img.size == (2 * BIG[1], BIG[0])
    back = np.asarray(Image.open(path))
    n = int(want[2].max()) + 1
    assert np.array_equal(back, VR.overlay_instances(rgb, want[2], V.palette(n), 128)) and np.array_equal(back[:, :BIG[1]], rgb)
