"""Onboarding a CAD model on the device (sam6d_hip.onboard over csrc/raster.hip and csrc/meshsample.hip) against the numpy
restatements of their recipes (tests/raster_ref.py, tests/meshsample_ref.py): mask, face, depth, xyz, rgb, n_dropped and the sampled
points bit for bit, then the chain render_templates -> save_templates -> inputs.templates and model_points -> inputs.test_data."""
import os

import numpy as np
import pytest
import torch

from tests import meshsample_ref as MS
from tests import raster_ref as RR
from tests._util import ROOT
from sam6d_hip import _lib, inputs, onboard

pytestmark = pytest.mark.gpu

POSES = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
LUT = onboard.srgb_table()
KEYS = ("mask", "face", "depth", "xyz", "rgb", "n_dropped")
PIXEL = (1.0, 1.0, 0.0, 0.0)  # intrinsics under which a vertex (x z, y z, z) lands at pixel coordinates (x, y)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)[None]
LIGHT0 = np.array([[2.0, -3.0, -4.0]], np.float32)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _render(dev, v, f, view, light, intr, size, normals=None, colors=None, near=1e-3, base_color=0.05, colorize=False, wave_area=0):
    return onboard.render_views(_t(np.asarray(v, np.float32), dev), _t(np.asarray(f, np.int32), dev), _t(normals, dev), _t(colors, dev),
                                _t(view, dev), _t(light, dev), intr, size, near=near, base_color=base_color, colorize=colorize,
                                wave_area=wave_area)


def _check(dev, v, f, view, light, intr, size, **kw):
    """device == restatement on every output, bit for bit; -> (device output as numpy, restatement)"""
    got = _render(dev, v, f, view, light, intr, size, **kw)
    ref_kw = {k: kw[k] for k in ("normals", "colors") if k in kw}
    want = RR.render(np.asarray(v, np.float32), np.asarray(f, np.int32), ref_kw.get("normals"), ref_kw.get("colors"), view, light, intr, size,
                     kw.get("near", 1e-3), kw.get("base_color", 0.05), kw.get("colorize", False), LUT)
    for k in KEYS:
        w = torch.from_numpy(np.ascontiguousarray(want[k])).to(dev)
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert torch.equal(got[k], w), (k, int((got[k] != w).sum()))
    return {k: got[k].cpu().numpy() for k in KEYS}, want


def _px(points, z=1.0):
    """camera-space vertices that land on the pixel coordinates `points` at depth z (a scalar or one per point)"""
    p = np.asarray(points, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(p),))
    return np.stack([p[:, 0] * z, p[:, 1] * z, z], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ single triangles, 8 x 8
A, B, C, D = (0.5, 0.5), (6.5, 0.5), (0.5, 6.5), (6.5, 6.5)


def test_edges_through_centres_and_a_shared_edge(dev):
    """A B C has its top and left edges and its hypotenuse through pixel centres and all vertices on centres: the top-left rule keeps
    the centres of the top and left edges and gives up those of the hypotenuse; with B D C beside it every centre of the half-open
    square [0.5, 6.5)^2 is taken exactly once, the shared edge's by face 1 (its edge C -> B runs upwards: a left edge)."""
    ii, jj = np.mgrid[0:8, 0:8]
    got, _ = _check(dev, _px([A, B, C]), [[0, 1, 2]], EYE, LIGHT0, PIXEL, (8, 8))
    assert np.array_equal(got["mask"][0] == 255, ii + jj < 6)
    got, _ = _check(dev, _px([A, B, C, D]), [[0, 1, 2], [1, 3, 2]], EYE, LIGHT0, PIXEL, (8, 8))
    assert np.array_equal(got["mask"][0] == 255, (ii < 6) & (jj < 6))
    assert np.array_equal(got["face"][0], np.where((ii < 6) & (jj < 6), np.where(ii + jj < 6, 0, 1), -1))
    assert (got["depth"][0][got["mask"][0] == 255] == 1.0).all()
    # the other winding of both faces draws the same pixels
    flipped, _ = _check(dev, _px([A, B, C, D]), [[0, 2, 1], [1, 2, 3]], EYE, LIGHT0, PIXEL, (8, 8))
    assert np.array_equal(flipped["face"], got["face"]) and np.array_equal(flipped["depth"], got["depth"])
    assert np.abs(flipped["xyz"] - got["xyz"]).max() <= 8 * 2.0 ** -24 * 6.5  # the attributes are mixed in the stored order


def test_coincident_and_interpenetrating_triangles(dev):
    tri = _px([(0.2, 0.3), (7.6, 1.1), (2.3, 7.7)], 2.0)
    got, _ = _check(dev, tri, [[0, 1, 2], [0, 1, 2], [1, 2, 0]], EYE, LIGHT0, PIXEL, (8, 8))
    assert set(np.unique(got["face"]).tolist()) == {-1, 0}  # a depth tie: the lower face id wins
    got, _ = _check(dev, tri, [[1, 2, 0], [0, 1, 2]], EYE, LIGHT0, PIXEL, (8, 8))
    assert (got["mask"] == 255).sum() > 15
    # two triangles through each other: depth 1 .. 3 across one, 3 .. 1 across the other
    v = np.concatenate([_px([(0.2, 0.2), (7.8, 0.4), (3.9, 7.8)], [1.0, 3.0, 2.0]), _px([(0.3, 0.1), (7.7, 0.3), (4.1, 7.7)], [3.0, 1.0, 2.0])])
    got, _ = _check(dev, v, [[0, 1, 2], [3, 4, 5]], EYE, LIGHT0, PIXEL, (8, 8))
    assert {0, 1} <= set(np.unique(got["face"]).tolist())


def test_slivers_zero_area_and_the_image_border(dev):
    got, _ = _check(dev, _px([(0.6, 0.6), (7.4, 0.6), (7.4, 0.9)]), [[0, 1, 2]], EYE, LIGHT0, PIXEL, (8, 8))
    assert (got["mask"] == 0).all() and (got["face"] == -1).all() and got["n_dropped"][0] == 0  # between the rows of centres
    v = _px([(1.5, 1.5), (4.5, 4.5), (6.5, 6.5), (3.0, 3.0)])
    got, _ = _check(dev, v, [[0, 1, 2], [3, 3, 3], [0, 0, 1]], EYE, LIGHT0, PIXEL, (8, 8))
    assert (got["mask"] == 0).all() and got["n_dropped"][0] == 0  # zero area: covers nothing, and is not "dropped"
    v = _px([(-5.0, -5.0), (4.2, 2.1), (2.2, 6.3), (20, 20), (30, 20), (20, 30), (-9, 2), (-3, 1), (-4, 7), (-30000.0, 3.0), (90000.0, 2.0), (5.0, 70000.0)])
    got, _ = _check(dev, v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], EYE, LIGHT0, PIXEL, (8, 8))
    assert 0 < (got["mask"] == 255).sum() < 64 and set(np.unique(got["face"]).tolist()) == {-1, 0}
    _check(dev, v, [[9, 10, 11], [0, 1, 2]], EYE, LIGHT0, PIXEL, (8, 8))  # coordinates past the snap limit are clamped, not wrapped


def test_near_plane_drops_whole_faces(dev):
    v = np.concatenate([_px([(1, 1), (7, 2), (3, 7)], -1.0), _px([(1, 1), (7, 2), (3, 7)], [2.0, 2.0, 0.25]), _px([(0.2, 0.2), (7.5, 0.5), (1.0, 7.5)], 3.0)])
    # (one face behind the camera, one with a vertex nearer than `near`, one in front)
    got, _ = _check(dev, v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], EYE, LIGHT0, PIXEL, (8, 8), near=0.5)
    assert got["n_dropped"].tolist() == [2]
    assert set(np.unique(got["face"]).tolist()) == {-1, 2}  # nothing is written for a dropped face
    with pytest.raises(ValueError, match="face indices"):
        _render(dev, v, [[6, 7, 9]], EYE, LIGHT0, PIXEL, (8, 8))
    with pytest.raises(ValueError, match="face indices"):
        _render(dev, v, [[6, -1, 8]], EYE, LIGHT0, PIXEL, (8, 8))


# ------------------------------------------------------------------------------------------------------------ sizes, paths, options
def _ico_scene(level, size, poses, radius=50.0):
    v, f = RR.icosphere(level, radius)
    view, light = onboard.view_matrices(POSES[list(poses)], 0.5 / radius)
    H, W = size
    return v, f, view, light, (0.5 * W / np.tan(0.5 * 0.691111), 0.5 * W / np.tan(0.5 * 0.691111), 0.5 * W, 0.5 * H)


def test_one_pixel(dev):
    got, _ = _check(dev, _px([(-3, -2), (5, -1), (0, 6)], 1.5), [[0, 1, 2]], EYE, LIGHT0, PIXEL, (1, 1))
    assert got["mask"].tolist() == [[[255]]]
    got, _ = _check(dev, _px([(0.6, 0.6), (5, 0.7), (0.7, 6)], 1.5), [[0, 1, 2]], EYE, LIGHT0, PIXEL, (1, 1))
    assert got["mask"].tolist() == [[[0]]]


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("attrs", ["plain", "normals", "colors", "both", "colorize"])
def test_odd_size_views_and_options(dev, T, attrs):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 17, 41)[:T])
    g = np.random.default_rng(4)
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if attrs in ("normals", "both", "colorize") else None
    colors = g.integers(0, 256, (len(v), 3), dtype=np.uint8) if attrs in ("colors", "both", "colorize") else None
    got, _ = _check(dev, v, f, view, light, intr, (17, 33), normals=normals, colors=colors, colorize=attrs == "colorize", base_color=0.3)
    lit = got["rgb"][got["mask"] == 255]
    assert (got["mask"] == 255).sum() > 40 * T and lit.max() > 0
    assert ((lit[:, 0] == lit[:, 1]) & (lit[:, 1] == lit[:, 2])).all() == (attrs in ("plain", "normals", "colorize"))


def _sphere_before_a_wall():
    """a 320-face icosphere (faces of a few pixels: the thread path) in front of one triangle that covers the whole image (the wave
    path), at 64 x 64 from fixture pose 17"""
    v, f, view, light, intr = _ico_scene(2, (64, 64), (17,))
    wall_cam = np.array([[-9.0, -6.0, 3.0], [9.0, -6.0, 3.0], [0.0, 12.0, 3.0]])  # camera space -> object space
    M = view[0].astype(np.float64)
    wall = (np.linalg.inv(M[:, :3]) @ (wall_cam - M[:, 3]).T).T.astype(np.float32)
    return np.concatenate([v, wall]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32), view, light, intr


def test_thread_and_wave_paths_agree(dev):
    v, f, view, light, intr = _sphere_before_a_wall()
    got, _ = _check(dev, v, f, view, light, intr, (64, 64))
    assert (got["mask"] == 255).all() and (got["face"] == 320).sum() > 2000 and (got["face"] < 320).sum() > 1000
    again = _render(dev, v, f, view, light, intr, (64, 64))
    waves = _render(dev, v, f, view, light, intr, (64, 64), wave_area=1)        # every face by a whole wave
    threads = _render(dev, v, f, view, light, intr, (64, 64), wave_area=1 << 30)  # every face by its own lane
    for k in KEYS:
        ref = torch.from_numpy(got[k]).to(dev)
        assert torch.equal(again[k], ref) and torch.equal(waves[k], ref) and torch.equal(threads[k], ref), k


def test_full_size_render(dev):
    v, f, view, light, intr = _ico_scene(3, (512, 512), (0, 17, 41))
    assert len(f) == 1280
    got, _ = _check(dev, v, f, view, light, intr, (512, 512))
    assert (got["n_dropped"] == 0).all() and all(95000 < (m == 255).sum() < 110000 for m in got["mask"])  # a disc of radius 183


def test_guard_values_and_refusals(dev):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 41))
    T, H, W, G = 2, 17, 33, 256
    d = dict(v=_t(v, dev), f=_t(f, dev), view=_t(view, dev), light=_t(light, dev), lut=_t(LUT, dev))
    want = RR.render(v, f, None, None, view, light, intr, (H, W), 1e-3, 0.05, False, LUT)
    sizes = dict(mask=(T * H * W, torch.uint8), face=(T * H * W, torch.int32), depth=(T * H * W, torch.float32), xyz=(T * H * W * 3, torch.float32),
                 rgb=(T * H * W * 3, torch.uint8), n_dropped=(T, torch.int32))
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(T=T, H=H, W=W, F=len(f), near=1e-3, ws_bytes=need, vert=d["v"].data_ptr(), wave_area=0):
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        _lib.call("sam6d_render_views", vert, len(v), d["f"].data_ptr(), F, None, None, d["view"].data_ptr(), d["light"].data_ptr(), T,
                  *[float(x) for x in intr], H, W, near, 0.05, 0, d["lut"].data_ptr(), wave_area, ptr["mask"], ptr["face"], ptr["depth"],
                  ptr["xyz"], ptr["rgb"], ptr["n_dropped"], ws.data_ptr() + 8 * G, ws_bytes, stream)

    call()
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all(), k
        assert np.array_equal(h[G:-G], np.asarray(want[k]).reshape(-1)), k
    hw = ws.cpu().numpy()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()
    before = {k: b.clone() for k, b in bufs.items()}
    ws_before = ws.clone()
    for kw, name in ((dict(H=0), "H x W"), (dict(W=2049), "H x W"), (dict(T=0), "T = 0"), (dict(T=1025), "T = 1025"), (dict(F=0), "F = 0"),
                     (dict(F=(1 << 24) + 1), "F = "), (dict(near=0.0), "near"), (dict(ws_bytes=need - 1), "workspace"), (dict(vert=None), "null"),
                     (dict(wave_area=-5), "wave_area")):
        with pytest.raises(RuntimeError, match=name):
            call(**kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        onboard.render_views(d["v"].cpu(), d["f"].cpu(), None, None, d["view"].cpu(), d["light"].cpu(), intr, (H, W))
    with pytest.raises(ValueError, match="2048"):
        onboard.render_views(d["v"], d["f"], None, None, d["view"], d["light"], intr, (H, 2049))
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and torch.equal(ws, ws_before)  # a refused call writes nothing
    # a face index outside the vertices, past the host's check: dropped whole and counted, nothing is read through it
    bad = f.copy()
    bad[3, 1], bad[5, 2] = len(v), -1
    d["f"] = _t(bad, dev)
    call()
    want = RR.render(v, bad, None, None, view, light, intr, (H, W), 1e-3, 0.05, False, LUT)
    assert want["n_dropped"].tolist() == [2, 2]
    for k, b in bufs.items():
        assert np.array_equal(b.cpu().numpy()[G:-G], np.asarray(want[k]).reshape(-1)), k


# ------------------------------------------------------------------------------------------------------------ sampler
def _soup(F, seed):
    """F triangles over F + 2 random vertices in millimetres; every 7th face repeats a vertex (zero area)"""
    g = np.random.default_rng(seed)
    v = ((g.random((F + 2, 3)) - 0.5) * 200.0).astype(np.float32)
    f = g.integers(0, F + 2, (F, 3)).astype(np.int32)
    if F > 7:
        f[::7, 2] = f[::7, 1]
    if F <= 2:
        f = np.array([[0, 1, 2], [1, 2, 3]][:F], np.int32)
    return v, f


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
@pytest.mark.parametrize("F, n", [(1, 1), (1, 2048), (2, 1024), (1025, 1), (1025, 2048), (70001, 1024), (70001, 100000)])
def test_samples_equal_the_restatement(dev, F, n, seed):
    v, f = _soup(F, F)
    pts, face = onboard.sample_surface(_t(v, dev), _t(f, dev), n, seed)
    wp, wf = MS.sample(v, f, n, seed)
    assert pts.dtype == torch.float32 and pts.shape == (n, 3) and face.dtype == torch.int32 and face.shape == (n,)
    assert torch.equal(face, _t(wf, dev)), int((face.cpu() != torch.from_numpy(wf)).sum())
    assert torch.equal(pts, _t(wp, dev))
    again = onboard.sample_surface(_t(v, dev), _t(f, dev), n, seed)
    assert torch.equal(again[0], pts) and torch.equal(again[1], face)
    if n > 300:  # rows of a longer draw
        tail = onboard.sample_surface(_t(v, dev), _t(f, dev), 100, seed, row=n - 100)
        assert torch.equal(tail[0], pts[n - 100:]) and torch.equal(tail[1], face[n - 100:])


def test_sampler_guards_and_refusals(dev):
    v, f = _soup(1025, 3)
    n, G = 500, 64
    dv, df = _t(v, dev), _t(f, dev)
    pts = torch.full((2 * G + n * 3,), 77.0, dtype=torch.float32, device=dev)
    face = torch.full((2 * G + n,), 77, dtype=torch.int32, device=dev)
    need = _lib.load().sam6d_mesh_sample_workspace_bytes(1025)
    ws = torch.full(((need + 7) // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=n, F=1025, ws_bytes=need, faces=df, vert=dv.data_ptr(), row=0xFFFFFF00):
        _lib.call("sam6d_mesh_sample", vert, len(v), faces.data_ptr(), F, n, 9, row, pts.data_ptr() + 4 * G, face.data_ptr() + 4 * G,
                  ws.data_ptr() + 8 * G, ws_bytes, stream)

    call()
    wp, wf = MS.sample(v, f, n, 9, row=0xFFFFFF00)  # the sample counter wraps modulo 2^32
    hp, hf, hw = pts.cpu().numpy(), face.cpu().numpy(), ws.cpu().numpy()
    assert (hp[:G] == 77).all() and (hp[-G:] == 77).all() and (hf[:G] == 77).all() and (hf[-G:] == 77).all()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()
    assert np.array_equal(hp[G:-G].reshape(n, 3), wp) and np.array_equal(hf[G:-G], wf)
    before = (pts.clone(), face.clone())
    flat = _t(np.array([[0, 1, 1], [2, 2, 2], [3, 3, 4]], np.int32), dev)
    for kw, name in ((dict(n=0), "n = 0"), (dict(n=(1 << 24) + 1), "n = "), (dict(F=0), "F = 0"), (dict(F=(1 << 24) + 1), "F = "),
                     (dict(ws_bytes=need - 1), "workspace"), (dict(vert=None), "null"), (dict(faces=flat, F=3), "zero area")):
        with pytest.raises(RuntimeError, match=name):
            call(**kw)
    assert torch.equal(pts, before[0]) and torch.equal(face, before[1])  # a refused call writes nothing to the outputs
    with pytest.raises(RuntimeError, match="zero area"):
        onboard.sample_surface(dv, flat, 10)
    with pytest.raises(ValueError, match="face indices"):
        onboard.sample_surface(dv, _t(np.array([[0, 1, 2000]], np.int32), dev), 10)


# ------------------------------------------------------------------------------------------------------------ the chain
def test_onboarding_chain(dev, tmp_path):
    from PIL import Image
    v, f = RR.icosphere(3, 60.0)
    v = (v * np.array([1.0, 0.8, 0.6], np.float32)).astype(np.float32)  # an ellipsoid in millimetres
    mesh = dict(vertices=v, faces=f, normals=None, colors=None)
    scale = onboard.norm_scale(_t(v, dev), _t(f, dev))
    pts, _ = MS.sample(v, f, 1024, 0)
    radius = max(np.linalg.norm(pts.max(axis=0)), np.linalg.norm(pts.min(axis=0)))
    assert abs(scale * radius - 0.5) < 1e-6  # the sampled cloud's corner radius goes to 0.5
    out = onboard.render_templates(mesh, POSES, size=128)
    assert out["scale"] == scale and out["rgb"].shape == (42, 128, 128, 3) and out["mask"].shape == (42, 128, 128)
    assert out["xyz"].shape == (42, 128, 128, 3) and out["xyz"].dtype == torch.float32 and (out["n_dropped"] == 0).all()
    mask = out["mask"].cpu().numpy()
    assert set(np.unique(mask).tolist()) == {0, 255} and all(1500 < (m == 255).sum() < 6000 for m in mask)
    xyz = out["xyz"].cpu().numpy()[mask == 255]  # CAD units: on the ellipsoid's faces, just inside its surface
    r = np.linalg.norm(xyz / np.array([60.0, 48.0, 36.0]), axis=1)
    assert 0.98 < r.min() and r.max() < 1.0 + 1e-5
    d = onboard.save_templates(out, str(tmp_path / "obj" / "templates"))
    assert len(os.listdir(d)) == 3 * 42
    rgb = np.stack([np.asarray(Image.open(os.path.join(d, "rgb_%d.png" % i))) for i in range(42)])
    msk = np.stack([np.asarray(Image.open(os.path.join(d, "mask_%d.png" % i))) for i in range(42)])
    xyz16 = np.stack([np.load(os.path.join(d, "xyz_%d.npy" % i)) for i in range(42)])
    assert np.array_equal(rgb, out["rgb"].cpu().numpy()) and np.array_equal(msk, mask) and xyz16.dtype == np.float16
    cfg = dict(img_size=224, n_sample_template_point=500, n_sample_observed_point=64, rgb_mask_flag=True)
    np.random.seed(0)
    tem, tem_pts, tem_choose = inputs.templates(out["rgb"], out["mask"], out["xyz"], cfg)
    assert len(tem) == len(tem_pts) == len(tem_choose) == 42
    assert tem[0].shape == (1, 3, 224, 224) and tem_pts[0].shape == (1, 500, 3) and tem_choose[0].shape == (1, 500)
    assert tem_choose[0].dtype == torch.int64 and float(tem_pts[0].abs().max()) <= 0.0601  # metres
    # the sampled model points go into test_data as they are
    model = onboard.model_points(mesh, 1024, seed=0)
    assert model.dtype == np.float32 and model.shape == (1024, 3) and np.array_equal(model, pts / np.float32(1000.0))
    H, W = 120, 160
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.random.default_rng(1)
    depth = np.full((H, W), 0.7, np.float32)
    masks = (((xx - 80) ** 2 + (yy - 60) ** 2) < 30 ** 2).astype(np.uint8)[None]
    K = np.array([[572.4114, 0.0, 80.0], [0.0, 573.57043, 60.0], [0.0, 0.0, 1.0]])
    data, kept = inputs.test_data(_t(g.integers(0, 256, (H, W, 3), dtype=np.uint8), dev), _t(depth, dev), K, _t(masks, dev), np.array([0.9]),
                                  model, cfg)
    assert kept == [0] and data["model"].shape == (1, 1024, 3) and torch.equal(data["model"][0], _t(model, dev))
