"""The textured resolve on the device (sam6d_hip.onboard.render_views with face_uv and texture, csrc/texture.hip) against the numpy
restatement of its recipe (tests/texture_ref.py): mask, face, depth, xyz, rgb and n_dropped bit for bit at the smallest shapes at which
the stage can go wrong, the untextured route unchanged, guard bytes, and the chain OBJ + MTL + PNG -> load_mesh -> render_templates ->
save_templates."""
import os

import numpy as np
import pytest
import torch

from tests import raster_ref as RR
from tests import texture_ref as TR
from tests._util import ROOT
from sam6d_hip import _lib, onboard

pytestmark = pytest.mark.gpu

POSES = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
LUT = onboard.srgb_table()
KEYS = ("mask", "face", "depth", "xyz", "rgb", "n_dropped")
PIXEL = (1.0, 1.0, 0.0, 0.0)  # intrinsics under which a vertex (x z, y z, z) lands at pixel coordinates (x, y)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)[None]
LIGHT0 = np.array([[2.0, -3.0, -4.0]], np.float32)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _image(shape, seed=0):
    """random bytes with 0 and 255 present"""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    img.reshape(-1)[:3] = (0, 255, 0)
    img.reshape(-1)[-3:] = (255, 0, 255)
    return img


def _render(dev, v, f, face_uv, texture, view, light, intr, size, normals=None, colors=None, decode_srgb=False, **kw):
    return onboard.render_views(_t(np.asarray(v, np.float32), dev), _t(np.asarray(f, np.int32), dev), _t(normals, dev), _t(colors, dev),
                                _t(view, dev), _t(light, dev), intr, size, face_uv=_t(face_uv, dev), texture=_t(texture, dev),
                                decode_srgb=decode_srgb, **kw)


def _check(dev, v, f, face_uv, texture, view, light, intr, size, normals=None, decode_srgb=False):
    """device == restatement on all six outputs, bit for bit; -> (device output as numpy, restatement)"""
    got = _render(dev, v, f, face_uv, texture, view, light, intr, size, normals=normals, decode_srgb=decode_srgb)
    want = TR.render(np.asarray(v, np.float32), np.asarray(f, np.int32), normals, face_uv, texture, onboard.texel_table(decode_srgb), view, light,
                     intr, size, 1e-3, LUT)
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


def _ico_scene(level, size, poses, radius=50.0):
    v, f = RR.icosphere(level, radius)
    view, light = onboard.view_matrices(POSES[list(poses)], 0.5 / radius)
    H, W = size
    return v, f, view, light, (0.5 * W / np.tan(0.5 * 0.691111), 0.5 * W / np.tan(0.5 * 0.691111), 0.5 * W, 0.5 * H)


# ------------------------------------------------------------------------------------------------------------ single faces, 16 x 16
QUAD = [(1.3, 1.2), (14.6, 2.1), (2.2, 14.4), (13.7, 13.9)]


def test_a_seam(dev):
    """two triangles sharing an edge whose coordinates run 0.9 -> 1.1 on one and -0.2 -> 0.1 on the other, with a corner at u exactly
    1.0 and one at exactly -1.0: both sides of the wrap, and the wrap point itself, inside one picture"""
    f = [[0, 1, 2], [1, 3, 2]]
    face_uv = np.array([[[0.9, 0.9], [1.1, 1.0], [1.0, 1.1]], [[-0.2, 0.1], [0.1, -0.2], [-1.0, 0.0]]], np.float32)
    got, want = _check(dev, _px(QUAD, [1.0, 1.5, 2.0, 1.2]), f, face_uv, _image((3, 5), 1), EYE, LIGHT0, PIXEL, (16, 16))
    assert {0, 1} <= set(np.unique(got["face"]).tolist()) and (got["mask"] == 255).sum() > 120
    u = want["uv"][0][..., 0][got["mask"][0] == 255]
    assert (u > 1.0).any() and (u < 1.0).any() and (u < 0.0).any()


def test_tiling_and_bad_coordinates(dev):
    """coordinates of 3.25 / -2.5 tile the texture; a face with a NaN and an infinite coordinate renders the texel coordinate (0, 0)
    all over -- exactly what the same face renders with all its coordinates 0 -- and disturbs nothing else"""
    v = np.concatenate([_px(QUAD, [1.0, 1.5, 2.0, 1.2]), _px([(3.5, 4.5), (12.5, 5.0), (8.0, 11.5)], 0.8)])
    f = [[0, 1, 2], [1, 3, 2], [4, 5, 6]]
    face_uv = np.array([[[3.25, -2.5], [-2.5, 3.25], [0.5, 0.25]], [[-2.5, 3.25], [3.25, 3.25], [0.5, 0.25]],
                        [[np.nan, 0.3], [0.2, np.inf], [0.7, 0.6]]], np.float32)
    tex = _image((5, 3), 2)
    got, want = _check(dev, v, f, face_uv, tex, EYE, LIGHT0, PIXEL, (16, 16))
    assert (got["face"] == 2).sum() > 20 and (got["face"] == 0).sum() > 20 and (got["face"] == 1).sum() > 20
    zero = face_uv.copy()
    zero[2] = 0.0
    same = _render(dev, v, f, zero, tex, EYE, LIGHT0, PIXEL, (16, 16))
    for k in KEYS:
        assert np.array_equal(same[k].cpu().numpy(), got[k]), k
    on_bad = want["albedo"][0][got["face"][0] == 2]
    assert (on_bad == TR.lookup(np.zeros(1, np.float32), np.zeros(1, np.float32), tex, onboard.texel_table())).all()


def test_winding_swap_keeps_the_stored_order(dev):
    """a face with area2 < 0 (the setup exchanges its vertices 1 and 2, so the resolve has to exchange the weights back) with three
    distinct coordinates at its corners, and beside it its mirror image with the other winding"""
    tri = [(1.2, 1.4), (7.3, 2.2), (3.1, 13.6)]
    mirror = [(16 - x, y) for x, y in tri]
    v = _px(tri + mirror, [1.0, 2.0, 1.5] * 2)
    f = np.array([[0, 2, 1], [3, 5, 4]], np.int32)
    face_uv = np.array([[[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]]] * 2, np.float32)
    s = RR.Setup(v, f, EYE[0], *PIXEL, 1e-3, 16, 16)
    assert sorted(s.swapped.tolist()) == [False, True] and s.live.all()
    got, want = _check(dev, v, f, face_uv, _image((4, 4), 3), EYE, LIGHT0, PIXEL, (16, 16))
    assert (got["face"] == 0).sum() > 20 and (got["face"] == 1).sum() > 20
    # the mirror image is the mirrored picture of coordinates (to rounding: the snapped vertices mirror exactly about x = 8)
    uv = want["uv"][0]
    both = (got["face"][0] == 0) & (got["face"][0][:, ::-1] == 1)
    assert both.sum() > 20 and np.abs(uv[both] - uv[:, ::-1][both]).max() < 1e-5


def test_perspective(dev):
    """a quad from z = 1 to z = 6 under an 8 x 8 checkerboard at 37 x 53: half way down the quad on the screen v is far from one half
    (0.5 in an affine interpolation), and the board's rows crowd towards the far edge"""
    H, W = 37, 53
    v = _px([(4.5, 2.5), (48.5, 2.5), (48.5, 34.5), (4.5, 34.5)], [6.0, 6.0, 1.0, 1.0])
    f = [[0, 1, 2], [0, 2, 3]]
    corner_uv = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)
    ii, jj = np.mgrid[0:8, 0:8]
    board = np.repeat((((ii + jj) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    got, want = _check(dev, v, f, corner_uv[np.asarray(f)], board, EYE, LIGHT0, PIXEL, (H, W))
    assert (got["mask"] == 255).sum() == 44 * 32
    # the centre of the quad on the screen lies on the diagonal from corner 0 (z = 6) to corner 2 (z = 1): the weights go with 1 / z,
    # so corner 2 has 6 / 7 of it and (u, v) = (6 / 7, 1 / 7), where an affine interpolation says (1 / 2, 1 / 2)
    mid = want["uv"][0][18, 26]
    assert abs(mid[0] - 6 / 7) < 0.02 and abs(mid[1] - 1 / 7) < 0.02


# ------------------------------------------------------------------------------------------------------------ shapes and options
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 3), (64, 64)])
def test_texture_shapes(dev, shape):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 41))
    g = np.random.default_rng(shape[0] * 100 + shape[1])
    face_uv = (g.random((len(f), 3, 2)) * 3 - 1).astype(np.float32)
    got, want = _check(dev, v, f, face_uv, _image(shape, 5), view, light, intr, (17, 33))
    assert (got["mask"] == 255).sum() > 80
    if shape != (1, 1):
        assert len(np.unique(want["albedo"][got["mask"] == 255])) > 20
    four = np.concatenate([_image(shape, 5), np.full(shape + (1,), 99, np.uint8)], axis=2)  # a fourth byte is ignored
    again = _render(dev, v, f, face_uv, four, view, light, intr, (17, 33))
    for k in KEYS:
        assert np.array_equal(again[k].cpu().numpy(), got[k]), k


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("decode_srgb", [False, True])
def test_views_and_attributes(dev, T, with_normals, decode_srgb):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 17, 41)[:T])
    g = np.random.default_rng(11)
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    face_uv = (g.random((len(f), 3, 2)) * 2 - 0.5).astype(np.float32)
    tex = _image((6, 9), 6)
    got, _ = _check(dev, v, f, face_uv, tex, view, light, intr, (17, 33), normals=normals, decode_srgb=decode_srgb)
    lit = got["rgb"][got["mask"] == 255]
    assert (got["mask"] == 255).sum() > 40 * T and lit.max() > 0 and not ((lit[:, 0] == lit[:, 1]) & (lit[:, 1] == lit[:, 2])).all()
    if T == 3 and not decode_srgb:
        # colorize wins over the texture: the untextured grey render, whatever colours the mesh has
        colors = g.integers(0, 256, (len(v), 3), dtype=np.uint8)
        grey = _render(dev, v, f, face_uv, tex, view, light, intr, (17, 33), normals=normals, colors=colors, colorize=True, base_color=0.3)
        want = RR.render(v, f, normals, None, view, light, intr, (17, 33), 1e-3, 0.3, False, LUT)
        for k in KEYS:
            assert np.array_equal(grey[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("b", [0, 77, 255])
def test_one_texel_equals_the_grey_render(dev, b, with_normals):
    """device against device: a 1 x 1 texture of bytes (b, b, b) filters to a + fx * (a - a) = a = texel_table()[b] exactly, so the
    textured resolve writes what the grey resolve (colorize) writes with that base_color, on all six outputs, bit for bit -- the two
    kernels share raster.h's resolve core and tone step"""
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 41))
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    face_uv = (np.random.default_rng(b).random((len(f), 3, 2)) * 3 - 1).astype(np.float32)
    got = _render(dev, v, f, face_uv, np.full((1, 1, 3), b, np.uint8), view, light, intr, (17, 33), normals=normals)
    grey = _render(dev, v, f, None, None, view, light, intr, (17, 33), normals=normals, colorize=True, base_color=float(onboard.texel_table()[b]))
    assert int((got["mask"] == 255).sum()) > 80
    for k in KEYS:
        assert got[k].dtype == grey[k].dtype and torch.equal(got[k], grey[k]), (k, int((got[k] != grey[k]).sum()))


def test_untextured_route_is_unchanged(dev):
    """render_views without the new keywords == sam6d_render_views called directly on the same inputs, byte for byte"""
    v, f, view, light, intr = _ico_scene(2, (64, 64), (6, 10, 36))
    g = np.random.default_rng(12)
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    colors = g.integers(0, 256, (len(v), 3), dtype=np.uint8)
    T, H, W = 3, 64, 64
    d = dict(v=_t(v, dev), f=_t(f, dev), n=_t(normals, dev), c=_t(colors, dev), view=_t(view, dev), light=_t(light, dev), lut=_t(LUT, dev))
    got = onboard.render_views(d["v"], d["f"], d["n"], d["c"], d["view"], d["light"], intr, (H, W), base_color=0.2)
    out = dict(mask=torch.empty((T, H, W), dtype=torch.uint8, device=dev), face=torch.empty((T, H, W), dtype=torch.int32, device=dev),
               depth=torch.empty((T, H, W), dtype=torch.float32, device=dev), xyz=torch.empty((T, H, W, 3), dtype=torch.float32, device=dev),
               rgb=torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev), n_dropped=torch.empty((T,), dtype=torch.int32, device=dev))
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=dev)
    _lib.call("sam6d_render_views", d["v"].data_ptr(), len(v), d["f"].data_ptr(), len(f), d["n"].data_ptr(), d["c"].data_ptr(), d["view"].data_ptr(),
              d["light"].data_ptr(), T, *[float(x) for x in intr], H, W, onboard.NEAR, 0.2, 0, d["lut"].data_ptr(), 0, out["mask"].data_ptr(),
              out["face"].data_ptr(), out["depth"].data_ptr(), out["xyz"].data_ptr(), out["rgb"].data_ptr(), out["n_dropped"].data_ptr(),
              ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    for k in KEYS:
        assert got[k].dtype == out[k].dtype and torch.equal(got[k], out[k]), k
    want = RR.render(v, f, normals, colors, view, light, intr, (H, W), onboard.NEAR, 0.2, False, LUT)
    assert np.array_equal(got["rgb"].cpu().numpy(), want["rgb"])


def test_python_refusals(dev):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0,))
    face_uv, tex = np.zeros((len(f), 3, 2), np.float32), _image((4, 4))
    args = (_t(v, dev), _t(f, dev), None, None, _t(view, dev), _t(light, dev), intr, (17, 33))
    for kw, name in ((dict(face_uv=_t(face_uv[:-1], dev)), "face_uv must be"), (dict(face_uv=_t(face_uv.astype(np.float64), dev)), "face_uv must be"),
                     (dict(face_uv=_t(face_uv, dev).cpu()), "face_uv must be a tensor on"), (dict(texture=_t(tex, dev).cpu()), "texture must be a tensor on"),
                     (dict(texture=_t(tex[:, :, :2], dev)), "texture must be"), (dict(texture=_t(tex.astype(np.int32), dev)), "texture must be"),
                     (dict(texture=_t(tex[:, :, 0], dev)), "texture must be"), (dict(texture=None), "go together")):
        full = dict(face_uv=_t(face_uv, dev), texture=_t(tex, dev))
        full.update(kw)
        with pytest.raises(ValueError, match=name):
            onboard.render_views(*args, **full)


def test_guard_values_and_refusals(dev):
    v, f, view, light, intr = _ico_scene(1, (17, 33), (0, 41))
    T, H, W, G = 2, 17, 33, 256
    g = np.random.default_rng(13)
    face_uv = (g.random((len(f), 3, 2)) * 3 - 1).astype(np.float32)
    tex = _image((5, 3), 7)
    tex4 = np.concatenate([tex, np.zeros((5, 3, 1), np.uint8)], axis=2)
    d = dict(v=_t(v, dev), f=_t(f, dev), view=_t(view, dev), light=_t(light, dev), lut=_t(LUT, dev), uv=_t(face_uv, dev), tex=_t(tex4, dev),
             texel=_t(onboard.texel_table(), dev))
    want = TR.render(v, f, None, face_uv, tex, onboard.texel_table(), view, light, intr, (H, W), 1e-3, LUT)
    sizes = dict(mask=(T * H * W, torch.uint8), face=(T * H * W, torch.int32), depth=(T * H * W, torch.float32), xyz=(T * H * W * 3, torch.float32),
                 rgb=(T * H * W * 3, torch.uint8), n_dropped=(T, torch.int32))
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(T=T, H=H, W=W, F=len(f), near=1e-3, ws_bytes=need, vert=d["v"].data_ptr(), wave_area=0, Ht=5, Wt=3, tex=d["tex"].data_ptr(),
             uv=d["uv"].data_ptr(), texel=d["texel"].data_ptr()):
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        _lib.call("sam6d_render_views_textured", vert, len(v), d["f"].data_ptr(), F, None, d["view"].data_ptr(), d["light"].data_ptr(), T,
                  *[float(x) for x in intr], H, W, near, 0.05, d["lut"].data_ptr(), wave_area, uv, tex, Ht, Wt, texel, ptr["mask"], ptr["face"],
                  ptr["depth"], ptr["xyz"], ptr["rgb"], ptr["n_dropped"], ws.data_ptr() + 8 * G, ws_bytes, stream)

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
                     (dict(wave_area=-5), "wave_area"), (dict(Ht=0), "Ht x Wt"), (dict(Wt=8193), "Ht x Wt"), (dict(tex=None), "null"),
                     (dict(uv=None), "null"), (dict(texel=None), "null"), (dict(tex=d["tex"].data_ptr() + 2), "4-byte aligned")):
        with pytest.raises(RuntimeError, match=name):
            call(**kw)
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and torch.equal(ws, ws_before)  # a refused call writes nothing


# ------------------------------------------------------------------------------------------------------------ the chain
def test_textured_onboarding_chain(dev, tmp_path):
    from PIL import Image
    v, f = RR.icosphere(2, 60.0)
    v = (v * np.array([1.0, 0.8, 0.6], np.float32)).astype(np.float32)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    vt = np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 2], -1, 1)) / np.pi], axis=1)
    img = _image((16, 32), 8)
    Image.fromarray(img, "RGB").save(str(tmp_path / "skin.png"))
    with open(str(tmp_path / "ball.mtl"), "w") as fh:
        fh.write("newmtl skin\nKd 1 1 1\nmap_Kd skin.png\n")
    with open(str(tmp_path / "ball.obj"), "w") as fh:
        fh.write("mtllib ball.mtl\nusemtl skin\n")
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in v))
        fh.write("".join("vt %r %r\n" % tuple(float(x) for x in p) for p in vt))
        fh.write("".join("f %d/%d %d/%d %d/%d\n" % tuple(int(i) + 1 for i in np.repeat(tri, 2)) for tri in f))
    mesh = onboard.load_mesh(str(tmp_path / "ball.obj"))
    assert np.array_equal(mesh["vertices"], v) and np.array_equal(mesh["faces"], f) and np.array_equal(mesh["texture"], img)
    assert np.array_equal(mesh["face_uv"], vt.astype(np.float32)[f]) and mesh["normals"] is None and mesh["colors"] is None
    poses = POSES[[6, 10, 36]]
    out = onboard.render_templates(mesh, poses, size=64)
    assert out["rgb"].shape == (3, 64, 64, 3) and (out["n_dropped"] == 0).all()
    view, light = onboard.view_matrices(poses, out["scale"])
    want = TR.render(v, f, None, mesh["face_uv"], img, onboard.texel_table(), view, light, onboard.intrinsics_from_fov(64, 0.691111), (64, 64),
                     onboard.NEAR, LUT)
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    plain = onboard.render_templates(dict(mesh, texture=None), poses, size=64)  # the same mesh without its image: today's grey render
    mask = out["mask"].cpu().numpy() == 255
    assert torch.equal(plain["mask"], out["mask"]) and torch.equal(plain["xyz"], out["xyz"]) and mask.sum() > 3 * 400
    differ = (plain["rgb"].cpu().numpy() != out["rgb"].cpu().numpy()).any(axis=-1)
    assert differ[mask].mean() > 0.9 and not differ[~mask].any()
    grey = onboard.render_templates(mesh, poses, size=64, colorize=True)  # colorize > texture
    assert torch.equal(grey["rgb"], plain["rgb"])
    d = onboard.save_templates(out, str(tmp_path / "obj" / "templates"))
    assert len(os.listdir(d)) == 3 * 3
    rgb = np.stack([np.asarray(Image.open(os.path.join(d, "rgb_%d.png" % i))) for i in range(3)])
    msk = np.stack([np.asarray(Image.open(os.path.join(d, "mask_%d.png" % i))) for i in range(3)])
    assert np.array_equal(rgb, out["rgb"].cpu().numpy()) and np.array_equal(msk, out["mask"].cpu().numpy())
