"""Textured CAD models (sam6d_hip.onboard's readers, csrc/texture.hip) without a GPU: OBJ + MTL + image and textured PLY files written
and read back, what the readers refuse, the numpy restatement of the TEXTURE recipe (tests/texture_ref.py) anchored to the untextured
restatement, to a float64 lookup and to the image's orientation, what the C entry refuses before a launch, and the kernel's registers."""
import os
import re

import numpy as np
import pytest
import torch

from tests import raster_ref as RR
from tests import texture_ref as TR
from tests._util import ROOT

POSES = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
NEAR = 1.0e-3
PIXEL = (1.0, 1.0, 0.0, 0.0)  # intrinsics under which a vertex (x z, y z, z) lands at pixel coordinates (x, y)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)[None]
LIGHT0 = np.array([[2.0, -3.0, -4.0]], np.float32)

# five vertices, a quad and two triangles: the mesh of tests/test_onboard_host.py::test_load_ply
VERT = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.25], [0.5, 0.5, 2]], np.float32)
NORM = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0.6, 0.8, 0]], np.float32)
POLY = [[0, 1, 2, 3], [0, 1, 4], [3, 2, 4]]
TRIS = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [3, 2, 4]], np.int32)
VT = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.5], [0.25, 0.75], [1.5, -0.25]], np.float32)
POLY_VT = [[0, 1, 2, 3], [5, 6, 4], [3, 2, 6]]  # texture coordinates of their own per corner: a seam at every face
TRIS_VT = np.array([[0, 1, 2], [0, 2, 3], [5, 6, 4], [3, 2, 6]])


def _image(shape, seed=0):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    img.reshape(-1)[:2] = (0, 255)
    return img


def _save_png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img, "RGB").save(path)


# ------------------------------------------------------------------------------------------------------------ OBJ
def _write_obj(path, form, negative=False, colors=None, poly=POLY, poly_vt=POLY_VT, poly_vn=None, mtl="m.mtl", materials=("skin",)):
    """form: 'v', 'v/vt', 'v//vn' or 'v/vt/vn'; negative: every index written relative to the end of its list"""
    lines = ["# written by the test", "mtllib %s" % mtl] if mtl else []
    for i, p in enumerate(VERT):
        lines.append("v %r %r %r" % tuple(float(x) for x in p) + (" %r %r %r" % tuple(float(c) for c in colors[i]) if colors is not None else ""))
    lines += ["vt %r %r" % (float(u), float(v)) for u, v in VT[:-1]] + ["vt %r %r 0.0" % tuple(float(x) for x in VT[-1])]
    lines += ["vn %r %r %r" % tuple(float(x) for x in n) for n in NORM]

    def ref(i, n):
        return str(i - n if negative else i + 1)

    for k, (face, face_vt) in enumerate(zip(poly, poly_vt)):
        if k < len(materials) and materials[k]:
            lines.append("usemtl %s" % materials[k])
        face_vn = poly_vn[k] if poly_vn else face
        corner = {"v": lambda a, b, c: ref(a, len(VERT)), "v/vt": lambda a, b, c: ref(a, len(VERT)) + "/" + ref(b, len(VT)),
                  "v//vn": lambda a, b, c: ref(a, len(VERT)) + "//" + ref(c, len(NORM)),
                  "v/vt/vn": lambda a, b, c: ref(a, len(VERT)) + "/" + ref(b, len(VT)) + "/" + ref(c, len(NORM))}[form]
        lines.append("f " + " ".join(corner(a, b, c) for a, b, c in zip(face, face_vt, face_vn)))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _write_mtl(path, entries):
    with open(path, "w") as fh:
        for name, map_kd in entries:
            fh.write("newmtl %s\nKd 0.8 0.8 0.8\n" % name + ("map_Kd %s\n" % map_kd if map_kd else ""))


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("form", ["v", "v/vt", "v//vn", "v/vt/vn"])
def test_load_obj_corner_forms(tmp_path, form, negative):
    from sam6d_hip import onboard
    img = _image((5, 3))
    _save_png(str(tmp_path / "tex" / "skin.png"), img)
    _write_mtl(str(tmp_path / "m.mtl"), [("skin", "-s 1 1 1 tex\\skin.png")])  # options are read over; a backslash path
    p = str(tmp_path / "m.obj")
    _write_obj(p, form, negative)
    m = onboard.load_mesh(p)
    assert m["vertices"].dtype == np.float32 and np.array_equal(m["vertices"], VERT)  # the file's v order
    assert m["faces"].dtype == np.int32 and np.array_equal(m["faces"], TRIS) and m["colors"] is None
    if "vn" in form:
        assert m["normals"].dtype == np.float32 and np.array_equal(m["normals"], NORM)
    else:
        assert m["normals"] is None
    if "vt" in form:
        assert m["face_uv"].dtype == np.float32 and m["face_uv"].shape == (4, 3, 2) and np.array_equal(m["face_uv"], VT[TRIS_VT])
        assert m["texture_file"] == str(tmp_path / "tex" / "skin.png")
        assert m["texture"].dtype == np.uint8 and np.array_equal(m["texture"], img)
    else:
        assert m["face_uv"] is None and m["texture_file"] is None and m["texture"] is None


def test_load_obj_colours_normals_and_no_image(tmp_path):
    from sam6d_hip import onboard
    p = str(tmp_path / "m.obj")
    col = np.array([[1.0, 0.0, 0.5], [0.2, 0.4, 0.6], [1.5, -0.2, 0.999], [0.0019, 0.002, 0.7 / 255], [0.25, 0.75, 1.0]])
    _write_mtl(str(tmp_path / "m.mtl"), [("skin", None)])  # a material without an image: the mesh renders as an untextured one
    _write_obj(p, "v/vt/vn", colors=col, poly_vn=[[0, 1, 2, 3], [0, 1, 4], [3, 2, 0]])  # vertex 4 meets vn 4 and vn 0
    m = onboard.load_obj(p)
    assert m["colors"].dtype == np.uint8
    assert m["colors"].tolist() == [[255, 0, 128], [51, 102, 153], [255, 0, 255], [0, 1, 1], [64, 191, 255]]  # floor(255 c + 0.5), clamped
    assert m["normals"] is None  # a position index with two vn indices: face-normal shading
    assert m["face_uv"] is None and m["texture_file"] is None
    _write_obj(p, "v/vt/vn", mtl=None)
    m = onboard.load_mesh(p)
    assert np.array_equal(m["normals"], NORM) and m["face_uv"] is None and m["texture"] is None


def test_load_obj_refusals(tmp_path):
    from sam6d_hip import onboard
    p = str(tmp_path / "m.obj")
    _write_mtl(str(tmp_path / "m.mtl"), [("skin", "a.png"), ("lid", "sub/b.png"), ("same", "./a.png")])
    _write_obj(p, "v/vt", poly=[[0, 1, 2, 3, 4]], poly_vt=[[0, 1, 2, 3, 4]])
    with pytest.raises(ValueError, match="5 corners"):
        onboard.load_obj(p)
    _write_obj(p, "v/vt", materials=("skin", "lid"))
    with pytest.raises(ValueError, match=r"2 diffuse images.*a\.png.*b\.png"):
        onboard.load_obj(p)
    _write_obj(p, "v/vt", materials=("skin", "same"))  # two materials, one image
    assert onboard.load_obj(p)["texture_file"] == str(tmp_path / "a.png")
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "a.png"))):
        onboard.load_mesh(p)  # the image the MTL names does not exist
    with open(p, "a") as fh:
        fh.write("f 1 2 5\n")
    with pytest.raises(ValueError, match="with and without"):
        onboard.load_obj(p)
    _write_obj(p, "v/vt", mtl="gone.mtl")
    with pytest.raises(FileNotFoundError, match="gone.mtl"):
        onboard.load_obj(p)
    open(p, "w").write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="vertex index 4"):
        onboard.load_obj(p)
    for name in ("m.stl", "m", "m.obj.gz"):
        with pytest.raises(ValueError, match="extension"):
            onboard.load_mesh(str(tmp_path / name))


# ------------------------------------------------------------------------------------------------------------ PLY
def _write_textured_ply(path, binary, vertex_uv=None, face_uv=False, texture_file=None, texnumber=True):
    """vertex_uv: the names of two per-vertex properties holding VT[:5]; face_uv: MeshLab's texcoord list (from POLY_VT)"""
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test"]
    if texture_file:
        head.append("comment TextureFile %s" % texture_file)
    head += ["element vertex %d" % len(VERT), "property float x", "property float y", "property float z"]
    if vertex_uv:
        head += ["property float %s" % vertex_uv[0], "property float %s" % vertex_uv[1]]
    head += ["element face %d" % len(POLY), "property list uchar int vertex_indices"]
    if face_uv:
        head += ["property list uchar float texcoord"] + (["property int texnumber"] if texnumber else [])
    head += ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for i in range(len(VERT)):
            row = list(VERT[i]) + (list(VT[i]) if vertex_uv else [])
            fh.write(np.array(row, "<f4").tobytes() if binary else (" ".join("%r" % float(x) for x in row) + "\n").encode())
        for face, face_vt in zip(POLY, POLY_VT):
            tex = VT[face_vt].reshape(-1)
            if binary:
                fh.write(np.array([len(face)], "u1").tobytes() + np.array(face, "<i4").tobytes())
                if face_uv:
                    fh.write(np.array([len(tex)], "u1").tobytes() + tex.astype("<f4").tobytes() + (np.array([0], "<i4").tobytes() if texnumber else b""))
            else:
                row = [str(len(face))] + [str(x) for x in face]
                if face_uv:
                    row += [str(len(tex))] + ["%r" % float(x) for x in tex] + (["0"] if texnumber else [])
                fh.write((" ".join(row) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("names", [("texture_u", "texture_v"), ("s", "t"), ("u", "v")])
def test_load_ply_vertex_uv(tmp_path, binary, names):
    from sam6d_hip import onboard
    img = _image((4, 6), 1)
    _save_png(str(tmp_path / "obj_000001.png"), img)
    p = str(tmp_path / "obj_000001.ply")
    _write_textured_ply(p, binary, vertex_uv=names, texture_file="obj_000001.png")
    m = onboard.load_mesh(p)
    assert np.array_equal(m["vertices"], VERT) and np.array_equal(m["faces"], TRIS) and m["normals"] is None and m["colors"] is None
    assert m["face_uv"].dtype == np.float32 and np.array_equal(m["face_uv"], VT[:5][TRIS])  # the quad's split included
    assert m["texture_file"] == str(tmp_path / "obj_000001.png") and np.array_equal(m["texture"], img)
    assert set(onboard.load_ply(p)) == {"vertices", "faces", "normals", "colors", "face_uv", "texture_file"}


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("texnumber", [False, True])
def test_load_ply_face_texcoord(tmp_path, binary, texnumber):
    from sam6d_hip import onboard
    p = str(tmp_path / "scan.ply")
    _write_textured_ply(p, binary, face_uv=True, texnumber=texnumber, vertex_uv=("s", "t") if texnumber else None)
    m = onboard.load_ply(p)
    assert np.array_equal(m["vertices"], VERT) and np.array_equal(m["faces"], TRIS)
    assert m["face_uv"].dtype == np.float32 and np.array_equal(m["face_uv"], VT[TRIS_VT])  # per corner: wins over the per-vertex pair
    assert m["texture_file"] is None and onboard.load_mesh(p)["texture"] is None


def test_load_ply_texture_refusals(tmp_path):
    from sam6d_hip import onboard
    p = str(tmp_path / "scan.ply")
    _write_textured_ply(p, False, vertex_uv=("s", "t"), texture_file="nowhere/skin.png")
    assert onboard.load_ply(p)["texture_file"] == str(tmp_path / "nowhere" / "skin.png")
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "nowhere" / "skin.png"))):
        onboard.load_mesh(p)
    head = b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
    vert = b"0 0 0\n1 0 0\n0 1 0\n"
    open(p, "wb").write(head + b"property list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n" + vert + b"3 0 1 2 4 0 0 1 0\n")
    with pytest.raises(ValueError, match="texcoord list of 4 values"):
        onboard.load_ply(p)
    open(p, "wb").write(head + b"property list uchar int vertex_indices\nproperty list uchar int flags\nend_header\n" + vert + b"3 0 1 2 1 0\n")
    with pytest.raises(ValueError, match="flags"):
        onboard.load_ply(p)


# ------------------------------------------------------------------------------------------------------------ images
def test_load_texture(tmp_path):
    from PIL import Image
    from sam6d_hip import onboard
    img = _image((37, 90), 2)
    p = str(tmp_path / "t.png")
    _save_png(p, img)
    assert np.array_equal(onboard.load_texture(p), img) and np.array_equal(onboard.load_texture(p, max_side=90), img)
    for max_side, factor in ((89, 2), (45, 2), (44, 3), (30, 3), (8, 12), (1, 90)):  # the smallest factor that brings 90 to or below max_side
        got = onboard.load_texture(p, max_side=max_side)
        assert np.array_equal(got, np.asarray(Image.fromarray(img, "RGB").reduce(factor))), max_side
        assert max(got.shape[:2]) <= max_side and (factor == 1 or -(-90 // (factor - 1)) > max_side)
    Image.fromarray(img[:, :, 0], "L").save(p)  # a grey image: three equal channels
    assert np.array_equal(onboard.load_texture(p), np.repeat(img[:, :, :1], 3, axis=2))
    Image.fromarray(np.zeros((1, 8193, 3), np.uint8), "RGB").save(p)
    with pytest.raises(ValueError, match="1 x 8193"):
        onboard.load_texture(p)
    assert onboard.load_texture(p, max_side=8192).shape == (1, 4097, 3)
    for bad in (0, 8193):
        with pytest.raises(ValueError, match="max_side"):
            onboard.load_texture(p, max_side=bad)


def test_texel_table():
    from sam6d_hip import onboard
    t = onboard.texel_table()
    assert t.dtype == np.float32 and t.shape == (256,) and t[0] == 0 and t[255] == 1
    assert np.array_equal(t, np.arange(256).astype(np.float32) / np.float32(255))  # the vertex-colour path's (float)byte / 255.0f
    s = onboard.texel_table(decode_srgb=True)
    assert s.dtype == np.float32 and s[0] == 0 and s[255] == 1 and (np.diff(s) > 0).all()
    assert abs(s[188] - 0.5) < 3e-3 and abs(s[10] - 10 / 255 / 12.92) < 1e-9  # the inverse of srgb_table()'s 0.5 -> 188
    lut = onboard.srgb_table()
    assert np.array_equal(lut[np.floor(s.astype(np.float64) * 4095 + 0.5).astype(int)], np.arange(256))  # round trip through both tables


def test_face_uv_and_texture_go_together():
    from sam6d_hip import onboard
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    args = (v, f, None, None, torch.zeros(1, 3, 4), torch.zeros(1, 3), (1, 1, 0, 0), (4, 4))
    with pytest.raises(ValueError, match="texture is missing"):
        onboard.render_views(*args, face_uv=torch.zeros(1, 3, 2))
    with pytest.raises(ValueError, match="face_uv is missing"):
        onboard.render_views(*args, texture=torch.zeros(2, 2, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):  # both: as far as the device check, as without them
        onboard.render_views(*args, face_uv=torch.zeros(1, 3, 2), texture=torch.zeros(2, 2, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["octahedron", "icosphere"])
def test_constant_texture_equals_constant_vertex_colours(name):
    """The anchor to tests/raster_ref.py: under a texture of one colour c (5 x 3 texels, arbitrary face_uv) the restatement's rgb is,
    bit for bit, raster_ref.render's with every vertex colour c -- and the other five outputs are raster_ref's anyway."""
    from sam6d_hip import onboard
    v, f = RR.octahedron() if name == "octahedron" else RR.icosphere(1)
    v = (v * np.float32(50.0)).astype(np.float32)
    view, light = onboard.view_matrices(POSES[[0, 17, 41]], 0.5 / 50.0)
    intr = onboard.intrinsics_from_fov(64, 0.691111)
    lut = onboard.srgb_table()
    g = np.random.default_rng(7)
    c = np.array([200, 100, 50], np.uint8)
    face_uv = (g.random((len(f), 3, 2)) * 5 - 2).astype(np.float32)
    texture = np.broadcast_to(c, (5, 3, 3)).copy()
    got = TR.render(v, f, None, face_uv, texture, onboard.texel_table(), view, light, intr, (64, 64), NEAR, lut)
    want = RR.render(v, f, None, np.broadcast_to(c, (len(v), 3)).copy(), view, light, intr, (64, 64), NEAR, 0.05, False, lut)
    assert (got["mask"] == 255).sum() > 3 * 900
    assert (got["albedo"][got["mask"] == 255] == (c.astype(np.float32) / np.float32(255))).all()
    for k in ("mask", "face", "depth", "xyz", "n_dropped"):
        assert np.array_equal(got[k], want[k]), k
    print("%s: %d of %d rgb bytes differ" % (name, int((got["rgb"] != want["rgb"]).sum()), got["rgb"].size))
    assert np.array_equal(got["rgb"], want["rgb"])


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("b", [0, 77, 255])
def test_one_texel_equals_the_grey_render(b, with_normals):
    """The two resolve kernels share one core, so the restatements must agree where the albedos do: a 1 x 1 texture of bytes (b, b, b)
    filters to a + fx * (a - a) = a = texel_table()[b] exactly, and the textured render is the grey render (colorize) with that
    base_color on all six outputs, bit for bit.  tests/test_texture_gpu.py holds the device to the same, device against device."""
    from sam6d_hip import onboard
    v, f = RR.icosphere(1, 50.0)
    view, light = onboard.view_matrices(POSES[[0, 41]], 0.5 / 50.0)
    intr = (0.5 * 33 / np.tan(0.5 * 0.691111), 0.5 * 33 / np.tan(0.5 * 0.691111), 0.5 * 33, 0.5 * 17)
    lut, table = onboard.srgb_table(), onboard.texel_table()
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    face_uv = (np.random.default_rng(b).random((len(f), 3, 2)) * 3 - 1).astype(np.float32)
    got = TR.render(v, f, normals, face_uv, np.full((1, 1, 3), b, np.uint8), table, view, light, intr, (17, 33), NEAR, lut)
    want = RR.render(v, f, normals, None, view, light, intr, (17, 33), NEAR, float(table[b]), True, lut)
    assert (got["mask"] == 255).sum() > 80
    for k in ("mask", "face", "depth", "xyz", "rgb", "n_dropped"):
        assert np.array_equal(got[k], want[k]), k


def _px(points, z=1.0):
    p = np.asarray(points, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(p),))
    return np.stack([p[:, 0] * z, p[:, 1] * z, z], axis=1).astype(np.float32)


def _lookup64(u, v, texture):
    """float64 bilinear, repeat-wrapped lookup of texture / 255, written with the modulo: independent of texture_ref's index steps"""
    Ht, Wt = texture.shape[:2]
    tx = (u - np.floor(u)) * Wt - 0.5
    ty = (1.0 - (v - np.floor(v))) * Ht - 0.5
    x0, y0 = np.floor(tx).astype(int), np.floor(ty).astype(int)
    fx, fy = (tx - x0)[:, None], (ty - y0)[:, None]
    t = texture.astype(np.float64) / 255.0
    top = t[y0 % Ht, x0 % Wt] * (1 - fx) + t[y0 % Ht, (x0 + 1) % Wt] * fx
    bot = t[(y0 + 1) % Ht, x0 % Wt] * (1 - fx) + t[(y0 + 1) % Ht, (x0 + 1) % Wt] * fx
    return top * (1 - fy) + bot * fy, (x0, y0)


def test_albedo_against_a_float64_lookup():
    """A tilted quad of two triangles (depth 1.2 .. 4) under a 7 x 5 random texture whose coordinates run past both ends of [0, 1], at
    48 x 40.  The float64 side: the pixel centre's ray meets the winning face's plane (Moeller-Trumbore in camera space: the
    perspective-correct barycentrics without the recipe's screen-space weights), its UV, and a repeat-wrapped bilinear lookup.
        |albedo - albedo64| <= 1e-5 + Sx * Wt * |u - u64| + Sy * Ht * |v - v64|
    Sx, Sy: the largest step between neighbouring texels (with the wrap) along each axis; a bilinear surface moves by at most that
    per texel, and Wt |du| texels is how far the two lookups stand apart.  1e-5: fp32 round-off of the lookup itself (tx carries
    3 operations on a value below 7, about 1e-6 texel, times a step below 1; the three lerps 6 more roundings of values below 1).
    |u - u64|, |v - v64| <= 2e-3: the recipe snaps vertices to 1/256 pixel, at most 1/512 pixel per axis, on a quad 27 pixels across
    at its narrowest over which the coordinates run by 1.9: 1.4e-4 in the plane of the screen, times up to (4 / 1.2)^2 = 11 where the
    perspective stretches it.  An affine interpolation is off by up to 0.2 here.  No pixel is left out (the issue allows 1 %):
    the bound holds across texel cells because the filter is continuous.  Measured: largest |duv| 1.7e-4, largest error 8.6e-4, largest error / bound 0.82."""
    from sam6d_hip import onboard
    quad = [(4.3, 5.1), (44.2, 3.4), (40.6, 36.7), (6.8, 33.2)]
    z = [1.5, 4.0, 3.0, 1.2]
    v = _px(quad, z)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    corner_uv = np.array([[-0.3, -0.2], [1.6, 0.1], [1.4, 1.7], [-0.1, 1.3]], np.float32)
    face_uv = corner_uv[f]
    texture = _image((5, 7), 3)
    out = TR.render(v, f, None, face_uv, texture, onboard.texel_table(), EYE, LIGHT0, PIXEL, (40, 48), NEAR, onboard.srgb_table())
    ys, xs = np.nonzero(out["mask"][0])
    assert len(ys) > 900
    face = out["face"][0][ys, xs]
    P = v.astype(np.float64)
    A, B, C = P[f[face, 0]], P[f[face, 1]], P[f[face, 2]]
    d = np.stack([xs + 0.5, ys + 0.5, np.ones(len(xs))], axis=1)
    e1, e2 = B - A, C - A
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    b1 = ((-A) * pv).sum(-1) / det
    b2 = (d * np.cross(-A, e1)).sum(-1) / det
    cu = corner_uv.astype(np.float64)[f[face]]  # (n, corner, 2)
    uv64 = (1 - b1 - b2)[:, None] * cu[:, 0] + b1[:, None] * cu[:, 1] + b2[:, None] * cu[:, 2]
    want, _ = _lookup64(uv64[:, 0], uv64[:, 1], texture)
    duv = np.abs(out["uv"][0][ys, xs].astype(np.float64) - uv64)
    t = texture.astype(np.float64) / 255.0
    Sx = np.abs(t - np.roll(t, 1, axis=1)).max()
    Sy = np.abs(t - np.roll(t, 1, axis=0)).max()
    bound = 1e-5 + Sx * 7 * duv[:, 0] + Sy * 5 * duv[:, 1]
    err = np.abs(out["albedo"][0][ys, xs].astype(np.float64) - want).max(axis=1)
    print("largest |duv| %.3g, largest error / bound %.3f, largest error %.3g" % (duv.max(), (err / bound).max(), err.max()))
    assert duv.max() <= 2e-3
    assert (err <= bound).all()
    assert (uv64.min(axis=0) < -0.1).all() and (uv64.max(axis=0) > 1.1).all()  # the wrap is exercised on both axes and both sides


def test_orientation_texel_centres_on_pixel_centres():
    """A fronto-parallel quad over the pixels [2, 2 + Wt) x [1, 1 + Ht) whose corners carry (0, 1) top left, (1, 1) top right, (1, 0)
    bottom right and (0, 0) bottom left: every pixel centre is a texel centre, so albedo is the image itself, row 0 along the quad's
    v = 1 edge -- no half-texel shift, no flip.  Tolerance 1e-5: u is a mix of three weights (8 roundings of a value below 1, 5e-7),
    times Wt = 7 texels, times a step below 1 between neighbouring texels."""
    from sam6d_hip import onboard
    Ht, Wt = 5, 7
    texture = _image((Ht, Wt), 4)
    v = _px([(2, 1), (2 + Wt, 1), (2 + Wt, 1 + Ht), (2, 1 + Ht)], 2.0)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    corner_uv = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)
    out = TR.render(v, f, None, corner_uv[f], texture, onboard.texel_table(), EYE, LIGHT0, PIXEL, (Ht + 3, Wt + 4), NEAR, onboard.srgb_table())
    want = np.zeros((Ht + 3, Wt + 4), bool)
    want[1:1 + Ht, 2:2 + Wt] = True
    assert np.array_equal(out["mask"][0] == 255, want)
    got = out["albedo"][0][1:1 + Ht, 2:2 + Wt]
    assert np.abs(got - texture.astype(np.float32) / np.float32(255)).max() <= 1e-5
    # and the repeat: the same quad with every coordinate moved by whole numbers is the same picture
    again = TR.render(v, f, None, (corner_uv + np.float32([3, -2]))[f], texture, onboard.texel_table(), EYE, LIGHT0, PIXEL, (Ht + 3, Wt + 4),
                      NEAR, onboard.srgb_table())
    assert np.abs(again["albedo"] - out["albedo"]).max() <= 1e-5


def test_wrap_edge_cases():
    """NaN, both infinities, the rounding case a - floor(a) == 1 and exact integers all land on texel coordinate 0"""
    a = np.array([np.nan, np.inf, -np.inf, -1e-9, 1.0, -1.0, 3.0, 0.0, 3.25, -2.5], np.float32)
    assert TR.wrap(a).tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25, 0.5]
    tex = _image((3, 4), 5)
    lut = np.arange(256).astype(np.float32) / np.float32(255)
    bad = TR.lookup(np.array([np.nan, np.inf], np.float32), np.array([0.0, -np.inf], np.float32), tex, lut)
    zero = TR.lookup(np.zeros(2, np.float32), np.zeros(2, np.float32), tex, lut)
    assert np.array_equal(bad, zero)
    # (u, v) = (0, 0): half way between the first and last column and between the last and first row
    t = lut[tex]
    want = (t[2, 3] + np.float32(0.5) * (t[2, 0] - t[2, 3]))
    want = want + np.float32(0.5) * ((t[0, 3] + np.float32(0.5) * (t[0, 0] - t[0, 3])) - want)
    assert np.array_equal(zero[0], want)


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_c_entry_refuses_by_name_before_a_launch():
    from sam6d_hip import _lib

    def render(T=1, H=8, W=8, F=1, V=3, near=1e-3, wave_area=0, ptr=64, ws=1 << 20, Ht=4, Wt=4, tex=64, uv=64, texel=64):
        # (refused before a pointer is followed: 64 stands for "not null")
        _lib.call("sam6d_render_views_textured", ptr, V, ptr, F, None, ptr, ptr, T, 1.0, 1.0, 0.0, 0.0, H, W, near, 0.05, ptr, wave_area, uv, tex,
                  Ht, Wt, texel, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ws, None)

    for kw, name in ((dict(H=0), "H x W"), (dict(W=2049), "H x W"), (dict(T=0), "T = 0"), (dict(T=1025), "T = 1025"), (dict(F=0), "F = 0"),
                     (dict(F=(1 << 24) + 1), "F = 16777217"), (dict(V=0), "V = 0"), (dict(near=0.0), "near"), (dict(wave_area=-1), "wave_area"),
                     (dict(ptr=None), "null pointer"), (dict(tex=None), "null pointer"), (dict(uv=None), "null pointer"),
                     (dict(texel=None), "null pointer"), (dict(ws=8 * 8 * 8 - 1), "workspace of 511 bytes"), (dict(ptr=68), "workspace is not 8-byte aligned"),
                     (dict(Ht=0), "Ht x Wt = 0 x 4"), (dict(Wt=8193), "Ht x Wt = 4 x 8193"), (dict(Ht=-1), "Ht x Wt"), (dict(tex=66), "texture is not 4-byte aligned")):
        with pytest.raises(RuntimeError, match="render_views_textured: .*" + name):
            render(**kw)


# ------------------------------------------------------------------------------------------------------------ the kernel
def test_kernel_resources():
    """textured_resolve_kernel uses no scratch and spills nothing, and keeps within its built VGPR count (52)
    rounded up to the next step of 8.  Only the register, scratch and spill notes of the code object are read."""
    from tests._util import kernel_resources
    found = kernel_resources(b"textured_resolve_kernel")
    print("\n[texture] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == {"textured_resolve_kernel"}, found  # the visibility kernel stays in raster.hip's code object
    assert found["textured_resolve_kernel"][0] <= 56 and found["textured_resolve_kernel"][1:] == (0, 0), found
