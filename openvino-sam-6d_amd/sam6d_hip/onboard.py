"""Onboarding a CAD model on the device: what Render/render_custom_templates.py does with BlenderProc, trimesh and cv2 -- the rendered
templates (rgb_i.png, mask_i.png, xyz_i.npy) that ISM/run_inference_custom.py:131-146 and PEM/run_inference_custom_pytorch.py:195-201
read -- and the trimesh surface samples of the two inference scripts, without any of the three.

What is pinned and what is not.  The reference tree holds no rendered template, and BlenderProc, trimesh and cv2 cannot be imported
where this was built.  The GEOMETRY (mask, visible face, depth, object-space xyz, sampled points) is therefore defined by the recipes
at the top of csrc/raster.hip and csrc/meshsample.hip and checked bit for bit against their numpy restatements (tests/raster_ref.py,
tests/meshsample_ref.py).  The SHADING of rgb and the sampler's random stream are the package's own: parity unpinned against Cycles /
trimesh, equal in distribution only.  The image size (512) and field of view (0.691111 rad) are what BlenderProc's default
configuration is believed to use; that could not be verified, so they are parameters.

A model may carry one texture image (an OBJ with its MTL, or a PLY that names a TextureFile): load_mesh reads it, and the renderer
takes the albedo from it by the TEXTURE recipe at the top of csrc/texture.hip (restated in tests/texture_ref.py); the geometry of a
textured render is the untextured one's.

Imports runtime, _lib, torch and numpy only (PIL inside load_texture and save_templates).  There is no CPU route: a CPU tensor raises.
"""
import os

import numpy as np
import torch

from . import _lib
from .runtime import _empty, _p, _s, on_tensor_device

MAX_SIZE = 2048     # H, W of sam6d_render_views
MAX_VIEWS = 1024
MAX_FACES = 1 << 24
MAX_SAMPLES = 1 << 24
MAX_TEXTURE = 8192  # Ht, Wt of sam6d_render_views_textured
LIGHT_SCALE = 2.5   # render_custom_templates.py:77
NEAR = 1.0e-3       # in scene units; a template camera stands at four object radii

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


_PLY_UV = (("texture_u", "texture_v"), ("s", "t"), ("u", "v"))


def _beside(path, name):
    """the file `name` (as a model file writes it: backslashes allowed) relative to the directory of `path`"""
    return os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(path)), name.strip().replace("\\", "/")))


def load_ply(path):
    """A triangle mesh from a PLY file, numpy only: ASCII and binary little-endian; vertex x / y / z, optional nx / ny / nz and
    red / green / blue (uchar); faces of three or four indices (a quad splits as 0-1-2, 0-2-3).  Other vertex properties and other
    elements are read over.  Texture coordinates: per-vertex texture_u / texture_v (or s / t, or u / v: the BOP models' way), expanded
    to the faces' corners, or a face element that carries a `texcoord` list of 6 floats (8 for a quad) beside its index list and any
    scalar properties such as texnumber (MeshLab's way; it wins where a file has both); `comment TextureFile NAME` names the image,
    relative to the PLY.  -> dict(vertices (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None, colors (V,3) u8 or None, face_uv
    (F,3,2) f32 or None, texture_file: a path or None).  Anything else (another format, a polygon with more corners, a missing
    coordinate, another list on a face) raises ValueError naming it."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("load_ply: %s is not a PLY file (no 'ply' ... 'end_header')" % path)
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements, texture_file = None, [], None
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if len(tok) >= 3 and tok[0] == "comment" and tok[1] == "TextureFile" and texture_file is None:
            texture_file = _beside(path, line.split(None, 2)[2])
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("load_ply: property before any element")
            for t in tok[1:-1]:
                if t != "list" and t not in _PLY_TYPES:
                    raise ValueError("load_ply: unknown property type '%s'" % t)
            elements[-1][2].append((tok[-1], tuple(tok[1:-1])))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("load_ply: format '%s' is not supported (ascii and binary_little_endian are)" % fmt)
    ascii_tokens = body.split() if fmt == "ascii" else None
    pos = 0
    vert = faces = face_uv = None
    for name, count, props in elements:
        has_list = any(t[0] == "list" for _, t in props)
        if not has_list:
            dt = np.dtype([(n, "<" + _PLY_TYPES[t[0]]) for n, t in props])
            if fmt == "ascii":
                flat = np.array(ascii_tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                pos += count * len(props)
                rec = {n: flat[:, k] for k, (n, _) in enumerate(props)}
            else:
                arr = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                rec = {n: arr[n] for n, _ in props}
            if name == "vertex":
                vert = rec
            continue
        lists = [n for n, t in props if t[0] == "list"]
        if name == "face" and (len(lists) > 2 or (len(lists) == 2 and "texcoord" not in lists) or lists == ["texcoord"]):
            raise ValueError("load_ply: a face element with lists %s is not supported (its index list and a texcoord list are)" % lists)
        rows, uv_rows = [], []
        for _ in range(count):  # (a list element is read row by row; elements other than face are read over the same way)
            idx = tex = None
            for pname, t in props:
                if t[0] != "list":
                    if fmt == "ascii":
                        pos += 1
                    else:
                        pos += np.dtype(_PLY_TYPES[t[0]]).itemsize
                    continue
                if fmt == "ascii":
                    k = int(ascii_tokens[pos])
                    item = [float(v) if _PLY_TYPES[t[2]][0] == "f" else int(v) for v in ascii_tokens[pos + 1:pos + 1 + k]]
                    pos += 1 + k
                else:
                    ct, it = np.dtype("<" + _PLY_TYPES[t[1]]), np.dtype("<" + _PLY_TYPES[t[2]])
                    k = int(np.frombuffer(body, dtype=ct, count=1, offset=pos)[0])
                    item = np.frombuffer(body, dtype=it, count=k, offset=pos + ct.itemsize).tolist()
                    pos += ct.itemsize + k * it.itemsize
                if pname == "texcoord" and len(lists) == 2:
                    tex = item
                else:
                    idx = item
            if name != "face":
                continue
            k = len(idx)
            if k not in (3, 4):
                raise ValueError("load_ply: a face with %d corners is not supported (triangles and quads are)" % k)
            if tex is not None and len(tex) != 2 * k:
                raise ValueError("load_ply: a face with %d corners has a texcoord list of %d values (%d expected)" % (k, len(tex), 2 * k))
            for a, b, c in ((0, 1, 2), (0, 2, 3))[:k - 2]:
                rows.append([idx[a], idx[b], idx[c]])
                if tex is not None:
                    uv_rows.append([tex[2 * a:2 * a + 2], tex[2 * b:2 * b + 2], tex[2 * c:2 * c + 2]])
        if name == "face":
            faces = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
            face_uv = np.asarray(uv_rows, dtype=np.float32).reshape(-1, 3, 2) if uv_rows else None
    if vert is None or any(k not in vert for k in "xyz"):
        raise ValueError("load_ply: no vertex element with x, y, z")
    if faces is None or faces.shape[0] == 0:
        raise ValueError("load_ply: no face element (a point cloud cannot be rendered or sampled)")

    def stack(keys, dtype):
        return np.ascontiguousarray(np.stack([vert[k] for k in keys], axis=1).astype(dtype)) if all(k in vert for k in keys) else None

    if face_uv is None:
        uv = next((stack(keys, np.float32) for keys in _PLY_UV if all(k in vert for k in keys)), None)
        if uv is not None:
            if faces.min() < 0 or faces.max() >= uv.shape[0]:
                raise ValueError("load_ply: face indices span %d .. %d, outside the %d vertices" % (faces.min(), faces.max(), uv.shape[0]))
            face_uv = np.ascontiguousarray(uv[faces])
    return dict(vertices=stack("xyz", np.float32), faces=faces, normals=stack(("nx", "ny", "nz"), np.float32),
                colors=stack(("red", "green", "blue"), np.uint8), face_uv=face_uv, texture_file=texture_file)


def load_obj(path):
    """A triangle mesh from a Wavefront OBJ file with its MTL, numpy only (what bproc.loader.load_obj takes at
    Render/render_custom_templates.py:60).  `v x y z [r g b]` (the optional float colours become u8 by floor(255 c + 0.5), clamped;
    kept only when every vertex has them), `vt u v [w]`, `vn`, and `f` with corners v, v/vt, v//vn or v/vt/vn, negative (relative)
    indices included; triangles and quads (a quad splits as 0-1-2, 0-2-3).  The vertices keep the file's `v` order: the geometry is
    the file's, nothing is split along texture seams, so texture coordinates are per corner (face_uv).  normals (V,3) is set only
    when every position index meets one and the same `vn` index throughout the file (a vertex no face uses gets 0); otherwise
    normals is None, which selects face-normal shading -- there are no per-corner normals.  mtllib / usemtl: `newmtl` and `map_Kd`
    are read, the image's name is the last token of map_Kd (its options are not applied), relative to the MTL.  The faces may use one
    distinct diffuse image: several raise ValueError naming them, as does a mix of faces with and without vt.  No vt, or no map_Kd
    at all, gives face_uv = None and texture_file = None: the mesh renders by its colours or base_color.  -> load_ply's dict."""
    verts, cols, vts, vns, maps = [], [], [], [], {}
    corners, uses = [], []  # per triangle: three (v, vt, vn) with None where absent; the material in force
    material = None

    def index(text, n, what):
        i = int(text)
        i = n + i if i < 0 else i - 1
        if not 0 <= i < n:
            raise ValueError("load_obj: %s index %s is outside the %d read so far" % (what, text, n))
        return i

    with open(path, "r", errors="replace") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError("load_obj: a vertex with %d coordinates" % (len(tok) - 1))
                verts.append([float(x) for x in tok[1:4]])
                if len(tok) >= 7:
                    cols.append([float(x) for x in tok[4:7]])
            elif tok[0] == "vt":
                vts.append([float(tok[1]), float(tok[2]) if len(tok) > 2 else 0.0])
            elif tok[0] == "vn":
                vns.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                k = len(tok) - 1
                if k not in (3, 4):
                    raise ValueError("load_obj: a face with %d corners is not supported (triangles and quads are)" % k)
                cs = []
                for c in tok[1:]:
                    part = c.split("/") + ["", ""]
                    cs.append((index(part[0], len(verts), "vertex"), index(part[1], len(vts), "vt") if part[1] else None,
                               index(part[2], len(vns), "vn") if part[2] else None))
                for a, b, c in ((0, 1, 2), (0, 2, 3))[:k - 2]:
                    corners.append((cs[a], cs[b], cs[c]))
                    uses.append(material)
            elif tok[0] == "usemtl":
                material = line.split("#", 1)[0].split(None, 1)[1].strip()
            elif tok[0] == "mtllib":
                mtl = _beside(path, line.split("#", 1)[0].split(None, 1)[1])
                if not os.path.isfile(mtl):
                    raise FileNotFoundError("load_obj: %s names the material library %s, which does not exist" % (path, mtl))
                name = None
                with open(mtl, "r", errors="replace") as mh:
                    for mline in mh:
                        mtok = mline.split("#", 1)[0].split()
                        if len(mtok) >= 2 and mtok[0] == "newmtl":
                            name = mline.split("#", 1)[0].split(None, 1)[1].strip()
                            maps.setdefault(name, None)
                        elif len(mtok) >= 2 and mtok[0] == "map_Kd" and name is not None:
                            maps[name] = _beside(mtl, mtok[-1])
    if not verts or not corners:
        raise ValueError("load_obj: %s has no %s (a point cloud cannot be rendered or sampled)" % (path, "faces" if verts else "vertices"))
    V = len(verts)
    vertices = np.asarray(verts, np.float32)
    faces = np.asarray([[c[0] for c in tri] for tri in corners], np.int32)
    colors = None
    if len(cols) == V:
        colors = np.clip(np.floor(255.0 * np.asarray(cols, np.float64) + 0.5), 0, 255).astype(np.uint8)
    normals = None
    if vns and all(c[2] is not None for tri in corners for c in tri):
        met = np.full(V, -1, np.int64)
        for tri in corners:
            for v, _, n in tri:
                if met[v] not in (-1, n):
                    met = None
                    break
                met[v] = n
            if met is None:
                break
        if met is not None:
            normals = np.where((met >= 0)[:, None], np.asarray(vns, np.float32)[np.maximum(met, 0)], np.float32(0)).astype(np.float32)
    with_vt = [all(c[1] is not None for c in tri) for tri in corners]
    if any(with_vt) and not all(with_vt):
        raise ValueError("load_obj: %d of the %d triangles have no vt at some corner: a mix of faces with and without texture "
                         "coordinates is not supported" % (with_vt.count(False), len(with_vt)))
    images = sorted({maps[m] for m in uses if maps.get(m) is not None})
    if len(images) > 1:
        raise ValueError("load_obj: the faces use %d diffuse images (%s); one texture per mesh is supported" % (len(images), ", ".join(images)))
    face_uv = texture_file = None
    if all(with_vt) and images:
        uv = np.asarray(vts, np.float32)
        face_uv = np.ascontiguousarray(uv[np.asarray([[c[1] for c in tri] for tri in corners], np.int64)])
        texture_file = images[0]
    return dict(vertices=vertices, faces=faces, normals=normals, colors=colors, face_uv=face_uv, texture_file=texture_file)


def load_texture(path, max_side=None):
    """An image file as a texture: (Ht,Wt,3) u8 through PIL's convert("RGB"), row 0 the top row.  max_side: reduce the image by the
    smallest integer factor that brings both sides to or below it, with PIL's Image.reduce (an exact box mean).  That is all the
    filtering there is: the renderer has no mip chain, so a texture much finer than the rendered surface aliases unless it is reduced
    here.  Sides outside 1 .. 8192 (after the reduction) raise ValueError."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if max_side is not None:
            if not 1 <= int(max_side) <= MAX_TEXTURE:
                raise ValueError("load_texture: max_side = %s is not in 1 .. %d" % (max_side, MAX_TEXTURE))
            factor = -(-max(im.size) // int(max_side))
            if factor > 1:
                im = im.reduce(factor)
        tex = np.array(im, dtype=np.uint8)  # (a copy: PIL's buffer is read-only)
    if not (1 <= tex.shape[0] <= MAX_TEXTURE and 1 <= tex.shape[1] <= MAX_TEXTURE):
        raise ValueError("load_texture: %s is %d x %d texels, not in 1 .. %d (pass max_side to reduce it)"
                         % (path, tex.shape[0], tex.shape[1], MAX_TEXTURE))
    return tex


def load_mesh(path):
    """load_ply or load_obj by the file's extension, with the image the file names loaded into mesh["texture"] ((Ht,Wt,3) u8, or
    None): what render_templates takes.  Another extension raises ValueError, a named image that does not exist FileNotFoundError."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".ply", ".obj"):
        raise ValueError("load_mesh: %s has the extension '%s'; .ply and .obj are read" % (path, ext))
    mesh = load_ply(path) if ext == ".ply" else load_obj(path)
    mesh["texture"] = None
    if mesh["texture_file"] is not None:
        if not os.path.isfile(mesh["texture_file"]):
            raise FileNotFoundError("load_mesh: %s names the texture %s, which does not exist" % (path, mesh["texture_file"]))
        mesh["texture"] = load_texture(mesh["texture_file"])
    return mesh


def _mesh_tensors(mesh, device=None, texture=False):
    """vertices f32, faces i32, normals, colors of a mesh dict (numpy or tensors) as contiguous tensors on one HIP device; with
    `texture`, also face_uv f32 and texture u8 (None where the mesh has none)."""
    v = mesh["vertices"]
    if device is None:
        device = v.device if torch.is_tensor(v) else torch.device("cuda")

    def put(x, dtype):
        return None if x is None else torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()

    out = (put(v, torch.float32), put(mesh["faces"], torch.int32), put(mesh.get("normals"), torch.float32), put(mesh.get("colors"), torch.uint8))
    return out + (put(mesh.get("face_uv"), torch.float32), put(mesh.get("texture"), torch.uint8)) if texture else out


def _check_mesh(vertices, faces):
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices must be (V,3) float32")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("faces must be (F,3) int32")
    V, F = vertices.shape[0], faces.shape[0]
    if not 1 <= F <= MAX_FACES:
        raise ValueError("F = %d is not in 1 .. %d" % (F, MAX_FACES))
    if V < 1:
        raise ValueError("V = %d is not positive" % V)
    return V, F


def _check_indices(faces, V):
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= V:
        raise ValueError("face indices span %d .. %d, outside the %d vertices" % (lo, hi, V))


@on_tensor_device
def _sample_surface(vertices, faces, n, seed, row):
    V, F = _check_mesh(vertices, faces)
    _check_indices(faces, V)
    need = _lib.load().sam6d_mesh_sample_workspace_bytes(F)
    ws = _empty(((need + 7) // 8,), vertices, torch.int64)
    points = _empty((n, 3), vertices)
    face = _empty((n,), vertices, torch.int32)
    _lib.call("sam6d_mesh_sample", _p(vertices), V, _p(faces), F, n, int(seed) & 0xFFFFFFFF, int(row) & 0xFFFFFFFF, _p(points), _p(face),
              ws.data_ptr(), ws.numel() * 8, _s())
    return points, face


def sample_surface(vertices, faces, n, seed=0, row=0):
    """n area-weighted points of the surface (trimesh.sample.sample_surface's role: Render/render_custom_templates.py:35), drawn on
    the device: vertices (V,3) f32 and faces (F,3) i32 HIP tensors -> points (n,3) f32, face ids (n) i32.  Sample j is sample row + j
    of the stream `seed`: a function of (mesh, seed, row + j) alone, defined in csrc/meshsample.hip -- NOT trimesh's stream, equal
    in distribution only.  n outside 1 .. 2^24 raises ValueError; a mesh without area raises RuntimeError."""
    n = int(n)
    if not 1 <= n <= MAX_SAMPLES:
        raise ValueError("sample_surface: n = %d is not in 1 .. %d" % (n, MAX_SAMPLES))
    return _sample_surface(vertices, faces, n, seed, row)


def norm_scale(vertices, faces, seed=0):
    """get_norm_info (Render/render_custom_templates.py:32-43): 1 / (2 * radius) with radius the larger norm of the two corners of the
    bounding box of 1024 surface samples -- the scale that puts that radius at 0.5.  A host float (one read-back)."""
    pts, _ = sample_surface(vertices, faces, 1024, seed)
    corners = torch.stack([pts.min(dim=0).values, pts.max(dim=0).values]).cpu().numpy().astype(np.float32)
    radius = max(float(np.linalg.norm(corners[1])), float(np.linalg.norm(corners[0])))
    return 1.0 / (2.0 * radius)


def model_points(mesh, n, seed=0):
    """mesh.sample(n).astype(np.float32) / 1000 of the inference scripts (ISM/run_inference_custom.py:232-234,
    PEM/run_inference_custom_pytorch.py:298-300): (n,3) f32 host array in metres, what inputs.test_data(model_points=...) takes."""
    v, f, _, _ = _mesh_tensors(mesh)
    pts, _ = sample_surface(v, f, n, seed)
    return pts.cpu().numpy().astype(np.float32) / np.float32(1000.0)


def view_matrices(cam_poses, scale=1.0):
    """The camera and light of Render/render_custom_templates.py:72-82 as the renderer's per-view inputs.  cam_poses (T,4,4): the
    predefined poses (cam_poses_level0.npy: camera-to-object, millimetres, z forward).  The script flips columns 1 and 2 into
    Blender's camera frame, scales the position by 0.001 * 2, scales the object by `scale` and puts a point light at 2.5 x the camera
    position.  -> view (T,3,4) f32, the matrix that takes a CAD-unit point to the camera frame the rasteriser uses (x right, y down,
    z forward: Blender's frame with y and z flipped back), and light (T,3) f32 in that frame.  Float64 throughout, rounded once.
    The input is not modified (the script's in-place edit is)."""
    pose = np.array(cam_poses, dtype=np.float64, copy=True).reshape(-1, 4, 4)
    pose[:, :3, 1:3] = -pose[:, :3, 1:3]                 # :72
    pose[:, :3, 3] = pose[:, :3, 3] * 0.001 * 2          # :73
    light_world = LIGHT_SCALE * pose[:, :3, 3]           # :81
    flip = np.diag([1.0, -1.0, -1.0])
    view = np.empty((pose.shape[0], 3, 4))
    light = np.empty((pose.shape[0], 3))
    for t in range(pose.shape[0]):
        w2c = flip @ np.linalg.inv(pose[t])[:3]          # world -> Blender camera -> (x right, y down, z forward)
        view[t, :, :3] = w2c[:, :3] * float(scale)       # the object is scaled about its origin (:61)
        view[t, :, 3] = w2c[:, 3]
        light[t] = w2c[:, :3] @ light_world[t] + w2c[:, 3]
    return view.astype(np.float32), light.astype(np.float32)


def srgb_table():
    """The 4096-entry u8 table of the sRGB transfer function at k / 4095, in float64."""
    x = np.arange(4096, dtype=np.float64) / 4095.0
    y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    return np.floor(255.0 * y + 0.5).astype(np.uint8)


def texel_table(decode_srgb=False):
    """The 256-entry f32 table that turns a texture byte into an albedo.  Default: np.float32(k) / np.float32(255), the very values
    the vertex-colour path computes from its bytes.  decode_srgb: the sRGB-to-linear transfer of k / 255, in float64, rounded once."""
    if not decode_srgb:
        return np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.arange(256, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, np.power((x + 0.055) / 1.055, 2.4)).astype(np.float32)


def render_views(vertices, faces, normals, colors, view, light, intrinsics, size, *, near=NEAR, base_color=0.05, colorize=False,
                 wave_area=0, face_uv=None, texture=None, decode_srgb=False):
    """sam6d_render_views: T views of one mesh.  vertices (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None, colors (V,3) u8 or
    None, view (T,3,4) f32, light (T,3) f32 -- HIP tensors; intrinsics (fx, fy, cx, cy) in pixels, size (H, W).  -> dict(mask (T,H,W)
    u8, face (T,H,W) i32, depth (T,H,W) f32, xyz (T,H,W,3) f32 in CAD units, rgb (T,H,W,3) u8, n_dropped (T) i32).  The recipe is at
    the top of csrc/raster.hip.  wave_area: the bounding-box area from which a whole wave takes a face (0 = the library's 256).
    face_uv (F,3,2) f32 and texture (Ht,Wt,3) or (Ht,Wt,4) u8 (the fourth byte is ignored), both HIP tensors and both or neither:
    with them and without colorize the albedo is the texture's (sam6d_render_views_textured, the TEXTURE recipe at the top of
    csrc/texture.hip; colors is then not used); decode_srgb takes the texture's bytes through the sRGB-to-linear table first
    (texel_table).  Without them every line is the untextured route."""
    if (face_uv is None) != (texture is None):
        raise ValueError("render_views: face_uv and texture go together (%s is missing)" % ("texture" if texture is None else "face_uv"))
    return _render_views(vertices, faces, normals, colors, view, light, intrinsics, size, near, base_color, colorize, wave_area, face_uv,
                         texture, decode_srgb)


@on_tensor_device
def _render_views(vertices, faces, normals, colors, view, light, intrinsics, size, near, base_color, colorize, wave_area, face_uv, texture,
                  decode_srgb):
    V, F = _check_mesh(vertices, faces)
    _check_indices(faces, V)
    H, W = int(size[0]), int(size[1])
    T = int(view.shape[0])
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError("render_views: H x W = %d x %d is not in 1 .. %d" % (H, W, MAX_SIZE))
    if not 1 <= T <= MAX_VIEWS:
        raise ValueError("render_views: T = %d is not in 1 .. %d" % (T, MAX_VIEWS))
    view, light = view.contiguous(), light.contiguous()
    if tuple(view.shape) != (T, 3, 4) or view.dtype != torch.float32 or tuple(light.shape) != (T, 3) or light.dtype != torch.float32:
        raise ValueError("render_views: view must be (T,3,4) and light (T,3), float32")
    for name, t, dt in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if t is not None and (tuple(t.shape) != (V, 3) or t.dtype != dt or not t.is_contiguous()):
            raise ValueError("render_views: %s must be a contiguous (V,3) %s tensor" % (name, dt))
    if texture is not None:
        for name, t in (("face_uv", face_uv), ("texture", texture)):
            if not torch.is_tensor(t) or t.device != vertices.device:
                raise ValueError("render_views: %s must be a tensor on the mesh's device (%s)" % (name, vertices.device))
        if tuple(face_uv.shape) != (F, 3, 2) or face_uv.dtype != torch.float32:
            raise ValueError("render_views: face_uv must be (F,3,2) float32")
        if texture.dim() != 3 or texture.shape[2] not in (3, 4) or texture.dtype != torch.uint8:
            raise ValueError("render_views: texture must be (Ht,Wt,3) or (Ht,Wt,4) uint8")
        Ht, Wt = int(texture.shape[0]), int(texture.shape[1])
        if not (1 <= Ht <= MAX_TEXTURE and 1 <= Wt <= MAX_TEXTURE):
            raise ValueError("render_views: texture Ht x Wt = %d x %d is not in 1 .. %d" % (Ht, Wt, MAX_TEXTURE))
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    lut = torch.from_numpy(srgb_table()).to(vertices.device)
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = _empty((need // 8,), vertices, torch.int64)
    out = dict(mask=_empty((T, H, W), vertices, torch.uint8), face=_empty((T, H, W), vertices, torch.int32), depth=_empty((T, H, W), vertices),
               xyz=_empty((T, H, W, 3), vertices), rgb=_empty((T, H, W, 3), vertices, torch.uint8), n_dropped=_empty((T,), vertices, torch.int32))
    if texture is not None and not colorize:
        face_uv = face_uv.contiguous()
        if texture.shape[2] == 3:  # one aligned 4-byte texel: padded once, here
            texture = torch.cat([texture, torch.zeros((Ht, Wt, 1), dtype=torch.uint8, device=texture.device)], dim=2)
        texture = texture.contiguous()
        texel = torch.from_numpy(texel_table(decode_srgb)).to(vertices.device)
        _lib.call("sam6d_render_views_textured", _p(vertices), V, _p(faces), F, _p(normals), _p(view), _p(light), T, fx, fy, cx, cy, H, W,
                  float(near), float(base_color), lut.data_ptr(), int(wave_area), _p(face_uv), texture.data_ptr(), Ht, Wt, _p(texel),
                  out["mask"].data_ptr(), _p(out["face"]), _p(out["depth"]), _p(out["xyz"]), out["rgb"].data_ptr(), _p(out["n_dropped"]),
                  ws.data_ptr(), ws.numel() * 8, _s())
        return out
    _lib.call("sam6d_render_views", _p(vertices), V, _p(faces), F, _p(normals), _p(colors), _p(view), _p(light), T, fx, fy, cx, cy, H, W,
              float(near), float(base_color), int(bool(colorize)), lut.data_ptr(), int(wave_area), out["mask"].data_ptr(), _p(out["face"]),
              _p(out["depth"]), _p(out["xyz"]), out["rgb"].data_ptr(), _p(out["n_dropped"]), ws.data_ptr(), ws.numel() * 8, _s())
    return out


def intrinsics_from_fov(size, fov):
    """(fx, fy, cx, cy) of a square image of `size` pixels whose horizontal field of view is `fov` radians."""
    f = 0.5 * size / np.tan(0.5 * fov)
    return (f, f, 0.5 * size, 0.5 * size)


def render_templates(mesh, cam_poses, *, normalize=True, colorize=False, base_color=0.05, size=512, fov=0.691111, seed=0,
                     decode_srgb=False):
    """Render/render_custom_templates.py:45-106 for one mesh: mesh = dict(vertices, faces[, normals, colors, face_uv, texture])
    (load_mesh's, numpy or HIP tensors), cam_poses (T,4,4) = the reference's cam_poses_level0.npy, loaded by the caller (the package
    ships no copy).  The albedo, in order of precedence: colorize (base_color), the texture (face_uv and texture both present;
    decode_srgb as render_views), the vertex colours, base_color.
    normalize: scale the object by norm_scale (`seed` is the sampler's) as the script's --normalize does.  size and fov: BlenderProc's
    defaults as far as known (see the module docstring).  -> dict of HIP tensors: rgb (T,S,S,3) u8, mask (T,S,S) u8 0 / 255, xyz
    (T,S,S,3) f32 in CAD units (what the script saves as 2 * (nocs - 0.5), :104-106), depth, face, n_dropped, and scale (a float).
    A face in front of the near plane is an error here: a template camera stands at four object radii."""
    v, f, nrm, col, uv, tex = _mesh_tensors(mesh, texture=True)
    if uv is None or tex is None:  # (a mesh with only one of the two renders as an untextured one)
        uv = tex = None
    scale = norm_scale(v, f, seed) if normalize else 1.0
    view, light = view_matrices(cam_poses, scale)
    out = render_views(v, f, nrm, col, torch.from_numpy(view).to(v.device), torch.from_numpy(light).to(v.device),
                       intrinsics_from_fov(size, fov), (size, size), base_color=float(base_color), colorize=bool(colorize), face_uv=uv,
                       texture=tex, decode_srgb=bool(decode_srgb))
    dropped = out["n_dropped"].cpu().numpy()
    if dropped.any():
        raise RuntimeError("render_templates: views %s have faces nearer than the near plane (%s faces): the camera is inside or too "
                           "close to the object" % (np.nonzero(dropped)[0].tolist(), dropped[dropped > 0].tolist()))
    out["scale"] = float(scale)
    return out


def save_templates(out, directory):
    """The files the inference scripts read (ISM/run_inference_custom.py:131-146, PEM/run_inference_custom_pytorch.py:195-201), as the
    render script names them (:98-106): rgb_i.png (RGB), mask_i.png (L, 0 / 255), xyz_i.npy (float16), written with PIL and numpy
    into `directory`.  -> the directory."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    rgb, mask, xyz = out["rgb"].cpu().numpy(), out["mask"].cpu().numpy(), out["xyz"].cpu().numpy()
    for i in range(rgb.shape[0]):
        Image.fromarray(rgb[i], "RGB").save(os.path.join(directory, "rgb_%d.png" % i))
        Image.fromarray(mask[i], "L").save(os.path.join(directory, "mask_%d.png" % i))
        np.save(os.path.join(directory, "xyz_%d.npy" % i), xyz[i].astype(np.float16))
    return directory
