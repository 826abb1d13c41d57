"""Onboarding a CAD model on the device: what Render/render_custom_templates.py does with BlenderProc, trimesh and cv2 -- the rendered
templates (rgb_i.png, mask_i.png, xyz_i.npy) that ISM/run_inference_custom.py:131-146 and PEM/run_inference_custom_pytorch.py:195-201
read -- and the trimesh surface samples of the two inference scripts, without any of the three.

What is pinned and what is not.  The reference tree holds no rendered template, and BlenderProc, trimesh and cv2 cannot be imported
where this was built.  The GEOMETRY (mask, visible face, depth, object-space xyz, sampled points) is therefore defined by the recipes
at the top of csrc/raster.hip and csrc/meshsample.hip and checked bit for bit against their numpy restatements (tests/raster_ref.py,
tests/meshsample_ref.py).  The SHADING of rgb and the sampler's random stream are the package's own: parity unpinned against Cycles /
trimesh, equal in distribution only.  The image size (512) and field of view (0.691111 rad) are what BlenderProc's default
configuration is believed to use; that could not be verified, so they are parameters.

Imports runtime, _lib, torch and numpy only.  There is no CPU route: a CPU tensor raises.
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
LIGHT_SCALE = 2.5   # render_custom_templates.py:77
NEAR = 1.0e-3       # in scene units; a template camera stands at four object radii

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply(path):
    """A triangle mesh from a PLY file, numpy only: ASCII and binary little-endian; vertex x / y / z, optional nx / ny / nz and
    red / green / blue (uchar); faces of three or four indices (a quad splits as 0-1-2, 0-2-3).  Other vertex properties and other
    elements are read over.  -> dict(vertices (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None, colors (V,3) u8 or None).
    Anything else (another format, a polygon with more corners, a missing coordinate) raises ValueError naming it."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("load_ply: %s is not a PLY file (no 'ply' ... 'end_header')" % path)
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
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
    vert = faces = None
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
        if len(props) != 1 and name == "face":
            raise ValueError("load_ply: a face element with properties beside its index list is not supported")
        rows = []
        for _ in range(count):  # (a list element is read row by row; elements other than face are read over the same way)
            for _, t in props:
                if t[0] != "list":
                    if fmt == "ascii":
                        pos += 1
                    else:
                        pos += np.dtype(_PLY_TYPES[t[0]]).itemsize
                    continue
                if fmt == "ascii":
                    k = int(ascii_tokens[pos])
                    idx = [int(v) for v in ascii_tokens[pos + 1:pos + 1 + k]]
                    pos += 1 + k
                else:
                    ct, it = np.dtype("<" + _PLY_TYPES[t[1]]), np.dtype("<" + _PLY_TYPES[t[2]])
                    k = int(np.frombuffer(body, dtype=ct, count=1, offset=pos)[0])
                    idx = np.frombuffer(body, dtype=it, count=k, offset=pos + ct.itemsize).tolist()
                    pos += ct.itemsize + k * it.itemsize
                if name == "face":
                    if k == 3:
                        rows.append(idx)
                    elif k == 4:
                        rows.append([idx[0], idx[1], idx[2]])
                        rows.append([idx[0], idx[2], idx[3]])
                    else:
                        raise ValueError("load_ply: a face with %d corners is not supported (triangles and quads are)" % k)
        if name == "face":
            faces = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    if vert is None or any(k not in vert for k in "xyz"):
        raise ValueError("load_ply: no vertex element with x, y, z")
    if faces is None or faces.shape[0] == 0:
        raise ValueError("load_ply: no face element (a point cloud cannot be rendered or sampled)")

    def stack(keys, dtype):
        return np.ascontiguousarray(np.stack([vert[k] for k in keys], axis=1).astype(dtype)) if all(k in vert for k in keys) else None

    return dict(vertices=stack("xyz", np.float32), faces=faces, normals=stack(("nx", "ny", "nz"), np.float32),
                colors=stack(("red", "green", "blue"), np.uint8))


def _mesh_tensors(mesh, device=None):
    """vertices f32, faces i32, normals, colors of a mesh dict (numpy or tensors) as contiguous tensors on one HIP device."""
    v = mesh["vertices"]
    if device is None:
        device = v.device if torch.is_tensor(v) else torch.device("cuda")

    def put(x, dtype):
        return None if x is None else torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()

    return put(v, torch.float32), put(mesh["faces"], torch.int32), put(mesh.get("normals"), torch.float32), put(mesh.get("colors"), torch.uint8)


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


@on_tensor_device
def render_views(vertices, faces, normals, colors, view, light, intrinsics, size, *, near=NEAR, base_color=0.05, colorize=False,
                 wave_area=0):
    """sam6d_render_views: T views of one mesh.  vertices (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None, colors (V,3) u8 or
    None, view (T,3,4) f32, light (T,3) f32 -- HIP tensors; intrinsics (fx, fy, cx, cy) in pixels, size (H, W).  -> dict(mask (T,H,W)
    u8, face (T,H,W) i32, depth (T,H,W) f32, xyz (T,H,W,3) f32 in CAD units, rgb (T,H,W,3) u8, n_dropped (T) i32).  The recipe is at
    the top of csrc/raster.hip.  wave_area: the bounding-box area from which a whole wave takes a face (0 = the library's 256)."""
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
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    lut = torch.from_numpy(srgb_table()).to(vertices.device)
    need = _lib.load().sam6d_render_views_workspace_bytes(T, H, W)
    ws = _empty((need // 8,), vertices, torch.int64)
    out = dict(mask=_empty((T, H, W), vertices, torch.uint8), face=_empty((T, H, W), vertices, torch.int32), depth=_empty((T, H, W), vertices),
               xyz=_empty((T, H, W, 3), vertices), rgb=_empty((T, H, W, 3), vertices, torch.uint8), n_dropped=_empty((T,), vertices, torch.int32))
    _lib.call("sam6d_render_views", _p(vertices), V, _p(faces), F, _p(normals), _p(colors), _p(view), _p(light), T, fx, fy, cx, cy, H, W,
              float(near), float(base_color), int(bool(colorize)), lut.data_ptr(), int(wave_area), out["mask"].data_ptr(), _p(out["face"]),
              _p(out["depth"]), _p(out["xyz"]), out["rgb"].data_ptr(), _p(out["n_dropped"]), ws.data_ptr(), ws.numel() * 8, _s())
    return out


def intrinsics_from_fov(size, fov):
    """(fx, fy, cx, cy) of a square image of `size` pixels whose horizontal field of view is `fov` radians."""
    f = 0.5 * size / np.tan(0.5 * fov)
    return (f, f, 0.5 * size, 0.5 * size)


def render_templates(mesh, cam_poses, *, normalize=True, colorize=False, base_color=0.05, size=512, fov=0.691111, seed=0):
    """Render/render_custom_templates.py:45-106 for one mesh: mesh = dict(vertices, faces[, normals, colors]) (load_ply's, numpy or
    HIP tensors), cam_poses (T,4,4) = the reference's cam_poses_level0.npy, loaded by the caller (the package ships no copy).
    normalize: scale the object by norm_scale (`seed` is the sampler's) as the script's --normalize does.  size and fov: BlenderProc's
    defaults as far as known (see the module docstring).  -> dict of HIP tensors: rgb (T,S,S,3) u8, mask (T,S,S) u8 0 / 255, xyz
    (T,S,S,3) f32 in CAD units (what the script saves as 2 * (nocs - 0.5), :104-106), depth, face, n_dropped, and scale (a float).
    A face in front of the near plane is an error here: a template camera stands at four object radii."""
    v, f, nrm, col = _mesh_tensors(mesh)
    scale = norm_scale(v, f, seed) if normalize else 1.0
    view, light = view_matrices(cam_poses, scale)
    out = render_views(v, f, nrm, col, torch.from_numpy(view).to(v.device), torch.from_numpy(light).to(v.device),
                       intrinsics_from_fov(size, fov), (size, size), base_color=float(base_color), colorize=bool(colorize))
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
