"""Onboarding a CAD model (sam6d_hip.onboard, csrc/raster.hip, csrc/meshsample.hip) without a GPU: the numpy restatements
(tests/raster_ref.py, tests/meshsample_ref.py) against checks that do not depend on them -- a float64 ray caster, reprojection,
anchors, on-face residuals, chi-square -- the PLY reader, the template files, the view matrices, the import layer, what is refused
before a launch, and the kernels' registers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshsample_ref as MS
from tests import raster_ref as RR
from tests._util import PKG, ROOT, kernel_resources

POSES = np.load(os.path.join(ROOT, "tests", "golden", "template_cam_poses.npz"))["cam_poses"]
NEAR = 1.0e-3


def _scene(mesh, size, poses=(0, 17, 41), radius=50.0):
    from sam6d_hip import onboard
    v, f = mesh
    v = (v * np.float32(radius)).astype(np.float32)
    view, light = onboard.view_matrices(POSES[list(poses)], 0.5 / radius)
    return v, f, view, light, onboard.intrinsics_from_fov(size, 0.691111)


@pytest.fixture(scope="module")
def rendered():
    """the restatement's renders of the two meshes at 64 x 64 from three fixture poses, shared by the tests below"""
    from sam6d_hip import onboard
    out = {}
    # poses: of the 42, the icosphere's 480 edges leave under 2 % of the mask within 2/256 pixel of an edge from about one in four
    # (by the float64 ray caster's count, 1.5 % to 3.1 %); three of those are taken
    for name, mesh, poses in (("octahedron", RR.octahedron(), (0, 17, 41)), ("icosphere", RR.icosphere(2), (6, 10, 36))):
        v, f, view, light, intr = _scene(mesh, 64, poses)
        out[name] = (v, f, view, intr, RR.render(v, f, None, None, view, light, intr, (64, 64), NEAR, 0.05, False, onboard.srgb_table()))
    return out


def _ray_cast(v, f, M, intr, H, W):
    """Float64 ray caster, independent of the rasteriser's recipe: Moeller-Trumbore per pixel centre and face in camera space.
    -> nearest face (H,W; -1 none), its depth and object-space point, the relative gap to the second depth, the distance in pixels
    from each centre to the nearest projected edge, and dxyz (H,W,4): how far the hit's (depth, x, y, z) moves when the ray moves by
    1/256 pixel in x plus 1/256 pixel in y on the hit face's plane."""
    fx, fy, cx, cy = intr
    M = np.asarray(M, np.float64)
    P = v.astype(np.float64) @ M[:, :3].T + M[:, 3]
    A, B, C = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)

    def hit(dx, dy):
        d = np.stack([(jj + dx - cx) / fx, (ii + dy - cy) / fy, np.ones_like(jj)], axis=-1).reshape(-1, 1, 3)
        e1, e2 = (B - A)[None], (C - A)[None]
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        with np.errstate(all="ignore"):
            tv = -A[None]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1)
            w = (d * qv).sum(-1) / det
            t = (e2 * qv).sum(-1) / det
        return u, w, t  # (HW, F)

    u, w, t = hit(0.0, 0.0)
    inside = (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0) & np.isfinite(t)
    tt = np.where(inside, t, np.inf)
    order = np.argsort(tt, axis=1)
    rows = np.arange(tt.shape[0])
    first, second = tt[rows, order[:, 0]], tt[rows, order[:, 1]]
    face = np.where(np.isfinite(first), order[:, 0], -1)
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(second), (second - first) / first, np.inf)
    vo = v.astype(np.float64)

    def attrs(u, w, t):
        k = np.maximum(face, 0)
        uu, ww = u[rows, k], w[rows, k]
        xyz = (1 - uu - ww)[:, None] * vo[f[k, 0]] + uu[:, None] * vo[f[k, 1]] + ww[:, None] * vo[f[k, 2]]
        return np.concatenate([t[rows, k][:, None], xyz], axis=1)

    a0 = attrs(u, w, t)
    s = 1.0 / 256.0
    dxyz = np.abs(attrs(*hit(s, 0.0)) - a0) + np.abs(attrs(*hit(0.0, s)) - a0)
    # distance from every centre to every projected edge segment
    sx, sy = fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy
    S = np.stack([sx, sy], axis=1)
    c = np.stack([jj.ravel(), ii.ravel()], axis=1)[:, None]
    dist = np.full(c.shape[0], np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        p, q = S[f[:, a]][None], S[f[:, b]][None]
        seg = q - p
        tpar = np.clip(((c - p) * seg).sum(-1) / np.maximum((seg * seg).sum(-1), 1e-300), 0, 1)
        dist = np.minimum(dist, np.sqrt((((p + tpar[..., None] * seg) - c) ** 2).sum(-1)).min(axis=1))
    sh = (H, W)
    return face.reshape(sh), a0[:, 0].reshape(sh), a0[:, 1:].reshape(H, W, 3), gap.reshape(sh), dist.reshape(sh), dxyz.reshape(H, W, 4)


@pytest.mark.parametrize("name", ["octahedron", "icosphere"])
def test_restatement_against_a_float64_ray_caster(rendered, name):
    """Mask and visible face equal the ray caster's outside the ambiguous pixels (a centre within 2/256 pixel of a projected edge, or
    two nearest depths within 1e-5 relative), and those are below 2 % of the mask.  On the rest, depth and xyz stay within
        bound = S + 32 * 2^-24 * magnitude.
    32 * 2^-24 * magnitude: unit round-off of fp32 times the recipe's operation count on the way to an attribute (projection 7,
    snap 4, edge conversion and weights 12, mix 5, rounded up) times the largest coordinate (the depth, or the largest |vertex|).
    S: the recipe snaps every projected vertex to 1/256 pixel, which moves the interpolating triangle by up to 1/512 pixel per axis
    under the fixed pixel centre; to first order the attribute moves by at most that displacement times its screen-space gradient.
    S is the ray caster's own change of the attribute for a ray moved by 1/256 pixel in x plus 1/256 in y on the hit face's plane:
    twice the largest snap per axis, which also covers the fp32 error of the projected coordinate (4 ulp of a 64-pixel coordinate
    is 3e-5 pixel).  Measured (radius 50 meshes at 64 x 64; octahedron from poses 0, 17, 41, icosphere from 6, 10, 36): ambiguous
    0 % and 1.5 - 1.8 % of the mask, largest error over bound 0.37 and 0.48."""
    v, f, view, intr, out = rendered[name]
    worst = 0.0
    for t in range(view.shape[0]):
        face, depth, xyz, gap, dist, sens = _ray_cast(v, f, view[t], intr, 64, 64)
        ambiguous = (dist <= 2.0 / 256.0) | (gap < 1e-5)
        n_mask = int((face >= 0).sum())
        assert n_mask > 300
        assert ambiguous[(face >= 0) | (out["mask"][t] > 0)].sum() < 0.02 * n_mask
        ok = ~ambiguous
        assert np.array_equal(out["face"][t][ok], face[ok])
        assert np.array_equal(out["mask"][t][ok] == 255, face[ok] >= 0)
        sel = ok & (face >= 0)
        mag = np.array([depth[sel].max()] + [np.abs(v).max()] * 3)
        bound = sens[sel] + 32 * 2.0 ** -24 * mag
        err = np.abs(np.concatenate([out["depth"][t][sel][:, None], out["xyz"][t][sel]], axis=1).astype(np.float64)
                     - np.concatenate([depth[sel][:, None], xyz[sel]], axis=1))
        worst = max(worst, float((err / bound).max()))
        print("%s view %d: mask %d, ambiguous %d, worst error / bound %.3f" % (name, t, n_mask, int(ambiguous[face >= 0].sum()), worst))
        assert (err <= bound).all()
        assert (out["depth"][t][out["mask"][t] == 0] == 0).all() and (out["face"][t][out["mask"][t] == 0] == -1).all()


@pytest.mark.parametrize("name", ["octahedron", "icosphere"])
def test_xyz_projects_back_into_its_pixel(rendered, name):
    """Independent of any restatement: xyz of a mask pixel, pushed through the view matrix and the intrinsics in float64, lands within
    0.5 pixel + the snap step (1/256) of the pixel's centre in both axes."""
    v, f, view, intr, out = rendered[name]
    fx, fy, cx, cy = intr
    for t in range(view.shape[0]):
        ys, xs = np.nonzero(out["mask"][t])
        M = view[t].astype(np.float64)
        P = out["xyz"][t][ys, xs].astype(np.float64) @ M[:, :3].T + M[:, 3]
        dx = np.abs(fx * P[:, 0] / P[:, 2] + cx - (xs + 0.5))
        dy = np.abs(fy * P[:, 1] / P[:, 2] + cy - (ys + 0.5))
        assert max(dx.max(), dy.max()) <= 0.5 + 1.0 / 256.0
        assert np.abs(P[:, 2] - out["depth"][t][ys, xs]).max() <= 1e-5 * P[:, 2].max()
        assert out["n_dropped"][t] == 0


def test_rgb_of_the_restatement_is_lit_and_grey(rendered):
    v, f, view, intr, out = rendered["icosphere"]
    rgb, mask = out["rgb"], out["mask"]
    assert (rgb[mask == 0] == 0).all()
    lit = rgb[mask == 255]
    assert (lit[:, 0] == lit[:, 1]).all() and (lit[:, 1] == lit[:, 2]).all()  # base_color grey
    assert 20 < lit.mean() < 120 and lit.max() > lit.min()  # albedo 0.05 under the script's light: dark, shaded, not black


# ------------------------------------------------------------------------------------------------------------ sampler
TRI = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 6], [5, 5, 5]], np.float32)


def test_sampler_anchors():
    assert ["%08x" % x for x in MS.keys(1, np.arange(4))] == ["dcacbaed", "f1040301", "f5d0477c", "57b6e681"]
    p, f = MS.sample(TRI, [[0, 1, 2], [0, 1, 3]], 4, seed=7, row=2)
    assert f.tolist() == [1, 0, 1, 1]
    assert p.tolist() == [[0.8892782926559448, 0.0, 2.2140347957611084], [1.0080128908157349, 0.7856429815292358, 0.0],
                          [0.18293821811676025, 0.0, 1.8775688409805298], [0.20886635780334473, 0.0, 4.798544883728027]]
    # one face: every sample on it, inside the triangle
    p, f = MS.sample(TRI, [[0, 1, 2]], 500, seed=3)
    assert (f == 0).all() and (p[:, 2] == 0).all() and (p[:, :2] >= 0).all() and (p[:, 0] + p[:, 1] <= 2.0 + 1e-6).all()
    # two faces with areas 1 : 3 (area 2 and 6): weights 2^24 / 3 floored and 2^24
    w = MS.weights(MS.areas(TRI, [[0, 1, 2], [0, 1, 3]]))
    assert w.tolist() == [5592405, 16777216]
    _, f = MS.sample(TRI, [[0, 1, 2], [0, 1, 3]], 40000, seed=0)
    assert abs((f == 1).mean() - 0.75) < 4 * (0.75 * 0.25 / 40000) ** 0.5
    # a zero-area face (a repeated vertex, and three points on a line) is never drawn, wherever it stands
    faces = [[0, 1, 1], [0, 1, 2], [0, 0, 0], [0, 1, 3], [1, 1, 2]]
    assert MS.weights(MS.areas(TRI, faces)).tolist() == [0, 5592405, 0, 16777216, 0]
    _, f = MS.sample(TRI, faces, 20000, seed=5)
    assert set(f.tolist()) == {1, 3}
    with pytest.raises(ValueError):
        MS.sample(TRI, [[0, 1, 1]], 4)
    # a face of negligible area still has weight 1; an index outside the vertices counts as no area
    tiny = np.array([[0, 0, 0], [1e-4, 0, 0], [0, 1e-4, 0], [100, 0, 0], [0, 100, 0]], np.float32)
    assert MS.weights(MS.areas(tiny, [[0, 1, 2], [0, 3, 4], [0, 3, 7]])).tolist() == [1, 16777216, 0]
    # rows of a longer draw
    a, fa = MS.sample(TRI, faces, 300, seed=9)
    b, fb = MS.sample(TRI, faces, 100, seed=9, row=200)
    assert np.array_equal(a[200:], b) and np.array_equal(fa[200:], fb)


@pytest.fixture(scope="module")
def ico_samples():
    v, f = RR.icosphere(2, 40.0)
    v = v * np.array([1.0, 0.6, 1.7], np.float32)  # faces of unequal area
    return v, f, {seed: MS.sample(v, f, 60000, seed=seed) for seed in (0, 1, 12345)}


def test_samples_lie_on_their_faces(ico_samples):
    """barycentric residual in float64 below 1e-6 of the longest edge: the point is its face's affine combination with weights in [0, 1]"""
    v, f, draws = ico_samples
    p, fid = draws[0]
    A, B, C = (v[f[fid, k]].astype(np.float64) for k in range(3))
    M = np.stack([B - A, C - A], axis=2)  # (n,3,2)
    rhs = p.astype(np.float64) - A
    sol = np.stack([np.linalg.lstsq(M[i], rhs[i], rcond=None)[0] for i in range(0, len(p), 50)])
    res = np.linalg.norm(np.einsum("nij,nj->ni", M[::50], sol) - rhs[::50], axis=1)
    edge = np.maximum(np.linalg.norm(B - A, axis=1), np.linalg.norm(C - A, axis=1))[::50]
    assert (res < 1e-6 * edge).all()
    assert (sol >= -1e-6).all() and (sol.sum(axis=1) <= 1 + 1e-6).all()


def _p_value(stat, dof):
    return float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64)))


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_face_counts_follow_the_areas(ico_samples, seed):
    """chi-square of the 320 face counts of 60 000 samples against the float64 areas: p >= 0.01 (tests/test_choice_host.py's bound).
    The weights are quantised to 2^-24 of the largest area: a relative error of the expectation far below the test's resolution."""
    v, f, draws = ico_samples
    A, B, C = (v[f[:, k]].astype(np.float64) for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(B - A, C - A), axis=1)
    e = 60000 * area / area.sum()
    c = np.bincount(draws[seed][1], minlength=len(f))
    p = _p_value(((c - e) ** 2 / e).sum(), len(f) - 1)
    print("seed %d: p = %.3f" % (seed, p))
    assert p >= 0.01
    # and the barycentric pair is uniform over the triangle: its mean is the centroid
    pts, fid = draws[seed]
    big = fid == np.argmax(c)
    centroid = (A + B + C)[np.argmax(c)] / 3
    assert np.linalg.norm(pts[big].mean(axis=0) - centroid) < 5 * np.linalg.norm((B - A)[np.argmax(c)]) / big.sum() ** 0.5


# ------------------------------------------------------------------------------------------------------------ files and views
def _write_ply(path, v, faces, normals=None, colors=None, binary=False, extra_element=False):
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        props += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test",
            "element vertex %d" % len(v)] + props
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices"]
    if extra_element:
        head += ["element edge 1", "property int vertex1", "property int vertex2"]
    head += ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for i in range(len(v)):
            row = list(v[i]) + (list(normals[i]) if normals is not None else [])
            col = (list(colors[i]) + [255]) if colors is not None else []
            if binary:
                fh.write(np.array(row, "<f4").tobytes() + np.array(col, "u1").tobytes())
            else:
                fh.write((" ".join(["%r" % float(x) for x in row] + ["%d" % c for c in col]) + "\n").encode())
        for face in faces:
            if binary:
                fh.write(np.array([len(face)], "u1").tobytes() + np.array(face, "<i4").tobytes())
            else:
                fh.write((" ".join(str(x) for x in [len(face)] + list(face)) + "\n").encode())
        if extra_element:
            fh.write(np.array([0, 1], "<i4").tobytes() if binary else b"0 1\n")


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply(tmp_path, binary):
    from sam6d_hip import onboard
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.25], [0.5, 0.5, 2]], np.float32)
    n = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0.6, 0.8, 0]], np.float32)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30], [200, 100, 50]], np.uint8)
    faces = [[0, 1, 2, 3], [0, 1, 4], [3, 2, 4]]
    want = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [3, 2, 4]], np.int32)
    p = str(tmp_path / "m.ply")
    _write_ply(p, v, faces, n, c, binary, extra_element=True)
    m = onboard.load_ply(p)
    assert m["vertices"].dtype == np.float32 and np.array_equal(m["vertices"], v)
    assert m["faces"].dtype == np.int32 and np.array_equal(m["faces"], want)
    assert m["normals"].dtype == np.float32 and np.array_equal(m["normals"], n)
    assert m["colors"].dtype == np.uint8 and np.array_equal(m["colors"], c)
    _write_ply(p, v, faces, None, None, binary)
    m = onboard.load_ply(p)
    assert np.array_equal(m["vertices"], v) and np.array_equal(m["faces"], want) and m["normals"] is None and m["colors"] is None
    _write_ply(p, v, [[0, 1, 2, 3, 4]], None, None, binary)
    with pytest.raises(ValueError, match="5 corners"):
        onboard.load_ply(p)


def test_load_ply_refusals(tmp_path):
    from sam6d_hip import onboard
    p = str(tmp_path / "bad.ply")
    open(p, "wb").write(b"solid not a ply\n")
    with pytest.raises(ValueError, match="not a PLY"):
        onboard.load_ply(p)
    open(p, "wb").write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        onboard.load_ply(p)
    open(p, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nelement face 0\n"
                        b"property list uchar int vertex_indices\nend_header\n0 0\n")
    with pytest.raises(ValueError, match="x, y, z"):
        onboard.load_ply(p)
    open(p, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    with pytest.raises(ValueError, match="no face element"):
        onboard.load_ply(p)
    open(p, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty quaternion x\nend_header\n")
    with pytest.raises(ValueError, match="quaternion"):
        onboard.load_ply(p)


def test_save_templates_round_trip(tmp_path):
    from PIL import Image
    from sam6d_hip import onboard
    g = np.random.default_rng(0)
    out = dict(rgb=torch.from_numpy(g.integers(0, 256, (3, 6, 5, 3), dtype=np.uint8)),
               mask=torch.from_numpy((g.random((3, 6, 5)) > 0.5).astype(np.uint8) * 255),
               xyz=torch.from_numpy((g.random((3, 6, 5, 3)) * 200 - 100).astype(np.float32)))
    d = onboard.save_templates(out, str(tmp_path / "templates"))
    assert sorted(os.listdir(d)) == sorted(["%s_%d.%s" % (k, i, e) for i in range(3) for k, e in (("rgb", "png"), ("mask", "png"), ("xyz", "npy"))])
    for i in range(3):
        rgb, mask, xyz = Image.open(os.path.join(d, "rgb_%d.png" % i)), Image.open(os.path.join(d, "mask_%d.png" % i)), \
            np.load(os.path.join(d, "xyz_%d.npy" % i))
        assert rgb.mode == "RGB" and mask.mode == "L" and xyz.dtype == np.float16 and xyz.shape == (6, 5, 3)
        assert np.array_equal(np.asarray(rgb), out["rgb"][i].numpy()) and np.array_equal(np.asarray(mask), out["mask"][i].numpy())
        assert set(np.unique(np.asarray(mask)).tolist()) <= {0, 255}
        assert np.array_equal(xyz, out["xyz"][i].numpy().astype(np.float16))


def test_view_matrices_follow_the_script():
    """Render/render_custom_templates.py:72-74 and :77-82 evaluated in float64 per pose, then taken to the rasteriser's frame: a
    Blender camera looks along -z with y up, so world -> camera is the inverse pose with rows 1 and 2 negated."""
    from sam6d_hip import onboard
    scale = 0.0123
    before = POSES.copy()
    view, light = onboard.view_matrices(POSES, scale)
    assert np.array_equal(POSES, before)  # the script edits its array in place; the function must not
    assert view.shape == (42, 3, 4) and view.dtype == np.float32 and light.shape == (42, 3) and light.dtype == np.float32
    for t in (0, 1, 17, 41):
        cam_pose = POSES[t].copy()
        cam_pose[:3, 1:3] = -cam_pose[:3, 1:3]
        cam_pose[:3, -1] = cam_pose[:3, -1] * 0.001 * 2
        light_w = np.array([2.5 * cam_pose[:3, -1][0], 2.5 * cam_pose[:3, -1][1], 2.5 * cam_pose[:3, -1][2]])
        R, c = cam_pose[:3, :3], cam_pose[:3, 3]
        for p in (np.zeros(3), np.array([30.0, -20.0, 55.0])):
            blender = R.T @ (scale * p - c)  # the scaled object's point in the Blender camera's frame
            want = blender * np.array([1.0, -1.0, -1.0])
            got = view[t].astype(np.float64) @ np.append(p, 1.0)
            assert np.abs(got - want).max() < 1e-6
        assert np.abs(light[t] - (R.T @ (light_w - c)) * np.array([1.0, -1.0, -1.0])).max() < 1e-6
        origin = view[t].astype(np.float64) @ np.array([0, 0, 0, 1.0])
        assert abs(origin[2] - 2.0) < 1e-5 and np.abs(origin[:2]).max() < 1e-5  # the camera looks at the object from four radii
        assert abs(np.linalg.norm(light[t]) - 3.0) < 1e-5  # 2.5 - 1 camera distances behind the camera


def test_srgb_table_and_intrinsics():
    from sam6d_hip import onboard
    lut = onboard.srgb_table()
    assert lut.dtype == np.uint8 and lut.shape == (4096,) and lut[0] == 0 and lut[-1] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    assert lut[round(0.5 * 4095)] == 188 and lut[round(0.05 * 4095)] == 63  # the sRGB transfer of 0.5 and 0.05
    fx, fy, cx, cy = onboard.intrinsics_from_fov(512, 0.691111)
    assert fx == fy and cx == cy == 256 and abs(2 * np.arctan(256 / fx) - 0.691111) < 1e-12


def test_module_imports_without_the_pipeline(tmp_path):
    """tests/test_import_layers_host.py's rule for the new module: importable without the shared library, and without sam6d_hip.pem"""
    child = ("import sys; sys.path.insert(0, %r)\nimport sam6d_hip.onboard\n"
             "print(' '.join(sorted(m for m in sys.modules if m == 'sam6d_hip' or m.startswith('sam6d_hip.') or m in ('PIL', 'cv2', 'trimesh'))))\n")
    env = dict(os.environ, SAM6D_LIB=str(tmp_path / "no_such_library.so"))
    r = subprocess.run([sys.executable, "-c", child % PKG], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert set(r.stdout.split()) == {"sam6d_hip", "sam6d_hip._lib", "sam6d_hip.runtime", "sam6d_hip.onboard"}, r.stdout


def test_render_script_has_the_reference_arguments():
    src = open(os.path.join(PKG, "render", "render_custom_templates.py")).read()
    for arg in ("--cad_path", "--output_dir", "--normalize", "--colorize", "--base_color", "--cam_poses"):
        assert arg in src
    assert not re.search(r"^\s*(import|from)\s+(blenderproc|trimesh|cv2)\b", src, flags=re.M)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_and_sizes_are_refused():
    from sam6d_hip import onboard
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        onboard.sample_surface(v, f, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        onboard.render_views(v, f, None, None, torch.zeros(1, 3, 4), torch.zeros(1, 3), (1, 1, 0, 0), (4, 4))
    for n in (0, -1, (1 << 24) + 1):
        with pytest.raises(ValueError, match="16777216"):
            onboard.sample_surface(v, f, n)


def test_c_entries_refuse_by_name_before_a_launch():
    from sam6d_hip import _lib
    lib = _lib.load()
    assert lib.sam6d_render_views_workspace_bytes(3, 17, 33) == 3 * 17 * 33 * 8
    assert lib.sam6d_render_views_workspace_bytes(1024, 2048, 2048) == 1 << 35
    for bad in ((0, 8, 8), (1025, 8, 8), (1, 0, 8), (1, 8, 2049)):
        assert lib.sam6d_render_views_workspace_bytes(*bad) == 0
    assert lib.sam6d_mesh_sample_workspace_bytes(0) == 0 and lib.sam6d_mesh_sample_workspace_bytes((1 << 24) + 1) == 0
    assert lib.sam6d_mesh_sample_workspace_bytes(1025) == 16 + 2 * 8 + 1025 * 12

    def render(T=1, H=8, W=8, F=1, V=3, near=1e-3, wave_area=0, ptr=64, ws=1 << 20):
        # (refused before a pointer is followed: 64 stands for "not null")
        _lib.call("sam6d_render_views", ptr, V, ptr, F, None, None, ptr, ptr, T, 1.0, 1.0, 0.0, 0.0, H, W, near, 0.05, 0, ptr, wave_area,
                  ptr, ptr, ptr, ptr, ptr, ptr, ptr, ws, None)

    for kw, name in ((dict(H=0), "H x W"), (dict(W=2049), "H x W"), (dict(T=0), "T = 0"), (dict(T=1025), "T = 1025"), (dict(F=0), "F = 0"),
                     (dict(F=(1 << 24) + 1), "F = 16777217"), (dict(V=0), "V = 0"), (dict(near=0.0), "near"), (dict(wave_area=-1), "wave_area"),
                     (dict(ptr=None), "null pointer"), (dict(ws=8 * 8 * 8 - 1), "workspace of 511 bytes"), (dict(ptr=68, ws=1 << 20), "aligned")):
        with pytest.raises(RuntimeError, match="render_views.*" + name):
            render(**kw)

    def sample(n=4, F=1, V=3, ptr=64, ws=1 << 20):
        _lib.call("sam6d_mesh_sample", ptr, V, ptr, F, n, 0, 0, ptr, ptr, ptr, ws, None)

    for kw, name in ((dict(n=0), "n = 0"), (dict(n=(1 << 24) + 1), "n = 16777217"), (dict(F=0), "F = 0"), (dict(F=(1 << 24) + 1), "F = 16777217"),
                     (dict(V=0), "V = 0"), (dict(ptr=None), "null pointer"), (dict(ws=35), "workspace of 35 bytes"), (dict(ptr=68), "aligned")):
        with pytest.raises(RuntimeError, match="mesh_sample.*" + name):
            sample(**kw)


# ------------------------------------------------------------------------------------------------------------ kernels
def test_kernel_resources():
    """none of the new kernels uses scratch or spills, and each keeps within its built VGPR count rounded up
    to the next step of 8 (built: raster_faces 62, raster_resolve 52, ms_area 18, ms_block_sum 9, ms_scan_blocks 14, ms_start 14,
    ms_sample 22).  The vector atomics are the 64-bit unsigned min of the z-buffer, the drop counter's add and area_max's unsigned max."""
    limits = dict(raster_faces_kernel=64, raster_resolve_kernel=56, ms_area_kernel=24, ms_block_sum_kernel=16, ms_scan_blocks_kernel=16,
                  ms_start_kernel=16, ms_sample_kernel=24)
    found, atomics = kernel_resources((b"raster_faces_kernel", b"ms_sample_kernel"), r"((?:raster|ms)_[a-z_]+_kernel)", disassemble=True)
    print("\n[onboard] (VGPRs, scratch bytes, spilled): %s; atomics %s" % (found, sorted(atomics)))
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
    assert atomics == {"global_atomic_umin_x2", "global_atomic_add", "global_atomic_umax"}, atomics
