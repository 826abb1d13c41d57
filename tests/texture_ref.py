"""Numpy restatement of the textured resolve (csrc/texture.hip, sam6d_hip.onboard.render_views with face_uv and texture), code of its
own: the TEXTURE paragraph at the top of texture.hip, float32 operation by operation in the order written there, on top of the
geometry of tests/raster_ref.py (its Setup, edge functions, weights and _mix are imported; visibility, mask, face, depth and xyz are
raster_ref.render_view's own outputs, and the lighting term v restates raster.hip's shading paragraph as raster_ref does).

    (u, v) = (l0*a0 + m1*a1) + m2*a2 of the face's stored-order corners
    r      = a - floor(a);  r = r if (r >= 0 and r < 1) else 0
    tx     = ru * float(Wt) - 0.5;  ty = (1 - rv) * float(Ht) - 0.5
    x0     = int(floor(tx)), fx = tx - floor(tx), x1 = x0 + 1;  x0 < 0 -> x0 + Wt;  x1 >= Wt -> x1 - Wt;  clamp;  the same for y
    a_ij   = texel_lut[byte of texel (y_j, x_i)]
    albedo = top + fy * (bot - top), top = a00 + fx * (a10 - a00), bot = a01 + fx * (a11 - a01)
"""
import numpy as np

from tests import raster_ref as RR

F32 = np.float32


def wrap(a):
    with np.errstate(all="ignore"):
        r = a - np.floor(a)
    return np.where((r >= 0) & (r < 1), r, F32(0)).astype(F32)


def taps(t, n):
    """the two texel indices of one axis of n texels at the texel coordinate t, and the weight of the second"""
    f0 = np.floor(t)
    w = t - f0
    i0 = f0.astype(np.int64)
    i1 = i0 + 1
    i0 = np.where(i0 < 0, i0 + n, i0)
    i1 = np.where(i1 >= n, i1 - n, i1)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w


def lookup(u, v, texture, texel_lut):
    """albedo (n,3) f32 of the interpolated coordinates u, v (n) f32"""
    texture = np.asarray(texture, np.uint8)
    lut = np.asarray(texel_lut, F32)
    Ht, Wt = texture.shape[:2]
    ru, rv = wrap(u), wrap(v)
    x0, x1, fx = taps(ru * F32(Wt) - F32(0.5), Wt)
    y0, y1, fy = taps((F32(1.0) - rv) * F32(Ht) - F32(0.5), Ht)
    out = np.empty((len(ru), 3), F32)
    for k in range(3):
        a00, a10 = lut[texture[y0, x0, k]], lut[texture[y0, x1, k]]
        a01, a11 = lut[texture[y1, x0, k]], lut[texture[y1, x1, k]]
        top = a00 + fx * (a10 - a00)
        bot = a01 + fx * (a11 - a01)
        out[:, k] = top + fy * (bot - top)
    assert all(a.dtype == F32 for a in (ru, rv, fx, fy, out))
    return out


def render_view(vert, faces, normals, face_uv, texture, texel_lut, M, light, fx, fy, cx, cy, H, W, near, lut):
    vert = np.asarray(vert, F32)
    faces = np.asarray(faces, np.int64)
    M = np.asarray(M, F32).reshape(3, 4)
    face_uv = np.asarray(face_uv, F32)
    # the geometry: raster_ref's (its rgb, the grey render, is replaced below)
    out = RR.render_view(vert, faces, normals, None, M, light, fx, fy, cx, cy, H, W, near, 0.05, False, lut)
    out["rgb"] = np.zeros((H, W, 3), np.uint8)
    out["albedo"] = np.zeros((H, W, 3), F32)
    out["uv"] = np.zeros((H, W, 2), F32)
    ys, xs = np.nonzero(out["mask"])
    if ys.size == 0:
        return out
    s = RR.Setup(vert, faces, M, fx, fy, cx, cy, near, H, W)
    f = out["face"][ys, xs].astype(np.int64)
    _, l = s.weights(f, s.edges(f, 256 * xs + 128, 256 * ys + 128))
    sw = s.swapped[f]
    m = [l[0], np.where(sw, l[2], l[1]), np.where(sw, l[1], l[2])]  # the stored vertex order
    fv = faces[f]
    # ---- the lighting term v (raster.hip, shading)
    P = s.P[f]
    Pc = [RR._mix(m, P[:, 0, k], P[:, 1, k], P[:, 2, k]) for k in range(3)]
    if normals is not None:
        normals = np.asarray(normals, F32)
        no = [RR._mix(m, normals[fv[:, 0], k], normals[fv[:, 1], k], normals[fv[:, 2], k]) for k in range(3)]
        n = [(M[k, 0] * no[0] + M[k, 1] * no[1]) + M[k, 2] * no[2] for k in range(3)]
    else:
        e1 = [P[:, 1, k] - P[:, 0, k] for k in range(3)]
        e2 = [P[:, 2, k] - P[:, 0, k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    facing = (n[0] * Pc[0] + n[1] * Pc[1]) + n[2] * Pc[2]
    n = [np.where(facing > 0, -c, c) for c in n]
    light = np.asarray(light, F32)
    L = [light[k] - Pc[k] for k in range(3)]
    d2 = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    ndl = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]
    with np.errstate(all="ignore"):
        cs = ndl / (np.sqrt(nn) * np.sqrt(d2))
        cs = np.where(cs > 0, cs, F32(0))
        v = RR.GAIN * cs / d2
    # ---- the albedo (texture.hip, TEXTURE)
    uv = face_uv[f]  # (n, corner, 2)
    with np.errstate(all="ignore"):
        tu = RR._mix(m, uv[:, 0, 0], uv[:, 1, 0], uv[:, 2, 0])
        tv = RR._mix(m, uv[:, 0, 1], uv[:, 1, 1], uv[:, 2, 1])
    alb = lookup(tu, tv, texture, texel_lut)
    out["uv"][ys, xs] = np.stack([tu, tv], axis=1)
    out["albedo"][ys, xs] = alb
    for k in range(3):
        with np.errstate(all="ignore"):
            lin = alb[:, k] * v
        lin = np.where(lin > 0, lin, F32(0))
        lin = np.where(lin < 1, lin, F32(1))
        out["rgb"][ys, xs, k] = np.asarray(lut)[(lin * F32(4095) + F32(0.5)).astype(np.int64)]
    assert all(a.dtype == F32 for a in (v, tu, tv, alb))
    return out


def render(vert, faces, normals, face_uv, texture, texel_lut, view, light, intrinsics, size, near, lut):
    """T views: the dict of sam6d_hip.onboard.render_views(..., face_uv=, texture=) in numpy, plus albedo (T,H,W,3) f32 and the
    interpolated coordinates uv (T,H,W,2) f32 before the wrap"""
    fx, fy, cx, cy = intrinsics
    H, W = size
    per = [render_view(vert, faces, normals, face_uv, texture, texel_lut, view[t], light[t], fx, fy, cx, cy, H, W, near, lut)
           for t in range(len(view))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}
