// Template rendering of a TEXTURED model (Render/render_custom_templates.py:60: bproc.loader.load_obj takes an OBJ with its MTL and
// diffuse image, or a PLY that names a texture file): raster.hip's renderer with the albedo of rgb taken from one texture image.
// Visibility is raster.hip's pass (rs_visibility), and the setup, coverage and weights are raster.h's device functions.  The resolve
// kernel below writes mask, face, depth, xyz and computes the lighting term v with raster_resolve_kernel's lines, repeated here and
// not called through a shared function: raster.hip's two kernels are pinned as built (tests/test_onboard_host.py), and moving those
// lines behind a wrapper both kernels call changed raster_resolve_kernel's code (50 -> 54 VGPRs).  The recipe below is restated in
// numpy, float32 operation by operation, in tests/texture_ref.py; like the rest of the shading it is the package's own.
//
// TEXTURE.  All float arithmetic is IEEE fp32 in the order written (the library is built with -ffp-contract=off and this file has no
// fused multiply-add); only + - * /, floorf and comparisons run on the device.
//   uv      (u, v) = (l0*a0 + m1*a1) + m2*a2 of the face's three stored-order corners of face_uv (F,3,2): perspective-correct, like
//           every attribute of raster.hip's RECIPE.
//   wrap    r = a - floorf(a);  r = (r >= 0 && r < 1) ? r : 0: the texture repeats; a NaN, an infinity and the rounding case r == 1
//           (a tiny negative a) give 0.
//   texel   tx = ru * (float)Wt - 0.5f;  ty = (1.0f - rv) * (float)Ht - 0.5f: texel (row j, column i) has its centre at
//           u = (i + 0.5) / Wt, v = 1 - (j + 0.5) / Ht, so v = 0 is the bottom edge of the image (row Ht - 1), as OBJ and PLY mean it.
//           x0f = floorf(tx), fx = tx - x0f, x0 = (int)x0f, x1 = x0 + 1;  x0 < 0 -> x0 + Wt;  x1 >= Wt -> x1 - Wt (the neighbour across
//           the border is the texel of the other side: repeat); the same for y with Ht.  All four indices are then clamped into the
//           image before anything is addressed.
//   value   a_ij[k] = texel_lut[byte k of texel (y_j, x_i)], k = 0, 1, 2.  The image is (Ht,Wt,4) u8, a texel one aligned 32-bit load
//           whose fourth byte is ignored; texel_lut is 256 f32 the host builds (k / 255 in fp32: the values the vertex-colour path
//           computes; or the sRGB-to-linear table).
//   filter  top = a00 + fx * (a10 - a00);  bot = a01 + fx * (a11 - a01);  albedo = top + fy * (bot - top), per channel (a_ij: column
//           x_i, row y_j).
//   then    raster.hip's lines: lin = albedo * v clamped to [0, 1] by comparisons, rgb = srgb_lut[(int)(lin * 4095 + 0.5)].
// There is no mip chain: a texture much finer than the rendered surface aliases (the host offers an exact box reduction at load).
//
// WORK.  One thread per pixel of every view, as raster_resolve_kernel; a covered pixel adds six loads of face_uv, four 4-byte loads of
// the image and twelve look-ups of the 1 KiB table to the untextured resolve.  The table is copied into LDS by every workgroup (one
// entry per thread): read from global memory, the twelve scattered loads cost more than the image's four (DESIGN, f16 measured).
#include "raster.h"
#include "../../include/sam6d_hip.h"

#define TX_MAX_SIDE 8192

struct TxImage {
  const float* face_uv;
  const unsigned* texels;  // (Ht, Wt) words: R, G, B in the low three bytes
  const float* lut;        // 256 albedos
  int Ht, Wt;
};

__device__ __forceinline__ float tx_wrap(float a) {
  const float r = a - floorf(a);
  return (r >= 0.f && r < 1.f) ? r : 0.f;
}

// the two taps of one axis of n texels at the texel coordinate t in [-0.5, n - 0.5] and the weight of the second: both indices in [0, n)
__device__ __forceinline__ void tx_taps(float t, int n, int& i0, int& i1, float& w) {
  const float f0 = floorf(t);
  w = t - f0;
  i0 = (int)f0;
  i1 = i0 + 1;
  if (i0 < 0) i0 += n;
  if (i1 >= n) i1 -= n;
  i0 = min(max(i0, 0), n - 1);
  i1 = min(max(i1, 0), n - 1);
}

// one thread per pixel of every view: the only writer of the outputs
__global__ __launch_bounds__(256) void textured_resolve_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                                               const float* __restrict__ view, RsCam cam, const float* normals,
                                                               const float* __restrict__ light, const unsigned char* __restrict__ srgb_lut,
                                                               TxImage tex, int T, const unsigned long long* __restrict__ zbuf,
                                                               unsigned char* __restrict__ mask, int* __restrict__ face_out,
                                                               float* __restrict__ depth, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
  // the byte -> albedo table in LDS, one entry per thread of the workgroup: a covered pixel looks it up twelve times
  __shared__ float albedo_of[256];
  albedo_of[threadIdx.x] = tex.lut[threadIdx.x];
  __syncthreads();
  const size_t hw = (size_t)cam.H * cam.W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw * (size_t)T) return;
  const int t = (int)(i / hw), p = (int)(i % hw), y = p / cam.W, x = p % cam.W;
  const unsigned long long key = zbuf[i];
  if (key == ~0ull) {
    mask[i] = 0;
    face_out[i] = -1;
    depth[i] = 0.f;
    xyz[i * 3] = xyz[i * 3 + 1] = xyz[i * 3 + 2] = 0.f;
    rgb[i * 3] = rgb[i * 3 + 1] = rgb[i * 3 + 2] = 0;
    return;
  }
  const int face = (int)(unsigned)(key & 0xffffffffull);
  const float* M = view + (size_t)t * 12;
  RsFace f;
  rs_setup(f, vert, V, faces, face, M, cam);
  long long w0, w1, w2;
  rs_cover(f, x, y, w0, w1, w2);
  float l0, l1, l2;
  const float d = rs_weights(f, w0, w1, w2, l0, l1, l2);
  // the weights in the face's stored order (a winding swap exchanged vertices 1 and 2): every attribute is mixed in that order
  const float m1 = f.swapped ? l2 : l1, m2 = f.swapped ? l1 : l2;
  const int* fv = faces + (size_t)face * 3;
  const float* a = vert + (size_t)fv[0] * 3;
  const float* b = vert + (size_t)fv[1] * 3;
  const float* c = vert + (size_t)fv[2] * 3;
  mask[i] = 255;
  face_out[i] = face;
  depth[i] = d;
#pragma unroll
  for (int k = 0; k < 3; ++k) xyz[i * 3 + k] = rs_mix(l0, m1, m2, a[k], b[k], c[k]);
  // ---- the lighting term v: raster_resolve_kernel's lines
  float P[3][3];  // camera-space vertices, stored order
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = vert + (size_t)fv[k] * 3;
    P[k][0] = rs_row(M, v[0], v[1], v[2]);
    P[k][1] = rs_row(M + 4, v[0], v[1], v[2]);
    P[k][2] = rs_row(M + 8, v[0], v[1], v[2]);
  }
  float Pc[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Pc[k] = rs_mix(l0, m1, m2, P[0][k], P[1][k], P[2][k]);
  if (normals) {
    float no[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) no[k] = rs_mix(l0, m1, m2, normals[(size_t)fv[0] * 3 + k], normals[(size_t)fv[1] * 3 + k], normals[(size_t)fv[2] * 3 + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (M[4 * k] * no[0] + M[4 * k + 1] * no[1]) + M[4 * k + 2] * no[2];
  } else {
    const float e1x = P[1][0] - P[0][0], e1y = P[1][1] - P[0][1], e1z = P[1][2] - P[0][2];
    const float e2x = P[2][0] - P[0][0], e2y = P[2][1] - P[0][1], e2z = P[2][2] - P[0][2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
  }
  const float facing = (n[0] * Pc[0] + n[1] * Pc[1]) + n[2] * Pc[2];
  if (facing > 0.f) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
  const float* lp = light + (size_t)t * 3;
  const float Lx = lp[0] - Pc[0], Ly = lp[1] - Pc[1], Lz = lp[2] - Pc[2];
  const float d2 = (Lx * Lx + Ly * Ly) + Lz * Lz;
  const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  const float ndl = (n[0] * Lx + n[1] * Ly) + n[2] * Lz;
  float cs = ndl / (sqrtf(nn) * sqrtf(d2));
  cs = cs > 0.f ? cs : 0.f;
  const float v = RS_GAIN * cs / d2;
  // ---- the albedo (TEXTURE)
  const float* uv = tex.face_uv + (size_t)face * 6;
  const float ru = tx_wrap(rs_mix(l0, m1, m2, uv[0], uv[2], uv[4]));
  const float rv = tx_wrap(rs_mix(l0, m1, m2, uv[1], uv[3], uv[5]));
  int x0, x1, y0, y1;
  float fx, fy;
  tx_taps(ru * (float)tex.Wt - 0.5f, tex.Wt, x0, x1, fx);
  tx_taps((1.0f - rv) * (float)tex.Ht - 0.5f, tex.Ht, y0, y1, fy);
  const unsigned* row0 = tex.texels + (size_t)y0 * tex.Wt;
  const unsigned* row1 = tex.texels + (size_t)y1 * tex.Wt;
  const unsigned t00 = row0[x0], t10 = row0[x1], t01 = row1[x0], t11 = row1[x1];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a00 = albedo_of[(t00 >> (8 * k)) & 255u], a10 = albedo_of[(t10 >> (8 * k)) & 255u];
    const float a01 = albedo_of[(t01 >> (8 * k)) & 255u], a11 = albedo_of[(t11 >> (8 * k)) & 255u];
    const float top = a00 + fx * (a10 - a00);
    const float bot = a01 + fx * (a11 - a01);
    float lin = (top + fy * (bot - top)) * v;
    lin = lin > 0.f ? lin : 0.f;
    lin = lin < 1.f ? lin : 1.f;
    rgb[i * 3 + k] = srgb_lut[(int)(lin * 4095.0f + 0.5f)];
  }
}

extern "C" int sam6d_render_views_textured(const float* vertices, int V, const int* faces, int F, const float* normals, const float* view,
                                           const float* light, int T, float fx, float fy, float cx, float cy, int H, int W, float near,
                                           float base_color, const unsigned char* srgb_lut, int wave_area, const float* face_uv,
                                           const unsigned char* texture, int Ht, int Wt, const float* texel_lut, unsigned char* mask,
                                           int* face, float* depth, float* xyz, unsigned char* rgb, int* n_dropped, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  (void)base_color;  // the untextured entry's grey albedo: kept in the argument list, nothing here is grey
  const int bad = rs_check("render_views_textured", V, F, T, H, W, near, wave_area,
                           vertices && faces && view && light && srgb_lut && face_uv && texture && texel_lut && mask && face && depth && xyz &&
                               rgb && n_dropped,
                           workspace, workspace_bytes);
  if (bad) return bad;
  SAM6D_REQUIRE(Ht >= 1 && Ht <= TX_MAX_SIDE && Wt >= 1 && Wt <= TX_MAX_SIDE, "render_views_textured: texture Ht x Wt = %d x %d is not in 1 .. %d",
                Ht, Wt, TX_MAX_SIDE);
  SAM6D_REQUIRE(((uintptr_t)texture & 3) == 0, "render_views_textured: texture is not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  const TxImage tex = {face_uv, (const unsigned*)texture, texel_lut, Ht, Wt};
  unsigned long long* zbuf = (unsigned long long*)workspace;
  const int err = rs_visibility("render_views_textured", vertices, V, faces, F, view, T, cam, wave_area, zbuf, n_dropped, s);
  if (err) return err;
  const size_t px = (size_t)T * H * W;  // at most 2^32: 2^24 blocks
  hipLaunchKernelGGL(textured_resolve_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, vertices, V, faces, view, cam, normals, light,
                     srgb_lut, tex, T, zbuf, mask, face, depth, xyz, rgb);
  SAM6D_LAUNCH_CHECK("render_views_textured (resolve)");
}
