// Template rendering of a TEXTURED model (Render/render_custom_templates.py:60: bproc.loader.load_obj takes an OBJ with its MTL and
// diffuse image, or a PLY that names a texture file): raster.hip's renderer with the albedo of rgb taken from one texture image.
// Visibility is raster.hip's pass (rs_visibility).  The resolve kernel below calls raster.h's rs_resolve_pixel, the function
// raster_resolve_kernel calls: it writes the background pixel, or mask, face, depth and xyz, and gives back the winner's weights and
// the lighting term v.  What is this file's own is the albedo; the tone step after it is raster.h's rs_tone again.  So a texture of one
// colour renders what the grey resolve renders with that albedo, bit for bit (tests/test_texture_gpu.py).  The recipe below is restated
// in numpy, float32 operation by operation, in tests/texture_ref.py; like the rest of the shading it is the package's own.
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
//   then    raster.hip's tone step (rs_tone): lin = albedo * v clamped to [0, 1] by comparisons, rgb = srgb_lut[(int)(lin * 4095 + 0.5)].
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
  RsHit h;
  if (!rs_resolve_pixel(i, vert, V, faces, view, cam, normals, light, zbuf, RsOut{mask, face_out, depth, xyz, rgb}, h)) return;
  // ---- the albedo (TEXTURE)
  const float* uv = tex.face_uv + (size_t)h.face * 6;
  const float ru = tx_wrap(rs_mix(h.l0, h.m1, h.m2, uv[0], uv[2], uv[4]));
  const float rv = tx_wrap(rs_mix(h.l0, h.m1, h.m2, uv[1], uv[3], uv[5]));
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
    rgb[i * 3 + k] = rs_tone((top + fy * (bot - top)) * h.v, srgb_lut);
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
