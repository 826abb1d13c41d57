// The ViT-B/16 image encoder of PEM's feature extraction (PEM/model/feature_extraction.py:21-35 ViT.forward, :98-118 ViT_AE.forward,
// :141-142 get_img_feats, PEM/utils/model_utils.py:86-98 get_chosen_pixel_feats) around the library's GEMMs and attention:
//   patch rows  (B,3,224,224) -> A (B*196, 768) in the Conv2d weight's (c, kh, kw) order, plus the cls rows cls_token + pos_embed[0]
//               of the residual stream X (B*197, 768); the patch GEMM (sam6d_gemm_nt_w16) adds the conv bias and pos_embed[1:]
//   LayerNorm   over 768 channels (eps as given: 1e-6 for the ViT), rows addressed per image, so the same kernel writes the four
//               pyramid taps straight into the (B*196, 3072) concat buffer at column 768 j (the cls rows are skipped)
//   gather      output_upscaling output U (B*196, 4096) -> bilinear 56 -> 224 -> chosen pixels (B, N, 256): only the four taps of
//               each chosen pixel are read; the (B, 256, 224, 224) map is never formed
// The attention (sam6d_vit_attention) is the RPE self-attention kernel of xattn.hip in the ViT layout; the GELU of fc1 is the GEMM's
// act = 2 epilogue (gemm.hip).
//
// All three kernels here are memory-bound data movement (no MFMA).  Resource use (-Rpass-analysis=kernel-resource-usage, gfx950):
//   vit_patch_rows_kernel         11 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32: 12 us)
//   vit_layernorm768_kernel       54 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32: 8 us per launch, ~20 MB moved)
//   vit_upsample_gather_kernel    30 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32, N = 2048: 42 us)
//   sattn_kernel<true> (xattn.hip) 153 VGPRs, 0 spill, 118 848 B dynamic LDS, 1 workgroup / CU (B = 32: 384 workgroups, 40 us)
#include "common.h"
#include "../../include/sam6d_hip.h"

#define VIT_C 768
#define VIT_IMG 224
#define VIT_GRID 14
#define VIT_PATCHES 196
#define VIT_TOK 197

// ---- patch rows: workgroup (patch p, image b); p == 196 writes the image's cls row of X instead -------------------------------
__global__ __launch_bounds__(256) void vit_patch_rows_kernel(const float* __restrict__ img, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, float* __restrict__ A,
                                                             float* __restrict__ X) {
  const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (p == VIT_PATCHES) {
    float* dst = X + (size_t)b * VIT_TOK * VIT_C;
#pragma unroll
    for (int u = 0; u < 3; ++u) dst[t + 256 * u] = cls[t + 256 * u] + pos[t + 256 * u];
    return;
  }
  const int py = p / VIT_GRID, px = p % VIT_GRID;
  float* dst = A + ((size_t)b * VIT_PATCHES + p) * VIT_C;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int col = t + 256 * u, c = col >> 8, kh = (col >> 4) & 15, kw = col & 15;  // column = c * 256 + kh * 16 + kw
    dst[col] = img[(((size_t)b * 3 + c) * VIT_IMG + py * 16 + kh) * VIT_IMG + px * 16 + kw];
  }
}

extern "C" int sam6d_vit_patch_rows(const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B,
                                    void* stream) {
  SAM6D_REQUIRE(img && cls_token && pos_embed && A && X && B >= 0, "vit_patch_rows: null pointer");
  SAM6D_REQUIRE(B <= 65535, "vit_patch_rows: B <= 65535");
  if (B == 0) return 0;
  hipLaunchKernelGGL(vit_patch_rows_kernel, dim3(VIT_PATCHES + 1, B), dim3(256), 0, (hipStream_t)stream, img, cls_token, pos_embed, A,
                     X);
  SAM6D_LAUNCH_CHECK("vit_patch_rows");
}

// ---- LayerNorm over 768 channels: one wave per row, 12 floats per lane (three float4 at 4 lane + 256 u), two-pass mean / variance
// in registers.  Row r of image b: x + (b sx + r) ldx -> y + (b sy + r) ldy.
__global__ __launch_bounds__(256) void vit_layernorm768_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                               const float* __restrict__ be, float* __restrict__ y, long total,
                                                               int rows, long ldx, long sx, long ldy, long sy, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total) return;
  const int lane = threadIdx.x & 63;
  const long b = row / rows, r = row % rows;
  const float* src = x + b * sx + r * ldx;
  float* dst = y + b * sy + r * ldy;
  float4 v[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) v[u] = *reinterpret_cast<const float4*>(src + 4 * lane + 256 * u);
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 3; ++u) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  const float mean = wave_sum_dpp(s) * (1.0f / VIT_C);
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    v[u].x -= mean; v[u].y -= mean; v[u].z -= mean; v[u].w -= mean;
    q += (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
  }
  const float rstd = 1.0f / sqrtf(wave_sum_dpp(q) * (1.0f / VIT_C) + eps);
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const int c = 4 * lane + 256 * u;
    const float4 gg = *reinterpret_cast<const float4*>(g + c);
    const float4 bb = *reinterpret_cast<const float4*>(be + c);
    float4 o;
    o.x = v[u].x * rstd * gg.x + bb.x;
    o.y = v[u].y * rstd * gg.y + bb.y;
    o.z = v[u].z * rstd * gg.z + bb.z;
    o.w = v[u].w * rstd * gg.w + bb.w;
    *reinterpret_cast<float4*>(dst + c) = o;
  }
}

extern "C" int sam6d_vit_layernorm768(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx,
                                      long sx, long ldy, long sy, float eps, void* stream) {
  SAM6D_REQUIRE(x && gamma && beta && y, "vit_layernorm768: null pointer");
  SAM6D_REQUIRE(nimg >= 0 && rows >= 0 && ldx >= VIT_C && ldy >= VIT_C && sx >= 0 && sy >= 0, "vit_layernorm768: bad sizes");
  SAM6D_REQUIRE(((ldx | ldy | sx | sy) & 3) == 0 && ((((size_t)x) | ((size_t)y) | ((size_t)gamma) | ((size_t)beta)) & 15) == 0,
                "vit_layernorm768: strides must be multiples of 4 floats and pointers 16-byte aligned");
  const long total = (long)nimg * rows;
  if (total == 0) return 0;
  SAM6D_REQUIRE((total + 3) / 4 < 2147483647L, "vit_layernorm768: too many rows");
  hipLaunchKernelGGL(vit_layernorm768_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y,
                     total, rows, ldx, sx, ldy, sy, eps);
  SAM6D_LAUNCH_CHECK("vit_layernorm768");
}

// ---- output_upscaling -> bilinear (56 -> 224, align_corners = False) -> chosen pixels.
// The 56 x 56 map of channel c at cell (gy, gx) is U[14 (gy >> 2) + (gx >> 2)][((gy & 3) 4 + (gx & 3)) 256 + c] (the
// reshape(B,14,14,4,4,256).permute(0,5,1,3,2,4) of ViT_AE.forward).  Source index and weights as ATen's upsample_bilinear2d:
//   src = max(scale (dst + 0.5) - 0.5, 0) with scale = 56 / 224, i0 = (int) src, i1 = i0 + (i0 < 55), l1 = src - i0, l0 = 1 - l1,
//   out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).
// One wave per chosen pixel, four channels per lane: each tap is one contiguous 1 KiB row segment of U.  An index outside
// [0, 224 * 224) yields a NaN row (visible downstream without a host synchronisation).
__device__ __forceinline__ void vit_src_index(int d, int& i0, int& i1, float& l0, float& l1) {
  float s = 0.25f * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < 55 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.0f - l1;
}
__device__ __forceinline__ const float* vit_cell(const float* Ub, int gy, int gx) {
  return Ub + (size_t)(VIT_GRID * (gy >> 2) + (gx >> 2)) * 4096 + ((gy & 3) * 4 + (gx & 3)) * 256;
}

__global__ __launch_bounds__(256) void vit_upsample_gather_kernel(const float* __restrict__ U, const long long* __restrict__ choose,
                                                                  float* __restrict__ out, long total, int N) {
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= total) return;
  const int lane = threadIdx.x & 63;
  const long b = pix / N;
  const long long idx = choose[pix];
  float4* dst = reinterpret_cast<float4*>(out + pix * 256) + lane;
  if (idx < 0 || idx >= (long long)VIT_IMG * VIT_IMG) {
    const float nan = __builtin_nanf("");
    *dst = make_float4(nan, nan, nan, nan);
    return;
  }
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  vit_src_index((int)(idx / VIT_IMG), y0, y1, ly0, ly1);
  vit_src_index((int)(idx % VIT_IMG), x0, x1, lx0, lx1);
  const float* Ub = U + (size_t)b * VIT_PATCHES * 4096 + 4 * lane;
  const float4 v00 = *reinterpret_cast<const float4*>(vit_cell(Ub, y0, x0));
  const float4 v01 = *reinterpret_cast<const float4*>(vit_cell(Ub, y0, x1));
  const float4 v10 = *reinterpret_cast<const float4*>(vit_cell(Ub, y1, x0));
  const float4 v11 = *reinterpret_cast<const float4*>(vit_cell(Ub, y1, x1));
  auto bil = [&](float a, float bq, float c, float d) { return ly0 * (lx0 * a + lx1 * bq) + ly1 * (lx0 * c + lx1 * d); };
  *dst = make_float4(bil(v00.x, v01.x, v10.x, v11.x), bil(v00.y, v01.y, v10.y, v11.y), bil(v00.z, v01.z, v10.z, v11.z),
                     bil(v00.w, v01.w, v10.w, v11.w));
}

extern "C" int sam6d_vit_upsample_gather(const float* U, const long long* choose, float* out, int B, int N, void* stream) {
  SAM6D_REQUIRE(U && choose && out && B >= 0 && N >= 0, "vit_upsample_gather: null pointer");
  SAM6D_REQUIRE(((((size_t)U) | ((size_t)out)) & 15) == 0, "vit_upsample_gather: U and out must be 16-byte aligned");
  const long total = (long)B * N;
  if (total == 0) return 0;
  SAM6D_REQUIRE((total + 3) / 4 < 2147483647L, "vit_upsample_gather: too many pixels");
  hipLaunchKernelGGL(vit_upsample_gather_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, choose, out,
                     total, N);
  SAM6D_LAUNCH_CHECK("vit_upsample_gather");
}
