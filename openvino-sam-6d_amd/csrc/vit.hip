// The row kernels of the ViT encoders: what PEM's ViT-B/16 (PEM/model/feature_extraction.py:21-35 ViT.forward, :98-118 ViT_AE.forward,
// :141-142 get_img_feats, PEM/utils/model_utils.py:86-98 get_chosen_pixel_feats) and ISM's DINOv2 ViT-L/14 (dinov2.hip) run around the
// library's GEMMs and attention.  One template each, instantiated per encoder:
//   patch rows  (B,3,224,224) -> A (B*NP, KPAD): the 3 P P values of a patch in the Conv2d weight's (c, kh, kw) order, zeros from there
//               to KPAD (K padded to a multiple of the GEMM's 32-wide k-step: ViT-B 768 = 768, DINOv2 588 -> 608, the packed weight's
//               columns 588..607 are zero too), plus the cls rows cls_token + pos_embed[0] of the residual stream X (B*(NP+1), C); the
//               patch GEMM (sam6d_gemm_nt_w16) adds the conv bias and pos_embed[1:]
//   LayerNorm   over C = 768 or 1024 channels (eps as given: 1e-6 for both), rows addressed per image, so the same kernel writes the
//               four pyramid taps straight into the (B*196, 3072) concat buffer at column 768 j (the cls rows are skipped), and
//               DINOv2's x_norm_clstoken / x_norm_patchtokens into their own tensors
// and, for ViT-B alone:
//   gather      output_upscaling output U (B*196, 4096) -> bilinear 56 -> 224 -> chosen pixels (B, N, 256): only the four taps of
//               each chosen pixel are read; the (B, 256, 224, 224) map is never formed
// The attention (sam6d_vit_attention) is the RPE self-attention kernel of xattn.hip in the ViT layout; the GELU of fc1 is the GEMM's
// act = 2 epilogue (gemm.hip).
//
// All kernels here are memory-bound data movement (no MFMA).  Resource use (-Rpass-analysis=kernel-resource-usage, gfx950):
//   patch_rows_kernel<768, 16, 768>     8 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32: 12 us)
//   patch_rows_kernel<1024, 14, 608>   14 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD
//   rows_layernorm_kernel<768>        54 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32: 8 us per launch, ~20 MB moved)
//   rows_layernorm_kernel<1024>       60 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD
//   vit_upsample_gather_kernel        30 VGPRs, 0 spill, 0 B LDS, occupancy 8 waves / SIMD      (B = 32, N = 2048: 42 us)
//   sattn_kernel<true> (xattn.hip) 153 VGPRs, 0 spill, 118 848 B dynamic LDS, 1 workgroup / CU (B = 32: 384 workgroups, 40 us)
#include "common.h"
#include "../../include/sam6d_hip.h"

#define VIT_IMG 224
#define VIT_GRID 14
#define VIT_PATCHES 196

// ---- patch rows of an encoder of width C with P x P patches of an IMG x IMG image: workgroup (patch p, image b); with CLS, p == NP
// writes the image's cls row of X instead (SAM's encoder has no cls token: CLS = false, cls / pos / X unused) -----------------------
template <int C, int P, int KPAD, int IMG = VIT_IMG, bool CLS = true>
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ img, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, float* __restrict__ A, float* __restrict__ X) {
  constexpr int GRID = IMG / P, NP = GRID * GRID, K = 3 * P * P;
  static_assert(C % 256 == 0 && IMG % P == 0 && KPAD >= K, "patch_rows_kernel: bad instantiation");
  const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (CLS && p == NP) {
    float* dst = X + (size_t)b * (NP + 1) * C;
#pragma unroll
    for (int u = 0; u < C / 256; ++u) dst[t + 256 * u] = cls[t + 256 * u] + pos[t + 256 * u];
    return;
  }
  const int py = p / GRID, px = p % GRID;
  float* dst = A + ((size_t)b * NP + p) * KPAD;
  for (int col = t; col < KPAD; col += 256) {  // column = (c P + kh) P + kw
    float v = 0.f;
    if (col < K) {
      const int c = col / (P * P), k = col % (P * P), kh = k / P, kw = k % P;
      v = img[(((size_t)b * 3 + c) * IMG + py * P + kh) * IMG + px * P + kw];
    }
    dst[col] = v;
  }
}

template <int C, int P, int KPAD>
static int patch_rows(const char* name, const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B,
                      void* stream) {
  SAM6D_REQUIRE(img && cls_token && pos_embed && A && X && B >= 0, "%s: null pointer", name);
  SAM6D_REQUIRE(B <= 65535, "%s: B <= 65535", name);
  if (B == 0) return 0;
  constexpr int NP = (VIT_IMG / P) * (VIT_IMG / P);
  hipLaunchKernelGGL((patch_rows_kernel<C, P, KPAD>), dim3(NP + 1, B), dim3(256), 0, (hipStream_t)stream, img, cls_token, pos_embed, A,
                     X);
  SAM6D_LAUNCH_CHECK(name);
}

extern "C" int sam6d_vit_patch_rows(const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B,
                                    void* stream) {
  return patch_rows<768, 16, 768>("vit_patch_rows", img, cls_token, pos_embed, A, X, B, stream);
}
extern "C" int sam6d_dino_patch_rows(const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B,
                                     void* stream) {
  return patch_rows<1024, 14, 608>("dino_patch_rows", img, cls_token, pos_embed, A, X, B, stream);
}

// ---- LayerNorm over C channels: one wave per row, C / 64 floats per lane (C / 256 float4 at 4 lane + 256 u), two-pass mean / variance
// in registers.  Row r of image b: x + b sx + r ldx -> y + b sy + r ldy, in floats.
template <int C>
__global__ __launch_bounds__(256) void rows_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ be, float* __restrict__ y, long total, int rows,
                                                             long ldx, long sx, long ldy, long sy, float eps) {
  constexpr int U = C / 256;
  static_assert(C % 256 == 0, "rows_layernorm_kernel: C must be a multiple of 256");
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total) return;
  const int lane = threadIdx.x & 63;
  const long b = row / rows, r = row % rows;
  const float* src = x + b * sx + r * ldx;
  float* dst = y + b * sy + r * ldy;
  float4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const float4*>(src + 4 * lane + 256 * u);
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  const float mean = wave_sum_dpp(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    v[u].x -= mean; v[u].y -= mean; v[u].z -= mean; v[u].w -= mean;
    q += (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
  }
  const float rstd = 1.0f / sqrtf(wave_sum_dpp(q) * (1.0f / C) + eps);
#pragma unroll
  for (int u = 0; u < U; ++u) {
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

template <int C>
static int rows_layernorm(const char* name, const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx,
                          long sx, long ldy, long sy, float eps, void* stream) {
  SAM6D_REQUIRE(x && gamma && beta && y, "%s: null pointer", name);
  SAM6D_REQUIRE(nimg >= 0 && rows >= 0 && ldx >= C && ldy >= C && sx >= 0 && sy >= 0, "%s: bad sizes", name);
  SAM6D_REQUIRE(((ldx | ldy | sx | sy) & 3) == 0 && ((((size_t)x) | ((size_t)y) | ((size_t)gamma) | ((size_t)beta)) & 15) == 0,
                "%s: strides must be multiples of 4 floats and pointers 16-byte aligned", name);
  const long total = (long)nimg * rows;
  if (total == 0) return 0;
  SAM6D_REQUIRE((total + 3) / 4 < 2147483647L, "%s: too many rows", name);
  hipLaunchKernelGGL(rows_layernorm_kernel<C>, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y,
                     total, rows, ldx, sx, ldy, sy, eps);
  SAM6D_LAUNCH_CHECK(name);
}

// SAM ViT-H: 1024 x 1024 image, 64 x 64 patches of 16 x 16, no cls row (pos_embed is the patch GEMM's residual)
extern "C" int sam6d_sam_patch_rows(const float* img, float* A, int B, void* stream) {
  SAM6D_REQUIRE(img && A && B >= 0, "sam_patch_rows: null pointer");
  SAM6D_REQUIRE(B <= 65535, "sam_patch_rows: B <= 65535");
  if (B == 0) return 0;
  hipLaunchKernelGGL((patch_rows_kernel<1280, 16, 768, 1024, false>), dim3(4096, B), dim3(256), 0, (hipStream_t)stream, img,
                     (const float*)nullptr, (const float*)nullptr, A, (float*)nullptr);
  SAM6D_LAUNCH_CHECK("sam_patch_rows");
}

extern "C" int sam6d_vit_layernorm768(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx,
                                      long sx, long ldy, long sy, float eps, void* stream) {
  return rows_layernorm<768>("vit_layernorm768", x, gamma, beta, y, nimg, rows, ldx, sx, ldy, sy, eps, stream);
}
extern "C" int sam6d_dino_layernorm1024(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx,
                                        long sx, long ldy, long sy, float eps, void* stream) {
  return rows_layernorm<1024>("dino_layernorm1024", x, gamma, beta, y, nimg, rows, ldx, sx, ldy, sy, eps, stream);
}

extern "C" int sam6d_sam_layernorm1280(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx,
                                       long sx, long ldy, long sy, float eps, void* stream) {
  return rows_layernorm<1280>("sam_layernorm1280", x, gamma, beta, y, nimg, rows, ldx, sx, ldy, sy, eps, stream);
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
