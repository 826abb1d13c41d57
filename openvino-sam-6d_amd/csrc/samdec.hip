// SAM's mask decoder for point prompts (ISM/segment_anything/modeling/mask_decoder.py:112-149 with the TwoWayTransformer of
// modeling/transformer.py:62-106, 151-182): the three places where the decoder touches all P x 4096 image rows.
//
// The kernels are specialised: transformer_dim 256, 8 heads, cross attention downsampled to 128 channels (16 per head), T = 7 tokens
// per prompt (iou, 4 mask tokens, the point, the padding point), a 64 x 64 embedding grid.  P is a run-time value.  The dense
// projections over the image rows (k / v / q of the cross attentions, ConvTranspose 1) are sam6d_gemm_nt(_w16) launches issued by
// sam6d_hip/samdec.py, several of them merged into one GEMM per pass over the keys and the `pe` parts added as per-image tables in
// the GEMM epilogue; these kernels do what lies between the GEMMs and keep it on chip:
//   samdec_i2t_kernel      image -> token attention: 8 x 7 scores, softmax over the 7 tokens, the 56 -> 256 contraction against the
//                          prompt's folded out_proj table, + bias + keys, norm4, one write of the new keys
//   samdec_t2i_kernel      token -> image attention, the 4096 keys split over 32 workgroups per prompt, + samdec_t2i_combine_kernel
//   samdec_upscale_kernel  LayerNorm2d + GELU + ConvTranspose 2 + GELU + the product with hyper_in[1:4], one write of the logits
// All arithmetic here is fp32 spelled as scalar fmaf, in both matmul modes (the modes apply to the GEMMs).
#include "common.h"
#include "../../include/sam6d_hip.h"

#define SD_C 256      // transformer_dim
#define SD_CI 128     // internal width of the cross attentions (downsample_rate 2)
#define SD_H 8        // heads
#define SD_D 16       // channels per head of the cross attentions
#define SD_T 7        // tokens per prompt
#define SD_TH 56      // (token, head) pairs; pair i = 8 j + h
#define SD_N 4096     // image tokens (64 x 64)
#define SD_G 64       // grid side
#define SD_SPLITS 32  // key ranges of the token -> image attention
#define SD_KEYS 128   // keys per range

static bool samdec_shape_ok(int dim, int heads, int tokens, int grid_h, int grid_w) {
  return dim == SD_C && heads == SD_H && tokens == SD_T && grid_h == SD_G && grid_w == SD_G;
}
#define SAMDEC_REQUIRE_SHAPE(name)                                                                                                   \
  SAM6D_REQUIRE(samdec_shape_ok(dim, heads, tokens, grid_h, grid_w),                                                                 \
                name ": built for transformer_dim 256, 8 heads, 7 tokens and a 64 x 64 grid (got dim %d, heads %d, tokens %d, grid %d x %d)", \
                dim, heads, tokens, grid_h, grid_w)

__device__ __forceinline__ float dot16(const f32x4 a0, const f32x4 a1, const f32x4 a2, const f32x4 a3, const float* __restrict__ b) {
  float s = a0[0] * b[0];
  s = fmaf(a0[1], b[1], s);
  s = fmaf(a0[2], b[2], s);
  s = fmaf(a0[3], b[3], s);
  s = fmaf(a1[0], b[4], s);
  s = fmaf(a1[1], b[5], s);
  s = fmaf(a1[2], b[6], s);
  s = fmaf(a1[3], b[7], s);
  s = fmaf(a2[0], b[8], s);
  s = fmaf(a2[1], b[9], s);
  s = fmaf(a2[2], b[10], s);
  s = fmaf(a2[3], b[11], s);
  s = fmaf(a3[0], b[12], s);
  s = fmaf(a3[1], b[13], s);
  s = fmaf(a3[2], b[14], s);
  s = fmaf(a3[3], b[15], s);
  return s;
}

__device__ __forceinline__ float tree_sum64(const float* v) {
  float s[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) s[i] = v[2 * i] + v[2 * i + 1];
#pragma unroll
  for (int n = 16; n >= 1; n >>= 1)
#pragma unroll
    for (int i = 0; i < n; ++i) s[i] = s[2 * i] + s[2 * i + 1];
  return s[0];
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- image -> token attention, out_proj folded, residual and norm4 --------------------------------------------------------------------
// Workgroup = (128 image tokens, prompt), 256 threads, four passes of 32 tokens.  Thread c keeps column c of the prompt's folded table
// (56 floats) in registers for all four passes.  Per pass: thread (token, head) forms the head's 7 scores and their softmax -> LDS;
// thread c contracts each token's 56 probabilities with its column, adds bias and the old key, -> LDS; a wave normalises 8 tokens.
#define I2T_TOK 32
#define I2T_PASSES 4
__global__ __launch_bounds__(256) void samdec_i2t_kernel(const float* __restrict__ q, long ldq, long sq, const float* __restrict__ ktok,
                                                         const float* __restrict__ fold, const float* __restrict__ bias,
                                                         const float* __restrict__ keys, long skeys, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float kt[SD_T * SD_CI];
  __shared__ __attribute__((aligned(16))) float pr[I2T_TOK][SD_TH];
  __shared__ __attribute__((aligned(16))) float xs[I2T_TOK][SD_C];
  const int p = blockIdx.y, t = threadIdx.x;
  for (int i = t; i < SD_T * SD_CI; i += 256) kt[i] = ktok[(size_t)p * SD_T * SD_CI + i];
  float f[SD_TH];
#pragma unroll
  for (int i = 0; i < SD_TH; ++i) f[i] = fold[((size_t)p * SD_TH + i) * SD_C + t];
  const float bo = bias[t];
  const int lane = t & 63, wv = t >> 6;
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + 4 * lane), b4 = *reinterpret_cast<const f32x4*>(beta + 4 * lane);
  __syncthreads();
  for (int pass = 0; pass < I2T_PASSES; ++pass) {
    const int tok0 = blockIdx.x * (I2T_TOK * I2T_PASSES) + pass * I2T_TOK;
    {
      const int tt = t >> 3, h = t & 7;
      const f32x4* qr = reinterpret_cast<const f32x4*>(q + (size_t)p * sq + (size_t)(tok0 + tt) * ldq + SD_D * h);
      const f32x4 q0 = qr[0], q1 = qr[1], q2 = qr[2], q3 = qr[3];
      float s[SD_T], m = -INFINITY;
#pragma unroll
      for (int j = 0; j < SD_T; ++j) {
        s[j] = dot16(q0, q1, q2, q3, &kt[j * SD_CI + SD_D * h]) * 0.25f;  // / sqrt(16)
        m = fmaxf(m, s[j]);
      }
      float l = 0.f;
#pragma unroll
      for (int j = 0; j < SD_T; ++j) {
        s[j] = expf(s[j] - m);
        l += s[j];
      }
#pragma unroll
      for (int j = 0; j < SD_T; ++j) pr[tt][j * SD_H + h] = s[j] / l;
    }
    __syncthreads();
    for (int tt = 0; tt < I2T_TOK; ++tt) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < SD_TH; i += 4) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(&pr[tt][i]);
        a = fmaf(pv[0], f[i], a);
        a = fmaf(pv[1], f[i + 1], a);
        a = fmaf(pv[2], f[i + 2], a);
        a = fmaf(pv[3], f[i + 3], a);
      }
      xs[tt][t] = keys[(size_t)p * skeys + (size_t)(tok0 + tt) * SD_C + t] + (a + bo);
    }
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < I2T_TOK / 4; ++r) {
      const int tt = wv * (I2T_TOK / 4) + r;
      const f32x4 x = *reinterpret_cast<const f32x4*>(&xs[tt][4 * lane]);
      const float mean = wave_sum((x[0] + x[1]) + (x[2] + x[3])) * (1.0f / SD_C);
      const float d0 = x[0] - mean, d1 = x[1] - mean, d2 = x[2] - mean, d3 = x[3] - mean;
      const float var = wave_sum(fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3)) * (1.0f / SD_C);
      const float rs = 1.0f / sqrtf(var + eps);
      f32x4 y;
      y[0] = fmaf(d0 * rs, g4[0], b4[0]);
      y[1] = fmaf(d1 * rs, g4[1], b4[1]);
      y[2] = fmaf(d2 * rs, g4[2], b4[2]);
      y[3] = fmaf(d3 * rs, g4[3], b4[3]);
      *reinterpret_cast<f32x4*>(out + ((size_t)p * SD_N + tok0 + tt) * SD_C + 4 * lane) = y;
    }
    // the next pass writes pr before its first barrier and xs only after it: both are free by then
  }
}

extern "C" int sam6d_samdec_image_to_token(const float* q, long ldq, long sq, const float* ktok, const float* fold, const float* bias,
                                           const float* keys, long skeys, const float* gamma, const float* beta, float eps, float* out,
                                           int P, int dim, int heads, int tokens, int grid_h, int grid_w, void* stream) {
  SAMDEC_REQUIRE_SHAPE("samdec_image_to_token");
  SAM6D_REQUIRE(P >= 0 && P <= 65535, "samdec_image_to_token: 0 <= P <= 65535 (got %d)", P);
  if (P == 0) return 0;
  SAM6D_REQUIRE(q && ktok && fold && bias && keys && gamma && beta && out, "samdec_image_to_token: null pointer");
  SAM6D_REQUIRE(ldq >= SD_CI && (ldq & 3) == 0 && (sq & 3) == 0 && sq >= 0 && skeys >= 0 && (((uintptr_t)q | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0,
                "samdec_image_to_token: q rows must be 16-byte aligned (ldq %ld, prompt stride %ld)", ldq, sq);
  SAM6D_REQUIRE(sq == 0 || sq >= (long)SD_N * ldq - (ldq - SD_CI), "samdec_image_to_token: prompt stride of q smaller than one prompt");
  SAM6D_REQUIRE(skeys == 0 || skeys >= (long)SD_N * SD_C, "samdec_image_to_token: prompt stride of keys smaller than one prompt");
  hipLaunchKernelGGL(samdec_i2t_kernel, dim3(SD_N / (I2T_TOK * I2T_PASSES), P), dim3(256), 0, (hipStream_t)stream, q, ldq, sq, ktok, fold, bias,
                     keys, skeys, gamma, beta, eps, out);
  SAM6D_LAUNCH_CHECK("samdec_image_to_token");
}

// ---- token -> image attention ------------------------------------------------------------------------------------------------------------
// Workgroup = (range of 128 keys, prompt), 256 threads.  Scores of the range's keys for the 56 (token, head) pairs -> LDS; per pair the
// range's maximum and exp-sum (a wave per pair); thread (channel, half of the range) accumulates its half's weighted v; the halves are
// added in LDS.  Partial (max, sum, weighted v) per range go to the workspace; samdec_t2i_combine_kernel merges the 32 ranges of a prompt.
__global__ __launch_bounds__(256) void samdec_t2i_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                         long ld, long skv, float* __restrict__ pm, float* __restrict__ pl,
                                                         float* __restrict__ po) {
  __shared__ __attribute__((aligned(16))) float qs[SD_T * SD_CI];
  __shared__ float sc[SD_TH][SD_KEYS + 1];
  __shared__ float half1[SD_T][SD_CI];
  const int p = blockIdx.y, split = blockIdx.x, t = threadIdx.x;
  const size_t row0 = (size_t)p * skv + (size_t)split * SD_KEYS * ld;
  for (int i = t; i < SD_T * SD_CI; i += 256) qs[i] = q[(size_t)p * SD_T * SD_CI + i];
  __syncthreads();
  {
    const int key = t & (SD_KEYS - 1), hh = t >> 7;
    const f32x4* kr = reinterpret_cast<const f32x4*>(k + row0 + (size_t)key * ld + 64 * hh);
#pragma unroll
    for (int h4 = 0; h4 < 4; ++h4) {
      const f32x4 k0 = kr[4 * h4], k1 = kr[4 * h4 + 1], k2 = kr[4 * h4 + 2], k3 = kr[4 * h4 + 3];
      const int h = 4 * hh + h4;
#pragma unroll
      for (int j = 0; j < SD_T; ++j) sc[j * SD_H + h][key] = dot16(k0, k1, k2, k3, &qs[j * SD_CI + SD_D * h]) * 0.25f;
    }
  }
  __syncthreads();
  {
    const int lane = t & 63, wv = t >> 6;
    const size_t pbase = ((size_t)p * SD_SPLITS + split) * SD_TH;
    for (int i = wv; i < SD_TH; i += 4) {
      const float s0 = sc[i][lane], s1 = sc[i][lane + 64];
      const float m = wave_max(fmaxf(s0, s1));
      const float e0 = expf(s0 - m), e1 = expf(s1 - m);
      const float l = wave_sum(e0 + e1);
      sc[i][lane] = e0;
      sc[i][lane + 64] = e1;
      if (lane == 0) {
        pm[pbase + i] = m;
        pl[pbase + i] = l;
      }
    }
  }
  __syncthreads();
  {
    const int c = t & (SD_CI - 1), half = t >> 7, h = c >> 4;
    float acc[SD_T];
#pragma unroll
    for (int j = 0; j < SD_T; ++j) acc[j] = 0.f;
    const float* vr = v + row0 + (size_t)(half * 64) * ld + c;
    for (int kk = 0; kk < 64; ++kk) {
      const float vv = vr[(size_t)kk * ld];
#pragma unroll
      for (int j = 0; j < SD_T; ++j) acc[j] = fmaf(sc[j * SD_H + h][half * 64 + kk], vv, acc[j]);
    }
    if (half == 1) {
#pragma unroll
      for (int j = 0; j < SD_T; ++j) half1[j][c] = acc[j];
    }
    __syncthreads();
    if (half == 0) {
      float* o = po + ((size_t)p * SD_SPLITS + split) * SD_T * SD_CI;
#pragma unroll
      for (int j = 0; j < SD_T; ++j) o[j * SD_CI + c] = acc[j] + half1[j][c];
    }
  }
}

__global__ __launch_bounds__(SD_CI) void samdec_t2i_combine_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                                   const float* __restrict__ po, float* __restrict__ out) {
  const int p = blockIdx.x, c = threadIdx.x, h = c >> 4;
  for (int j = 0; j < SD_T; ++j) {
    const int i = j * SD_H + h;
    const float* m = pm + (size_t)p * SD_SPLITS * SD_TH + i;
    const float* l = pl + (size_t)p * SD_SPLITS * SD_TH + i;
    float mx = -INFINITY;
    for (int s = 0; s < SD_SPLITS; ++s) mx = fmaxf(mx, m[s * SD_TH]);
    float num = 0.f, den = 0.f;
    for (int s = 0; s < SD_SPLITS; ++s) {
      const float w = expf(m[s * SD_TH] - mx);
      num = fmaf(w, po[(((size_t)p * SD_SPLITS + s) * SD_T + j) * SD_CI + c], num);
      den = fmaf(w, l[s * SD_TH], den);
    }
    out[((size_t)p * SD_T + j) * SD_CI + c] = num / den;
  }
}

extern "C" size_t sam6d_samdec_token_to_image_workspace_bytes(int P) {
  if (P <= 0 || P > 65535) return 0;
  return (size_t)P * SD_SPLITS * (2 * SD_TH + SD_T * SD_CI) * sizeof(float);
}

extern "C" int sam6d_samdec_token_to_image(const float* q, const float* k, const float* v, long ld, long skv, float* out, int P, int dim,
                                           int heads, int tokens, int grid_h, int grid_w, void* ws, size_t ws_bytes, void* stream) {
  SAMDEC_REQUIRE_SHAPE("samdec_token_to_image");
  SAM6D_REQUIRE(P >= 0 && P <= 65535, "samdec_token_to_image: 0 <= P <= 65535 (got %d)", P);
  if (P == 0) return 0;
  SAM6D_REQUIRE(q && k && v && out && ws, "samdec_token_to_image: null pointer");
  SAM6D_REQUIRE(ld >= SD_CI && (ld & 3) == 0 && (skv & 3) == 0 && skv >= 0 && ((uintptr_t)k & 15) == 0,
                "samdec_token_to_image: k rows must be 16-byte aligned (ld %ld, prompt stride %ld)", ld, skv);
  SAM6D_REQUIRE(skv == 0 || skv >= (long)SD_N * ld - (ld - SD_CI), "samdec_token_to_image: prompt stride of k / v smaller than one prompt");
  SAM6D_REQUIRE(ws_bytes >= sam6d_samdec_token_to_image_workspace_bytes(P), "samdec_token_to_image: workspace too small");
  float* pm = (float*)ws;
  float* pl = pm + (size_t)P * SD_SPLITS * SD_TH;
  float* po = pl + (size_t)P * SD_SPLITS * SD_TH;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(samdec_t2i_kernel, dim3(SD_SPLITS, P), dim3(256), 0, s, q, k, v, ld, skv, pm, pl, po);
  SAM6D_LAUNCH_CHECK_CONT("samdec_token_to_image");
  hipLaunchKernelGGL(samdec_t2i_combine_kernel, dim3(P), dim3(SD_CI), 0, s, pm, pl, po, out);
  SAM6D_LAUNCH_CHECK("samdec_token_to_image");
}

// ---- output_upscaling after ConvTranspose 1, and the mask product --------------------------------------------------------------------------
// One thread per (image token, sub-pixel of ConvTranspose 1): its 64 channels stay in registers through LayerNorm2d and GELU; the
// 64 -> 4 x 32 weights of ConvTranspose 2 are the same for every lane (uniform loads); each of the 128 outputs goes through GELU and
// into the three dot products with hyper_in[1:4] at once, so a thread ends with 4 pixels x 3 masks and writes nothing else.
#define UP_C1 64  // channels after ConvTranspose 1
#define UP_C2 32  // channels after ConvTranspose 2
__global__ __launch_bounds__(256) void samdec_upscale_kernel(const float* __restrict__ ct1, long ld, long sp, const float* __restrict__ ln_g,
                                                             const float* __restrict__ ln_b, float eps, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, const float* __restrict__ hyper,
                                                             float* __restrict__ low) {
  __shared__ float hy[3 * UP_C2];
  const int p = blockIdx.y, t = threadIdx.x;
  if (t < 3 * UP_C2) hy[t] = hyper[(size_t)p * 3 * UP_C2 + t];
  __syncthreads();
  const int row = blockIdx.x * 256 + t;  // 4 token + sub-pixel
  const int tok = row >> 2, s1 = row & 3;
  const f32x4* xr = reinterpret_cast<const f32x4*>(ct1 + (size_t)p * sp + (size_t)tok * ld + UP_C1 * s1);
  float x[UP_C1];
#pragma unroll
  for (int i = 0; i < UP_C1 / 4; ++i) {
    const f32x4 v = xr[i];
    x[4 * i] = v[0];
    x[4 * i + 1] = v[1];
    x[4 * i + 2] = v[2];
    x[4 * i + 3] = v[3];
  }
  // pairwise sums (the same 63 additions as a chain, 6 roundings deep instead of 63): with almost no spread over the channels the
  // mean's rounding error is measured against the spread, not against the values
  const float mean = tree_sum64(x) * (1.0f / UP_C1);
  float sq[UP_C1];
#pragma unroll
  for (int i = 0; i < UP_C1; ++i) {
    x[i] -= mean;
    sq[i] = x[i] * x[i];
  }
  const float rs = 1.0f / sqrtf(tree_sum64(sq) * (1.0f / UP_C1) + eps);
#pragma unroll
  for (int i = 0; i < UP_C1; ++i) x[i] = gelu_erf(fmaf(x[i] * rs, ln_g[i], ln_b[i]));
  const int ty = tok >> 6, tx = tok & 63;
  const int py = 4 * ty + 2 * (s1 >> 1), px = 4 * tx + 2 * (s1 & 1);
  float* lp = low + (size_t)p * 3 * (4 * SD_G) * (4 * SD_G);
  for (int s2 = 0; s2 < 4; ++s2) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int o = 0; o < UP_C2; ++o) {
      const float* w = w2 + (size_t)(s2 * UP_C2 + o) * UP_C1;
      float a = b2[s2 * UP_C2 + o];
#pragma unroll
      for (int i = 0; i < UP_C1; ++i) a = fmaf(x[i], w[i], a);
      a = gelu_erf(a);
      m0 = fmaf(hy[o], a, m0);
      m1 = fmaf(hy[UP_C2 + o], a, m1);
      m2 = fmaf(hy[2 * UP_C2 + o], a, m2);
    }
    const size_t at = (size_t)(py + (s2 >> 1)) * (4 * SD_G) + px + (s2 & 1);
    lp[at] = m0;
    lp[(size_t)(4 * SD_G) * (4 * SD_G) + at] = m1;
    lp[(size_t)2 * (4 * SD_G) * (4 * SD_G) + at] = m2;
  }
}

extern "C" int sam6d_samdec_upscale_masks(const float* ct1, long ld, long sp, const float* ln_gamma, const float* ln_beta, float eps,
                                          const float* w2, const float* b2, const float* hyper, float* low, int P, int dim, int heads,
                                          int tokens, int grid_h, int grid_w, void* stream) {
  SAMDEC_REQUIRE_SHAPE("samdec_upscale_masks");
  SAM6D_REQUIRE(P >= 0 && P <= 65535, "samdec_upscale_masks: 0 <= P <= 65535 (got %d)", P);
  if (P == 0) return 0;
  SAM6D_REQUIRE(ct1 && ln_gamma && ln_beta && w2 && b2 && hyper && low, "samdec_upscale_masks: null pointer");
  SAM6D_REQUIRE(ld >= SD_C && (ld & 3) == 0 && (sp & 3) == 0 && ((uintptr_t)ct1 & 15) == 0 && sp >= (long)SD_N * ld - (ld - SD_C),
                "samdec_upscale_masks: rows must be 16-byte aligned and prompts must not overlap (ld %ld, prompt stride %ld)", ld, sp);
  hipLaunchKernelGGL(samdec_upscale_kernel, dim3(SD_N * 4 / 256, P), dim3(256), 0, (hipStream_t)stream, ct1, ld, sp, ln_gamma, ln_beta, eps, w2,
                     b2, hyper, low);
  SAM6D_LAUNCH_CHECK("samdec_upscale_masks");
}
