// ISM's proposal descriptors: CropResizePad and the DINOv2 ViT-L/14 around the library's GEMMs
// (ISM/model/dinov2.py:115-326 CustomDINOv2, ISM/utils/bbox_utils.py:89-126 CropResizePad, ISM/model/vision_transformer.py:179-266,
// ISM/model/layers/attention.py, layers/block.py, layers/layer_scale.py):
//   crops       (H,W,3) u8 image + (N,H,W) masks + (N,4) boxes -> (N,3,224,224) normalised masked crops and (N,224,224) masks in one
//               launch: ToTensor + Normalize, times the mask, crop, nearest resize by 224 / max(box side), zero padding, second resize.
//               A pure gather; every source index is the one torch computes, so the result is bit-exact.
//   patch rows, LayerNorm: patch_rows_kernel<1024, 14, 608> and rows_layernorm_kernel<1024> of vit.hip (the row kernels of the ViT
//               encoders), behind sam6d_dino_patch_rows / sam6d_dino_layernorm1024 there
//   attention   257 tokens, 16 heads of 64: one workgroup per (image, head); see dino_attention_kernel
// The dense projections are sam6d_gemm_nt / _w16 (fc1 with the erf-GELU epilogue, proj / fc2 with the in-place residual; LayerScale is
// folded into their weights at pack time).
#include "common.h"
#include "crop_index.h"
#include "../../include/sam6d_hip.h"

#define DN_C 1024
#define DN_IMG CROP_IMG

// ---- proposal crops -------------------------------------------------------------------------------------------------------------
// which image pixel an output pixel reads: crop_source of crop_index.h, the recipe csrc/refdata.hip shares
__global__ __launch_bounds__(256) void dino_crop_kernel(const unsigned char* __restrict__ img, const float* __restrict__ masks,
                                                        const long long* __restrict__ boxes, int H, int W,
                                                        float* __restrict__ out_rgb, float* __restrict__ out_mask) {
  const int i = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= DN_IMG * DN_IMG) return;
  const int Y = pix / DN_IMG, X = pix % DN_IMG;
  float r = 0.f, g = 0.f, b = 0.f, m = 0.f;
  int sy, sx;
  if (crop_source(boxes + 4 * i, H, W, Y, X, sy, sx)) {
    const size_t at = (size_t)sy * W + sx;
    m = masks[(size_t)i * H * W + at];
    if (out_rgb) {
      const unsigned char* p = img + 3 * at;
      // ToTensor (u8 / 255), Normalize ((x - mean) / std), times the mask: fp32, in torch's order (dinov2.py:144-149, 167-169)
      r = (((float)p[0] / 255.0f) - 0.485f) / 0.229f * m;
      g = (((float)p[1] / 255.0f) - 0.456f) / 0.224f * m;
      b = (((float)p[2] / 255.0f) - 0.406f) / 0.225f * m;
    }
  }
  if (out_rgb) {
    float* o = out_rgb + (size_t)i * 3 * DN_IMG * DN_IMG + pix;
    o[0] = r;
    o[DN_IMG * DN_IMG] = g;
    o[2 * DN_IMG * DN_IMG] = b;
  }
  if (out_mask) out_mask[(size_t)i * DN_IMG * DN_IMG + pix] = m;
}

extern "C" int sam6d_dino_crop_proposals(const unsigned char* image, const float* masks, const long long* boxes, int N, int H, int W,
                                         float* out_rgb, float* out_mask, void* stream) {
  SAM6D_REQUIRE(masks && boxes && (out_rgb || out_mask) && (image || !out_rgb), "dino_crop_proposals: null pointer");
  SAM6D_REQUIRE(N >= 0 && N <= 65535, "dino_crop_proposals: N <= 65535 (got %d)", N);
  SAM6D_REQUIRE(H > 0 && W > 0 && (long)H * W <= 2147483647L / 3, "dino_crop_proposals: bad image size %d x %d", H, W);
  if (N == 0) return 0;
  hipLaunchKernelGGL(dino_crop_kernel, dim3((DN_IMG * DN_IMG + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, image, masks, boxes, H,
                     W, out_rgb, out_mask);
  SAM6D_LAUNCH_CHECK("dino_crop_proposals");
}

// ---- self-attention, up to 272 tokens, 16 heads of 64 ---------------------------------------------------------------------------
// One workgroup (8 waves) per (image, head), the register-chained scheme whose steps are in common.h ("shared steps of the
// register-chained attention kernels") at 17 key tiles, with a schedule of its own: the 197-token kernels of xattn.hip plan their
// registers (13 score tiles, 7 probability k-steps and the prefetched next group beside them) and their two groups per wave around 208
// keys; 272 keys need 17 tiles, 9 k-steps and up to three token groups per wave.  Here:
//   k_h (272 x 64) and v_h^T (64 x 288) are cut ONCE into fp16 hi / lo images in LDS (power-of-two scale per image; rows / keys
//   beyond n are zero), in plain row-major order with 16 bytes of padding per row (no swizzle);
//   every 16-token group of a wave runs   S^T (keys x tok) = k_h . (q / 8)^T     17 tiles x 2 k-steps
//                                         softmax over the lane's 68 values + 3 partner lanes, fp32, keys >= n masked to -inf
//                                         out^T (64 x tok) = v_h^T . P^T         4 tiles x 9 k-steps
//   on v_mfma_f32_16x16x32_f16 with three products per step (lo.hi, hi.lo, hi.hi).  The accumulator of S^T holds keys
//   16 i + 4 g + r of the lane's own token, which is the B-operand layout of the second product when k-slot 8 g + e of step s stands
//   for key 32 s + 16 (e >> 2) + 4 g + (e & 3): the probabilities never leave the registers.
// The token count is not padded in HBM: 257 = 16 tiles + 1 key, the tail is masked here.
#define DA_MAXN 272
#define DA_NT 17
#define DA_VS 9
#define DA_WAVES 8
#define DA_KROW 144                       // bytes per k row and plane: 64 fp16 + 16 bytes of padding
#define DA_VROW 592                       // bytes per v^T row and plane: 288 fp16 + 16 bytes of padding
#define DA_KPLANE (DA_MAXN * DA_KROW)     // 39 168
#define DA_VPLANE (64 * DA_VROW)          // 37 888
#define DA_LDS (2 * DA_KPLANE + 2 * DA_VPLANE + 64)  // 154 176 bytes of the 160 KiB

__global__ __launch_bounds__(DA_WAVES * 64) void dino_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* kh = lds;
  unsigned char* kl = lds + DA_KPLANE;
  unsigned char* vh = lds + 2 * DA_KPLANE;
  unsigned char* vl = vh + DA_VPLANE;
  float* red = reinterpret_cast<float*>(vl + DA_VPLANE);  // 16 floats
  const int h = blockIdx.x, b = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const int ngroups = (n + 15) >> 4;
  const float* kb = qkv + (size_t)b * n * (3 * DN_C) + DN_C + 64 * h;
  const float* vb = kb + DN_C;

  // ---- the image scales: max |k|, max |v| of this (image, head)
  float mk = 0.f, mv = 0.f;
  for (int e = t; e < n * 16; e += DA_WAVES * 64) {
    const int j = e >> 4, c4 = e & 15;
    mk = fmaxf(mk, amax4(*reinterpret_cast<const float4*>(kb + (size_t)j * (3 * DN_C) + 4 * c4)));
    mv = fmaxf(mv, amax4(*reinterpret_cast<const float4*>(vb + (size_t)j * (3 * DN_C) + 4 * c4)));
  }
  mk = wave_max_dpp(mk);
  mv = wave_max_dpp(mv);
  if (lane == 0) { red[wave] = mk; red[8 + wave] = mv; }
  __syncthreads();
  float sk = 0.f, sv = 0.f;
#pragma unroll
  for (int w = 0; w < DA_WAVES; ++w) { sk = fmaxf(sk, red[w]); sv = fmaxf(sv, red[8 + w]); }
  sk = pow2_scale(sk);
  sv = pow2_scale(sv);

  // ---- k_h image (272 rows) and v_h^T image (288 keys), zeros beyond n (second read of k and v: L2)
  auto src = [&](int j) -> const float* { return kb + (size_t)j * (3 * DN_C); };
  attn_build_k<64, DA_MAXN, DA_KROW, DA_WAVES * 64>(kh, kl, t, n, sk, src, 0);
  attn_build_vt<64, DA_VS * 32 / 4, DA_VROW, DA_WAVES * 64>(vh, vl, t, n, sv, src, DN_C);
  __syncthreads();

  const float inv_k = 1.0f / sk, inv_v = (1.0f / sv) * (1.0f / 16384.0f);
  // (the group loop keeps its own text: on the shared softmax / split / fragment / store steps it measured 1.3 % slower, see
  // profiles/README.md, "Attention-kernel helpers")
  for (int grp = wave; grp < ngroups; grp += DA_WAVES) {  // (wave-uniform)
    const int tok = min(grp * 16 + fr, n - 1);
    // q / 8 (the softmax scale 1 / sqrt(64): a power of two) as split B fragments: k-slot 8 g + e of step ks = channel 32 ks + 8 g + e
    const float* qsrc = qkv + ((size_t)b * n + tok) * (3 * DN_C) + 64 * h;
    float4 qa[2], qb[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qa[ks] = *reinterpret_cast<const float4*>(qsrc + 32 * ks + 8 * fg);
      qb[ks] = *reinterpret_cast<const float4*>(qsrc + 32 * ks + 8 * fg + 4);
    }
    float qm = fmaxf(fmaxf(amax4(qa[0]), amax4(qb[0])), fmaxf(amax4(qa[1]), amax4(qb[1])));
    const float sq = pow2_scale(tok_max(qm * 0.125f));
    half8 qh[2], ql[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const float e8[8] = {qa[ks].x, qa[ks].y, qa[ks].z, qa[ks].w, qb[ks].x, qb[ks].y, qb[ks].z, qb[ks].w};
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        _Float16 hi, lo;
        sam6d_split_f16(e8[u] * 0.125f * sq, hi, lo);
        qh[ks][u] = hi;
        ql[ks][u] = lo;
      }
    }
    // S^T tiles: rows = keys 16 i + fr (A operand from the k image), columns = the group's tokens
    f32x4 s[DA_NT];
#pragma unroll
    for (int i = 0; i < DA_NT; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const size_t off = (size_t)(16 * i + fr) * DA_KROW + 64 * ks + 16 * fg;
        const half8 ah = *reinterpret_cast<const half8*>(kh + off);
        const half8 al = *reinterpret_cast<const half8*>(kl + off);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, qh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ql[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, qh[ks], acc, 0, 0, 0);
      }
      s[i] = acc;
    }
    // softmax over the keys (F.softmax: exp(x - max) / sum), the lane's 68 logits and its three partner lanes
    const float inv = inv_k * (1.0f / sq);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < DA_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * i + 4 * fg + r;
        s[i][r] = key < n ? s[i][r] * inv : -INFINITY;
        mx = fmaxf(mx, s[i][r]);
      }
    mx = tok_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < DA_NT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[i][r] = __builtin_amdgcn_exp2f((s[i][r] - mx) * 1.4426950408889634f);
        sum += s[i][r];
      }
    sum = tok_sum(sum);
    const float pscale = 16384.0f / sum;  // probabilities times 2^14 (fp16-safe), the 2^-14 is in inv_v
    half8 ph[DA_VS], pl[DA_VS];
#pragma unroll
    for (int i = 0; i < 2 * DA_VS; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = i < DA_NT ? s[i < DA_NT ? i : 0][r] * pscale : 0.f;
        _Float16 hi, lo;
        sam6d_split_f16(pv, hi, lo);
        ph[i >> 1][4 * (i & 1) + r] = hi;
        pl[i >> 1][4 * (i & 1) + r] = lo;
      }
    // out^T tiles: rows = channels 16 i + fr (A operand from the v^T image: keys 32 s + 4 g .. + 3 and 32 s + 16 + 4 g .. + 3)
    f32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < DA_VS; ++st) {
        const size_t off = (size_t)(16 * i + fr) * DA_VROW + 2 * (32 * st + 4 * fg);
        const half4 h0 = *reinterpret_cast<const half4*>(vh + off), h1 = *reinterpret_cast<const half4*>(vh + off + 32);
        const half4 l0 = *reinterpret_cast<const half4*>(vl + off), l1 = *reinterpret_cast<const half4*>(vl + off + 32);
        const half8 ah = half8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const half8 al = half8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, ph[st], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, pl[st], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ph[st], acc, 0, 0, 0);
      }
      o[i] = acc;
    }
    if (grp * 16 + fr < n) {
      float* dst = out + ((size_t)b * n + tok) * DN_C + 64 * h;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(dst + 16 * i + 4 * fg) = make_float4(o[i][0] * inv_v, o[i][1] * inv_v, o[i][2] * inv_v, o[i][3] * inv_v);
    }
  }
}

extern "C" int sam6d_dino_attention(const float* qkv, float* out, int B, int n, void* stream) {
  SAM6D_REQUIRE(qkv && out && B >= 0, "dino_attention: null pointer");
  SAM6D_REQUIRE(n > 0 && n <= DA_MAXN, "dino_attention: needs 0 < n <= %d tokens per image (n = %d)", DA_MAXN, n);
  SAM6D_REQUIRE(((((size_t)qkv) | ((size_t)out)) & 15) == 0, "dino_attention: pointers must be 16-byte aligned");
  SAM6D_REQUIRE(B <= 65535, "dino_attention: B <= 65535");
  if (B == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "dino_attention", {{(const void*)dino_attention_kernel, DA_LDS}})) return rc;
  hipLaunchKernelGGL(dino_attention_kernel, dim3(DN_C / 64, B), dim3(DA_WAVES * 64), DA_LDS, (hipStream_t)stream, qkv, out, n);
  SAM6D_LAUNCH_CHECK("dino_attention");
}
