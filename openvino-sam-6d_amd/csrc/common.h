// Shared helpers for the gfx950 (CDNA4, wave64) kernels of libsam6d_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include <type_traits>

#define SAM6D_WAVE 64

// ---- error plumbing -------------------------------------------------------------------------------------
// Every extern "C" entry point returns 0 on success, a negative SAM6D_E* code for bad arguments and a positive
// hipError_t for runtime failures; sam6d_last_error() returns the text.  (The reference prints and exit(-1)s on a
// CUDA launch failure, EXT/include/cuda_utils.h:42-51; SURVEY 8b asks for a checked error instead.)
#define SAM6D_EINVAL (-1)
#define SAM6D_ENOTIMPL (-2)

void sam6d_set_error(const char* fmt, ...);

#define SAM6D_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      sam6d_set_error(__VA_ARGS__);         \
      return SAM6D_EINVAL;                  \
    }                                       \
  } while (0)

#define SAM6D_LAUNCH_CHECK(name)                                                        \
  do {                                                                                  \
    hipError_t e__ = hipGetLastError();                                                 \
    if (e__ != hipSuccess) {                                                            \
      sam6d_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));           \
      return (int)e__;                                                                  \
    }                                                                                   \
    return 0;                                                                           \
  } while (0)

#define SAM6D_LAUNCH_CHECK_CONT(name)                                                   \
  do {                                                                                  \
    hipError_t e__ = hipGetLastError();                                                 \
    if (e__ != hipSuccess) {                                                            \
      sam6d_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));           \
      return (int)e__;                                                                  \
    }                                                                                   \
  } while (0)

// after the hipMemsetAsync calls of an entry `name`: e is the first error among them
#define SAM6D_MEMSET_CHECK(name, e)                                                     \
  do {                                                                                  \
    if ((e) != hipSuccess) {                                                            \
      sam6d_set_error("%s: memset failed: %s", name, hipGetErrorString(e));             \
      return (int)(e);                                                                  \
    }                                                                                   \
  } while (0)

// the refusal of a null argument, by the argument's own name
#define SAM6D_POINTER(who, p) SAM6D_REQUIRE((p) != nullptr, who ": " #p " is a null pointer")

// ---- device helpers ---------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));     // one MFMA accumulator tile per lane
typedef _Float16 half8 __attribute__((ext_vector_type(8)));  // one fp16 MFMA operand (k = 32) per lane
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes of packed halves: one LDS / buffer fragment read
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the integer reductions: exact, so the order is free
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
// ---- DPP / permlane reductions (no LDS crossbar: ds_bpermute costs an LDS round trip per step, these are plain VALU).
// The summation ORDER differs from the xor butterfly above, so results can differ in the last bit: use them where no bit
// recipe of the reference is pinned (attention, LayerNorm, focus, norms); max / min are order-independent.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), CTRL, 0xf, 0xf, false));
}
// all-reduce over each 16-lane row: rotations by 8, 4, 2, 1 (row_ror) -- every lane ends with the row total
__device__ __forceinline__ float row16_sum_dpp(float v) {
  v += dpp_f32<0x128>(v);  // row_ror:8
  v += dpp_f32<0x124>(v);  // row_ror:4
  v += dpp_f32<0x122>(v);  // row_ror:2
  v += dpp_f32<0x121>(v);  // row_ror:1
  return v;
}
__device__ __forceinline__ float row16_max_dpp(float v) {
  v = fmaxf(v, dpp_f32<0x128>(v));
  v = fmaxf(v, dpp_f32<0x124>(v));
  v = fmaxf(v, dpp_f32<0x122>(v));
  v = fmaxf(v, dpp_f32<0x121>(v));
  return v;
}
// exchange with the lane 16 / 32 away (gfx950 v_permlane16_swap / v_permlane32_swap on a copy)
__device__ __forceinline__ float xor16_f32(float v) {
  typedef unsigned u2_ __attribute__((ext_vector_type(2)));
  const u2_ r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float((threadIdx.x & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float xor32_f32(float v) {
  typedef unsigned u2_ __attribute__((ext_vector_type(2)));
  const u2_ r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = row16_sum_dpp(v);
  v += xor16_f32(v);
  v += xor32_f32(v);
  return v;
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = row16_max_dpp(v);
  v = fmaxf(v, xor16_f32(v));
  v = fmaxf(v, xor32_f32(v));
  return v;
}

// a token's channels live in the four lanes 16 apart (g = lane >> 4) of an MFMA tile: reductions over the token
__device__ __forceinline__ float tok_max(float m) {
  m = fmaxf(m, xor16_f32(m));
  return fmaxf(m, xor32_f32(m));
}
__device__ __forceinline__ float tok_sum(float s) {
  s += xor16_f32(s);
  return s + xor32_f32(s);
}

__device__ __forceinline__ float row16_min_dpp(float v) {
  v = fminf(v, dpp_f32<0x128>(v));
  v = fminf(v, dpp_f32<0x124>(v));
  v = fminf(v, dpp_f32<0x122>(v));
  v = fminf(v, dpp_f32<0x121>(v));
  return v;
}
__device__ __forceinline__ float wave_min_dpp(float v) {
  v = row16_min_dpp(v);
  v = fminf(v, xor16_f32(v));
  v = fminf(v, xor32_f32(v));
  return v;
}
// inclusive prefix sum over the 64 lanes on the DPP path (no ds_bpermute round trips): Hillis-Steele inside each 16-lane row (row_shr
// 1, 2, 4, 8 with zero fill), then the row totals of the rows before (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
__device__ __forceinline__ int wave_incl_scan_i32_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2, 3
  return v;
}
// max / min do not depend on the order of the reduction: the DPP form everywhere (round 4; the ds_bpermute butterfly cost six LDS round
// trips per call in the latency-bound per-proposal kernels)
__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }
__device__ __forceinline__ float wave_min(float v) { return wave_min_dpp(v); }
// first maximum of (value, index) pairs over the wave: the largest value and, among the lanes that hold it, the lowest index (what a
// sequential `v > best` scan in index order keeps).  Indices below 2^24 (exact as floats); index 0x7fffffff = "no element seen".
__device__ __forceinline__ void wave_argmax_first(float& best, int& bi) {
  const float m = wave_max_dpp(best);
  const float nk = wave_max_dpp((best == m && bi != 0x7fffffff) ? -(float)bi : -3.0e38f);
  best = m;
  bi = nk < -1.0e30f ? 0x7fffffff : (int)(-nk);
}
// The first-maximum scan itself: take() the candidates in ascending index order (strict >, so the first maximum stays), wave_merge()
// where a wave shares the scan, label() maps "no element seen" (nothing but -inf / NaN) to 0.
struct FirstMax {
  int bi = 0x7fffffff;
  float best = -INFINITY;
  __device__ __forceinline__ void take(float v, int i) {
    if (v > best) {
      best = v;
      bi = i;
    }
  }
  // a candidate that is itself a (value, index) pair in memory: the index is read only where the value wins
  __device__ __forceinline__ void take(float v, const int* i) {
    if (v > best) {
      best = v;
      bi = *i;
    }
  }
  __device__ __forceinline__ void wave_merge() { wave_argmax_first(best, bi); }
  __device__ __forceinline__ int label() const { return bi == 0x7fffffff ? 0 : bi; }
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// murmur3's 32-bit finaliser (a bijection modulo 2^32) and the counter-based key h(r) = fmix(fmix(r ^ b) + a) of the device draws
// (choice.hip, meshsample.hip; a and b are hashes of the seed and the row)
__device__ __forceinline__ unsigned hash_fmix(unsigned x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned hash_key(unsigned r, unsigned a, unsigned b) { return hash_fmix(hash_fmix(r ^ b) + a); }

// squared distance in the torch-CPU K=3 matmul recipe (PEM/utils/model_utils.py:101-128):
//   s = (p0*p0 + p1*p1) + p2*p2 (plain adds), xy = fma(x2,y2, fma(x1,y1, x0*y0)), d = max((sx - 2xy) + sy, 0)
// The library is built with -ffp-contract=off, so only the explicit fmaf calls fuse.
__device__ __forceinline__ float sqnorm3(float a, float b, float c) { return (a * a + b * b) + c * c; }
__device__ __forceinline__ float pdist3(float x0, float x1, float x2, float sx, float y0, float y1, float y2, float sy) {
  const float xy = fmaf(x2, y2, fmaf(x1, y1, x0 * y0));
  const float d = (sx - 2.0f * xy) + sy;
  return d < 0.0f ? 0.0f : d;
}

// One axis of torch's upsample_bilinear2d with align_corners=False (ATen UpSampleBilinear2d.cu, area_pixel_compute_source_index):
// output index dst of an axis of n source pixels, scale = (float)n / n_out -> the two source indices and their fp32 weights.  The
// recipe of csrc/amg.hip ("THE VALUE OF A PIXEL") and csrc/segresize.hip; one copy, so both sample the same grid.
__host__ __device__ __forceinline__ void amg_tap(float scale, int dst, int n, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > n - 1) i0 = n - 1;  // never taken for a valid size (src < n - 0.5); keeps every index in range
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

// OpenCV's 8-bit INTER_LINEAR (imgproc/src/resize.cpp; the recipe is written down in csrc/rgbprep.hip): saturate_cast<short> of an
// int and of rint(float), and the coordinate map of one output index, scale = 1.0 / ((double)n_out / n) -> (s, f) before any clamp.
__device__ __forceinline__ int sat_s16(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int sat_s16f(float v) { return (int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }
__device__ __forceinline__ void cv_coord(int d, double scale, int& s, float& f) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
}

// sin and cos of the same fp32 argument, <= 1.5 ulp each for |x| < 1e5 (checked against fp64 over [0, 1000], the range of
// the sinusoidal-embedding arguments: indices up to ~870 times frequencies <= 1): three-term Cody-Waite reduction by
// pi/2 with fma, degree-9 / degree-8 minimax polynomials on [-pi/4, pi/4], quadrant fix-up.  ~30 VALU instructions,
// branch-free.  The caller guarantees the range (geo.hip routes clouds with larger indices to the sincosf kernel).
#define SAM6D_FAST_SINCOS_LIMIT 1.0e5f
__device__ __forceinline__ void fast_sincosf(float x, float* sn, float* cs) {
  const float j = rintf(x * 0.636619747f);
  float a = fmaf(j, -1.57079601e+00f, x);
  a = fmaf(j, -3.13916473e-07f, a);
  a = fmaf(j, -5.39030253e-15f, a);
  const float s = a * a;
  float z = 2.86567956e-6f;
  z = fmaf(z, s, -1.98559923e-4f);
  z = fmaf(z, s, 8.33338592e-3f);
  z = fmaf(z, s, -1.66666672e-1f);
  z = z * s;
  const float ps = fmaf(z, a, a);
  float c = 2.44677067e-5f;
  c = fmaf(c, s, -1.38877297e-3f);
  c = fmaf(c, s, 4.16666567e-2f);
  c = fmaf(c, s, -0.5f);
  const float pc = fmaf(c, s, 1.0f);
  const int q = (int)j;
  const float s0 = (q & 1) ? pc : ps, c0 = (q & 1) ? ps : pc;
  *sn = (q & 2) ? -s0 : s0;
  *cs = ((q + 1) & 2) ? -c0 : c0;
}

// fp32 -> fp16 (hi, lo) pair with hi + lo = x to 22 significand bits.  x is first made opaque to the optimiser: when x is the product
// of a multiplication, clang folds the multiplication into ONE of the conversions (v_fma_mixlo_f16: a single rounding of the exact
// product) and uses the separately rounded fp32 product for the other; on a rounding tie the two disagree and hi + lo is off by one
// fp16 ulp of hi (found as a 3e-5 error of a single softmax probability, 2^-11 relative).  The empty asm costs no instruction.
__device__ __forceinline__ void sam6d_split_f16(float x, _Float16& hi, _Float16& lo) {
  asm("" : "+v"(x));
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

// The range of every split-precision operand: its values are multiplied by pow2_scale(their max |.|) before the split and the product
// by the inverse afterwards (exact, both are powers of two), so no hi half overflows fp16 and no lo half falls into subnormals.
__device__ __forceinline__ float pow2_scale(float amax) {
  // power of two s with amax * s in [2^13, 2^14); 1 for zero / non-finite input
  if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.0f;
  int e;
  (void)frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
  e = 14 - e;
  e = e > 100 ? 100 : (e < -100 ? -100 : e);
  return ldexpf(1.0f, e);
}

// The same split for a pair, as four instructions: v_cvt_pk_f16_f32 (hi pair, round to nearest even), two v_fma_mix_f32 (x - hi, exact: the
// fp16 operand is read straight from the packed register) and v_cvt_pk_f16_f32 (lo pair).  The plain C form above costs eight (two
// conversions, two conversions back, two subtractions, a conversion pair, a pack); every split-precision kernel splits activations between
// its MFMAs, where vector instructions are what bounds it (profiles/README.md, issue micro-benchmark).  Bit-identical results.
__device__ __forceinline__ void sam6d_split2_f16(float a, float b, unsigned& hi2, unsigned& lo2) {
  float la, lb;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi2) : "v"(a), "v"(b));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(la) : "v"(hi2), "v"(a));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(lb) : "v"(hi2), "v"(b));
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo2) : "v"(la), "v"(lb));
}

// max |.| of four values
__device__ __forceinline__ float amax4(float a, float b, float c, float d) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))); }
__device__ __forceinline__ float amax4(float4 v) { return amax4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float amax4(f32x4 v) { return amax4(v[0], v[1], v[2], v[3]); }

// four values at once: the hi halves and the lo halves, each as one 8-byte group
__device__ __forceinline__ void split4(const float4 v, half4& hi, half4& lo) {
  unsigned h0, h1, l0, l1;
  sam6d_split2_f16(v.x, v.y, h0, l0);
  sam6d_split2_f16(v.z, v.w, h1, l1);
  hi = __builtin_bit_cast(half4, u32x2{h0, h1});
  lo = __builtin_bit_cast(half4, u32x2{l0, l1});
}

// ---- shared steps of the split-precision panel kernels (block.hip, xattn.hip) ------------------------------------
// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E-1
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// split the pair (a, b) into slots i, i + 1 of an MFMA operand pair: hi halves to xh, lo halves to xl
__device__ __forceinline__ void sam6d_split2_f16(float a, float b, half8& xh, half8& xl, int i) {
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  unsigned hi, lo;
  sam6d_split2_f16(a, b, hi, lo);
  const f16x2 h2 = __builtin_bit_cast(f16x2, hi), l2 = __builtin_bit_cast(f16x2, lo);
  xh[i] = h2[0];
  xh[i + 1] = h2[1];
  xl[i] = l2[0];
  xl[i + 1] = l2[1];
}

// One 256-channel fp32 row as the B operand of a transposed product (block.hip, header comment): lane group fg = lane >> 4 of the
// token's four lanes takes channels 32 s + 4 fg .. + 3 and 32 s + 16 + 4 fg .. + 3 of every k-step s = 0 .. 7.  The row is scaled by
// pow2_scale of its max |.| and split into xh[8] / xl[8]; returns the scale.  NT: non-temporal loads, for rows that are read exactly
// once and must not evict the weight images that every workgroup re-reads from the L2.
template <bool NT>
__device__ __forceinline__ float split_row256(const float* __restrict__ src, int fg, half8* xh, half8* xl) {
  f32x4 va[8], vb[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const f32x4* pa = reinterpret_cast<const f32x4*>(src + 32 * s + 4 * fg);
    const f32x4* pb = reinterpret_cast<const f32x4*>(src + 32 * s + 16 + 4 * fg);
    va[s] = NT ? __builtin_nontemporal_load(pa) : *pa;
    vb[s] = NT ? __builtin_nontemporal_load(pb) : *pb;
  }
  float m = 0.f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    m = fmaxf(m, amax4(va[s]));
    m = fmaxf(m, amax4(vb[s]));
  }
  const float sx = pow2_scale(tok_max(m));
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const float e[8] = {va[s][0], va[s][1], va[s][2], va[s][3], vb[s][0], vb[s][1], vb[s][2], vb[s][3]};
#pragma unroll
    for (int u = 0; u < 8; u += 2) sam6d_split2_f16(e[u] * sx, e[u + 1] * sx, xh[s], xl[s], u);
  }
  return sx;
}

// LDS-DMA of NP pieces of 1 KiB (64 lanes x 16 B) from a global image to the same offsets of its LDS copy: pieces first, first + stride, ...
// (the waves that share a copy pass their index and their number).  Unrolled at compile time, not a loop: in a loop the compiler hoists
// src + lane * 16 as loop-invariant, and every piece then needs a 64-bit vector address instead of scalar base + 32-bit lane offset.
template <int NP>
__device__ __forceinline__ void dma_pieces(const unsigned char* src, unsigned char* dst, int first, int stride, int lane) {
  static_for<0, NP>([&](auto K) {
    const int pc = first + stride * decltype(K)::value;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + (size_t)pc * 1024 + lane * 16),
                                     (void __attribute__((address_space(3)))*)(dst + pc * 1024), 16, 0, 0);
  });
}

// ---- shared steps of the register-chained attention kernels (xattn.hip, dinov2.hip, samenc.hip) ------------------
// One scheme, five kernels (xattn_kernel, sattn_kernel, dino_attention_kernel, sam_window_attention_kernel,
// sam_global_attention_kernel): k and v are cut once into fp16 hi / lo LDS images with a power-of-two scale per image; a 16-token group
// forms S^T = k . q^T on v_mfma_f32_16x16x32_f16 in three products, the softmax runs in registers over the lane's tiles and its three
// partner lanes, the probabilities are scaled by 2^14 and split in place (the accumulator layout of S^T is the B-operand layout of the
// second product: k-slot 8 g + e of step s stands for key 32 s + 16 (e >> 2) + 4 g + (e & 3)), and out^T = v^T . P^T leaves as four
// floats per lane and tile.  Every kernel keeps its own schedule (what is loaded when, how the logits are formed); the steps between
// are these.  profiles/README.md, "Attention-kernel helpers", has the compiled-code comparison and the shapes it refused.

// acc += a . b of one 16x16x32 step from the split operands: al . bh, then ah . bl, then ah . bh
__device__ __forceinline__ f32x4 mfma3_16(half8 ah, half8 al, half8 bh, half8 bl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}
// single (launch-uniform): matmul mode 2 keeps the hi . hi product only
__device__ __forceinline__ f32x4 mfma3_16(half8 ah, half8 al, half8 bh, half8 bl, f32x4 acc, bool single) {
  if (!single) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// The image scales of a workgroup of eight waves, in two halves with the caller's barrier (and whatever else it has to do) between
// them: every wave puts its max |k| and max |v| into red[16]; afterwards every thread takes the power-of-two scales of the two maxima.
__device__ __forceinline__ void wg_amax_put(float mk, float mv, float* red, int wave, int lane) {
  mk = wave_max_dpp(mk);
  mv = wave_max_dpp(mv);
  if (lane == 0) { red[wave] = mk; red[8 + wave] = mv; }
}
__device__ __forceinline__ void wg_scales_get(const float* red, float& sk, float& sv) {
  sk = sv = 0.f;
#pragma unroll
  for (int w = 0; w < 8; ++w) { sk = fmaxf(sk, red[w]); sv = fmaxf(sv, red[8 + w]); }
  sk = pow2_scale(sk);
  sv = pow2_scale(sv);
}

// 8 floats times pre times s as one split operand (pre: a literal prescale such as the softmax's 1 / 8, applied first as the kernels
// always did; 1 costs nothing)
__device__ __forceinline__ void split8(float4 a, float4 b, float pre, float s, half8& hi8, half8& lo8) {
  const float e8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    _Float16 hi, lo;
    sam6d_split_f16(e8[u] * pre * s, hi, lo);
    hi8[u] = hi;
    lo8[u] = lo;
  }
}

// The HD channels of the fp32 row at `src`, times pre, as the split B operand of (HD + 31) / 32 k-steps in the contiguous-slot layout:
// slot 8 fg + e of step ks = channel 32 ks + 8 fg + e, zero from channel HD on.  Returns the row's own power-of-two scale (over the
// four lanes of the token).
template <int HD>
__device__ __forceinline__ float split_q_row(const float* __restrict__ src, int fg, float pre, half8* qh, half8* ql) {
  constexpr int KS = (HD + 31) / 32;
  float4 a[KS], b[KS];
  float m = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = 32 * ks + 8 * fg;
    a[ks] = b[ks] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HD % 32 == 0 || c < HD) {
      a[ks] = *reinterpret_cast<const float4*>(src + c);
      b[ks] = *reinterpret_cast<const float4*>(src + c + 4);
    }
    const float mks = fmaxf(amax4(a[ks]), amax4(b[ks]));
    m = ks ? fmaxf(m, mks) : mks;  // (not fmaxf(0, .) in the first step: an instruction the 64-channel caller never had)
  }
  const float sq = pow2_scale(tok_max(m * pre));
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) split8(a[ks], b[ks], pre, sq, qh[ks], ql[ks]);
  return sq;
}

// The plain (row-major, unswizzled) images.  k: row = key, channel c at byte 2 c of a row of KROW bytes per plane, rows 0 .. NROW - 1
// all written.  v^T: row = channel, key j at byte 2 j of a row of VROW bytes per plane, keys 0 .. 4 NQ - 1 all written.  Both are zero
// from key nkeys on.  Key j's HD channels are src(j)[off .. off + HD); NTH threads share the work (t: the thread's index).
template <int HD, int NROW, int KROW, int NTH, class Src>
__device__ __forceinline__ void attn_build_k(unsigned char* kh, unsigned char* kl, int t, int nkeys, float sk, Src&& src, int off) {
  for (int e = t; e < NROW * (HD / 4); e += NTH) {
    const int j = e / (HD / 4), c4 = e % (HD / 4);
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nkeys) kv = *reinterpret_cast<const float4*>(src(j) + off + 4 * c4);
    half4 hi4, lo4;
    split4(make_float4(kv.x * sk, kv.y * sk, kv.z * sk, kv.w * sk), hi4, lo4);
    *reinterpret_cast<half4*>(kh + (size_t)j * KROW + 8 * c4) = hi4;
    *reinterpret_cast<half4*>(kl + (size_t)j * KROW + 8 * c4) = lo4;
  }
}
template <int HD, int NQ, int VROW, int NTH, class Src>
__device__ __forceinline__ void attn_build_vt(unsigned char* vh, unsigned char* vl, int t, int nkeys, float sv, Src&& src, int off) {
  for (int e = t; e < NQ * HD; e += NTH) {
    const int d = e % HD, jq = e / HD;  // (a wave reads consecutive channels of one key)
    float x4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * jq + u;
      x4[u] = (j < nkeys) ? src(j)[off + d] * sv : 0.f;
    }
    half4 hi4, lo4;
    split4(make_float4(x4[0], x4[1], x4[2], x4[3]), hi4, lo4);
    *reinterpret_cast<half4*>(vh + (size_t)d * VROW + 8 * jq) = hi4;
    *reinterpret_cast<half4*>(vl + (size_t)d * VROW + 8 * jq) = lo4;
  }
}

// Softmax over a token's keys from the finished logits s (masked keys at -inf) and the lane's maximum of them: the token's maximum,
// exp(x - max) in place, the token's sum.  Returns 2^14 / sum: the probabilities go to the second product times 2^14 (<= 2^14:
// fp16-safe) and the caller folds the 2^-14 into its output scale.
template <int NT>
__device__ __forceinline__ float attn_softmax(f32x4 (&s)[NT], float mx) {
  mx = tok_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[i][r] = __builtin_amdgcn_exp2f((s[i][r] - mx) * 1.4426950408889634f);
      sum += s[i][r];
    }
  sum = tok_sum(sum);
  return 16384.0f / sum;
}

// s[i] * pscale as the split B operand of VS k-steps of 32 keys (two tiles per step; zero from tile NT on).  Returned by value: filled
// in through references, the halves are assembled where they are computed and not where they are used, which moves registers
// (README, as above)
template <int VS>
struct SplitB {
  half8 h[VS], l[VS];
};
template <int NT, int VS>
__device__ __forceinline__ SplitB<VS> attn_pack_probs(const f32x4 (&s)[NT], float pscale) {
  SplitB<VS> p;
#pragma unroll
  for (int i = 0; i < 2 * VS; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pv = i < NT ? s[i < NT ? i : 0][r] * pscale : 0.f;
      _Float16 hi, lo;
      sam6d_split_f16(pv, hi, lo);
      p.h[i >> 1][4 * (i & 1) + r] = hi;
      p.l[i >> 1][4 * (i & 1) + r] = lo;
    }
  return p;
}

// A operand of k-step st of the out^T product from a plain v^T image (attn_build_vt; the swizzled images of xattn.hip go through
// xa_mma): keys 32 st + 4 g .. + 3 and 32 st + 16 + 4 g .. + 3 of channel `row`, two 8-byte reads 32 bytes apart per plane.  By value,
// as SplitB; the product loops around it stay in the kernels (README, as above).
struct HiLo8 {
  half8 h, l;
};
template <int VROW>
__device__ __forceinline__ HiLo8 attn_vt_frag(const unsigned char* vh, const unsigned char* vl, int row, int st, int fg) {
  const size_t off = (size_t)row * VROW + 2 * (32 * st + 4 * fg);
  const half4 h0 = *reinterpret_cast<const half4*>(vh + off), h1 = *reinterpret_cast<const half4*>(vh + off + 32);
  const half4 l0 = *reinterpret_cast<const half4*>(vl + off), l1 = *reinterpret_cast<const half4*>(vl + off + 32);
  return HiLo8{half8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]}, half8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]}};
}

// the lane's four channels 16 i + 4 fg .. + 3 of every out^T tile, times scale, to the token's output row
template <int NO>
__device__ __forceinline__ void attn_store(float* dst, const f32x4 (&o)[NO], float scale, int fg) {
#pragma unroll
  for (int i = 0; i < NO; ++i)
    *reinterpret_cast<float4*>(dst + 16 * i + 4 * fg) = make_float4(o[i][0] * scale, o[i][1] * scale, o[i][2] * scale, o[i][3] * scale);
}

// ---- shared steps of the 32x32x16 split-product tile kernels (gemm.hip, ism.hip, finematch.hip) ------------------
// Four waves in a 2 x 2 grid over a BM x BN workgroup tile, each wave TM x TN tiles of v_mfma_f32_32x32x16_f16.  The operands lie in
// LDS as four fp16 planes (A hi, A lo, B hi, B lo) of one 32-wide k chunk; a . b is evaluated as a_lo.b_hi + a_hi.b_lo + a_hi.b_hi.
typedef float f32x16 __attribute__((ext_vector_type(16)));  // one 32 x 32 MFMA accumulator tile per lane

// k chunk of a plane and its LDS row in halves.  Rows of 40 halves (80 B): 16 consecutive rows land on 16 different 16-byte slots of
// the 256-B bank row, so the ds_read_b128 fragment reads are conflict-free.
#define SP_BK 32
#define SP_LD 40

// C/D map of the 32 x 32 tile: register r of lane (fr = lane & 31, fk = lane >> 5) is column fr of row (r & 3) + 8 (r >> 2) + 4 fk.
// row0: the tile's first row, in the caller's index type (the terms are added to it one by one, as the kernels wrote it out).
template <class T>
__device__ __forceinline__ T sp_row(T row0, int r, int fk) {
  return row0 + (r & 3) + 8 * (r >> 2) + 4 * fk;
}

template <int TM, int TN>
__device__ __forceinline__ void sp_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// The four planes of a BM x BN tile in one staging buffer of SpLayout<BM, BN>::HALVES halves: offsets of A hi, A lo, B hi, B lo
template <int BM, int BN>
struct SpLayout {
  static constexpr int AH = 0, AL = BM * SP_LD, BH = 2 * BM * SP_LD, BL = (2 * BM + BN) * SP_LD, HALVES = 2 * (BM + BN) * SP_LD;
};
struct SpPlanes {
  _Float16 *Ah, *Al, *Bh, *Bl;
};

// The products of one staged chunk into the wave's TM x TN accumulators, per accumulator al . bh, then ah . bl, then ah . bh.  The
// wave's tile starts at row wm of the A planes and row wn of the B planes; lane = (fr = lane & 31, fk = lane >> 5).
// single (launch-uniform): matmul mode 2 keeps the hi . hi product only.
template <int TM, int TN>
__device__ __forceinline__ void sp_chunk(f32x16 (&acc)[TM][TN], const SpPlanes& p, int wm, int wn, int fr, int fk, bool single) {
#pragma unroll
  for (int ks = 0; ks < SP_BK; ks += 16) {
    half8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      ah[i] = *reinterpret_cast<const half8*>(&p.Ah[(wm + 32 * i + fr) * SP_LD + ks + 8 * fk]);
      al[i] = *reinterpret_cast<const half8*>(&p.Al[(wm + 32 * i + fr) * SP_LD + ks + 8 * fk]);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bh[j] = *reinterpret_cast<const half8*>(&p.Bh[(wn + 32 * j + fr) * SP_LD + ks + 8 * fk]);
      bl[j] = *reinterpret_cast<const half8*>(&p.Bl[(wn + 32 * j + fr) * SP_LD + ks + 8 * fk]);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if (!single) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
        }
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
      }
  }
}

// Wave-private transposing slab: a wave puts EJ accumulator tiles (32 rows x WC = 32 EJ columns) through LDS so that a lane owns 4
// consecutive columns of one row and its global accesses are 16 bytes wide.  Rows of SLD floats; LPR lanes per row, RPP rows per pass,
// NP passes: pass `it` gives the lane row it * RPP + lane / LPR, columns (lane % LPR) * 4 .. + 3.  The caller reads the slab and
// puts a wave barrier behind its reads before the next write.
template <int EJ>
struct SpSlab {
  static constexpr int WC = EJ * 32, SLD = WC + 4, LPR = WC / 4, RPP = 64 / LPR, NP = 32 / RPP;
  static __device__ __forceinline__ void write(float* slab, const f32x16* tiles, int fr, int fk) {
    float* dst = &slab[sp_row(0, 0, fk) * SLD + fr];
#pragma unroll
    for (int j = 0; j < EJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[sp_row(0, r, 0) * SLD + j * 32] = tiles[j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// One-time per-DEVICE setup (hipFuncSetAttribute, CU count ...): `done` is a bit mask over device ordinals owned by the call site.
// sam6d_first_use_on_device returns true while the calling thread's current device has not COMPLETED its setup; the call site runs the
// setup and, only after it succeeded, calls sam6d_setup_done_on_device -- a failed setup is retried by the next call instead of being
// skipped.  The mask is read / updated atomically: two host threads driving different GPUs may both run the (idempotent) setup of
// their own device, neither can lose the other's bit.  A process that drives several GPUs gets every device initialised, instead of
// device 0's state being reused for all of them.  Ordinals >= SAM6D_MAX_DEVICES: dev_out = -1, the call site rejects the launch.
#define SAM6D_MAX_DEVICES 64
static inline bool sam6d_first_use_on_device(const unsigned long long* done, int* dev_out = nullptr) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev < 0 || dev >= SAM6D_MAX_DEVICES) {
    if (dev_out) *dev_out = -1;
    return true;  // never cached: the setup runs (or the call site rejects the ordinal) on every call
  }
  if (dev_out) *dev_out = dev;
  return ((__atomic_load_n(done, __ATOMIC_ACQUIRE) >> dev) & 1ull) == 0;
}
static inline void sam6d_setup_done_on_device(unsigned long long* done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SAM6D_MAX_DEVICES) return;
  (void)__atomic_fetch_or(done, 1ull << dev, __ATOMIC_RELEASE);
}

// Reserves dynamic LDS beyond the 64 KB default, once per device: hipFuncSetAttribute for every (kernel, bytes) pair; the device's
// bit in the call site's `done` mask is set only after all of them succeeded (see above: a failure is retried by the next call).
struct Sam6dLdsUse {
  const void* kernel;
  int bytes;
};
static inline int sam6d_reserve_lds(unsigned long long* done, const char* name, std::initializer_list<Sam6dLdsUse> uses) {
  if (!sam6d_first_use_on_device(done)) return 0;
  for (const Sam6dLdsUse& u : uses) {
    const hipError_t e = hipFuncSetAttribute(u.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, u.bytes);
    if (e != hipSuccess) {
      sam6d_set_error("%s: cannot reserve %d bytes of LDS: %s", name, u.bytes, hipGetErrorString(e));
      return (int)e;
    }
  }
  sam6d_setup_done_on_device(done);
  return 0;
}

// Compute units of the calling thread's current device, asked once per device (and source file); 0 if the query fails or the ordinal
// is >= SAM6D_MAX_DEVICES -- what a caller does then is its own policy.
static inline int sam6d_cu_count() {
  static int cache[SAM6D_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SAM6D_MAX_DEVICES) return 0;
  int cu = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
  if (cu <= 0) {
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) return 0;
    __atomic_store_n(&cache[dev], cu, __ATOMIC_RELAXED);
  }
  return cu;
}

// matmul mode 2 (fp16 single product) per kernel family: bit 0 generic GEMM, 1 block kernels, 2 cross attention, 3 fine similarity.
// SAM6D_HALF_MASK (environment, read once; default 15 = all) narrows it -- a bisecting aid, see DESIGN "Mode 2".
extern "C" int sam6d_get_matmul_mode(void);
static inline int sam6d_half_for(int family_bit) {
  static int mask = -1;
  if (mask < 0) {
    const char* e = getenv("SAM6D_HALF_MASK");
    mask = e ? atoi(e) : 15;
  }
  return (sam6d_get_matmul_mode() == 2 && ((mask >> family_bit) & 1)) ? 1 : 0;
}
