// SAM's ViT-H image encoder around the library's GEMMs (ISM/segment_anything/modeling/image_encoder.py:106-116 ImageEncoderViT.forward,
// :166-182 Block.forward, :224-240 Attention.forward, :243-289 window_partition / window_unpartition, :292-361 get_rel_pos /
// add_decomposed_rel_pos; common.py:38-43 LayerNorm2d): the attention with decomposed relative-position bias, 16 heads of 80, on the
// 64 x 64 token grid of a 1024 x 1024 image, in its two forms, and the gather of the neck's 3 x 3 convolution.
//   window   14 x 14 windows of the grid padded to 70 x 70: one workgroup per (window, head, image), the register-chained scheme of
//            common.h ("shared steps of the register-chained attention kernels") at 13 key tiles.  Partition and un-partition are index arithmetic; a padded position is a key whose
//            k and v are the qkv bias (the reference pads after norm1, so the padded token is zero) and is never a query.
//   global   4096 keys: one workgroup per (128 queries, head, image), online softmax over 64 tiles of 64 keys = one grid row each.
//            Every workgroup cuts the k and v tiles it reads into fp16 hi / lo images itself (scale per tile): no pre-pass, no
//            workspace; the price is that the 32 workgroups of a head each convert the head's k and v (20 elements per thread and
//            tile, beside 66 MFMAs per wave) and read them as fp32 from the L2.
// Both: scores (q . k) / sqrt(80) + q . Rh[qh - kh + S - 1] + q . Rw[qw - kw + S - 1] with the UNSCALED q in the bias terms.  The bias
// is T^T = R . q^T, two small MFMA products per 16-query group (R split in registers from global memory), re-indexed through a
// wave-private LDS table U[token][k position]; q . k is evaluated unscaled and multiplied by 1 / sqrt(80) in fp32.  Products are
// v_mfma_f32_16x16x32_f16 with three terms (lo.hi, hi.lo, hi.hi) and power-of-two operand scales; softmax in fp32; the probabilities
// never leave the registers (accumulator layout of S^T = B-operand layout of the second product, see common.h).  Head width 80 is
// zero-padded to three k-steps of 32 in the fragments, not in memory.  The kernels do not distinguish matmul modes 0 and 1 (as
// sattn_kernel and dino_attention_kernel).
//
// Resource use (-Rpass-analysis=kernel-resource-usage, gfx950), no scratch in any kernel (tests/test_sam_encoder_host.py keeps it so):
//   sam_window_attention_kernel  124 VGPRs, 162 368 B dynamic LDS, one workgroup of 8 waves per CU
//   sam_global_attention_kernel  162 VGPRs,  78 976 B dynamic LDS (the registers, not the LDS, keep it at one workgroup per CU)
//   sam_neck_gather_kernel        16 VGPRs, no LDS
#include "common.h"
#include "../../include/sam6d_hip.h"

#define SE_HD 80      // head width
#define SE_GRID 64    // tokens per side
#define SE_NTOK 4096
#define SE_KROW 176   // bytes per k row and plane: 80 fp16 + 16 bytes of padding (11 slots of 16 bytes: conflict-free fragment reads)
#define SE_SCALE 0.11180339887498948f  // 80^-0.5
#define SE_LOG2E 1.4426950408889634f

__device__ __forceinline__ void se_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A operand of k-step ks from a k image (rows of SE_KROW bytes per plane): channels 32 ks + 8 fg .. + 7 of `row`, zero from 80 on
__device__ __forceinline__ void se_k_frag(const unsigned char* kh, const unsigned char* kl, int row, int ks, int fg, half8& ah, half8& al) {
  const int c = 32 * ks + 8 * fg;
  const size_t off = (size_t)row * SE_KROW + 2 * min(c, SE_HD - 8);  // (branch-free: a clamped read, then a select)
  const u32x4 z = u32x4{0u, 0u, 0u, 0u};
  const u32x4 vh = *reinterpret_cast<const u32x4*>(kh + off), vl = *reinterpret_cast<const u32x4*>(kl + off);
  ah = __builtin_bit_cast(half8, c < SE_HD ? vh : z);
  al = __builtin_bit_cast(half8, c < SE_HD ? vl : z);
}

// power-of-two scale of a relative-position table (nr x 80 fp32): every wave scans it on its own
__device__ __forceinline__ float se_table_scale(const float* __restrict__ rel, int nr, int lane) {
  float m = 0.f;
  for (int e = lane; e < nr * (SE_HD / 4); e += 64) m = fmaxf(m, amax4(*reinterpret_cast<const float4*>(rel + 4 * e)));
  return pow2_scale(wave_max_dpp(m));
}

// One tile of T^T = R . q^T: rows = table rows 16 t + fr (zero from nr on), columns = the group's tokens.  The lane's register r
// holds sr sq (q_token . R[16 t + 4 fg + r]).
__device__ __forceinline__ f32x4 se_rel_tile(const float* __restrict__ rel, int nr, int t, float sr, const half8* qh, const half8* ql,
                                             int fr, int fg) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int row = 16 * t + fr;
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int c = 32 * ks + 8 * fg;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (row < nr && c < SE_HD) {
      a = *reinterpret_cast<const float4*>(rel + (size_t)row * SE_HD + c);
      b = *reinterpret_cast<const float4*>(rel + (size_t)row * SE_HD + c + 4);
    }
    half8 ah, al;
    split8(a, b, 1.0f, sr, ah, al);
    acc = mfma3_16(ah, al, qh[ks], ql[ks], acc);
  }
  return acc;
}

// ---- windowed attention ---------------------------------------------------------------------------------------------------------
#define SW_WIN 14
#define SW_NW 5                           // windows per side of the 70 x 70 padded grid
#define SW_TOK 196
#define SW_NT 13                          // key tiles of 16 (208 rows, zeros from 196 on)
#define SW_VS 7                           // k-steps of 32 keys of the second product
#define SW_WAVES 8
#define SW_VROW 464                       // bytes per v^T row and plane: 224 fp16 + 16 bytes of padding
#define SW_KPLANE (16 * SW_NT * SE_KROW)  // 36 608
#define SW_VPLANE (SE_HD * SW_VROW)       // 37 120
#define SW_UROW 29                        // floats per token of the bias table: 14 (h) + 14 (w), odd stride
#define SW_UWAVE (16 * SW_UROW * 4)       // 1 856 bytes per wave
#define SW_LDS (2 * SW_KPLANE + 2 * SW_VPLANE + SW_WAVES * SW_UWAVE + 64)  // 162 368 bytes of the 160 KiB

__global__ __launch_bounds__(SW_WAVES * 64) void sam_window_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ pad_qkv,
                                                                             const float* __restrict__ rel_h, const float* __restrict__ rel_w,
                                                                             float* __restrict__ out, int heads) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* kh = lds;
  unsigned char* kl = lds + SW_KPLANE;
  unsigned char* vh = lds + 2 * SW_KPLANE;
  unsigned char* vl = vh + SW_VPLANE;
  float* uall = reinterpret_cast<float*>(vl + SW_VPLANE);
  float* red = uall + SW_WAVES * 16 * SW_UROW;  // 16 floats
  const int wy = blockIdx.x / SW_NW, wx = blockIdx.x % SW_NW, h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const int D = heads * SE_HD;
  const size_t ld = 3 * (size_t)D;
  const float* base = qkv + (size_t)b * SE_NTOK * ld + SE_HD * h;
  const float* padb = pad_qkv + SE_HD * h;
  // the q | k | v row of window position j = 14 jh + jw: a row of the image, or the padding row (the qkv bias)
  auto src = [&](int j) -> const float* {
    const int y = SW_WIN * wy + j / SW_WIN, x = SW_WIN * wx + j % SW_WIN;
    return (y < SE_GRID && x < SE_GRID) ? base + (size_t)(y * SE_GRID + x) * ld : padb;
  };

  // ---- the image scales: max |k|, max |v| over the window's 196 keys (padded ones included)
  float mk = 0.f, mv = 0.f;
  for (int e = t; e < SW_TOK * (SE_HD / 4); e += SW_WAVES * 64) {
    const int j = e / (SE_HD / 4), c4 = e % (SE_HD / 4);
    const float* row = src(j);
    mk = fmaxf(mk, amax4(*reinterpret_cast<const float4*>(row + D + 4 * c4)));
    mv = fmaxf(mv, amax4(*reinterpret_cast<const float4*>(row + 2 * D + 4 * c4)));
  }
  wg_amax_put(mk, mv, red, wave, lane);
  __syncthreads();
  float sk, sv;
  wg_scales_get(red, sk, sv);

  // ---- k image (208 rows, zeros from key 196 on; the row padding is never read) and v^T image (zeros from key 196 to 223)
  attn_build_k<SE_HD, 16 * SW_NT, SE_KROW, SW_WAVES * 64>(kh, kl, t, SW_TOK, sk, src, D);
  attn_build_vt<SE_HD, SW_VS * 32 / 4, SW_VROW, SW_WAVES * 64>(vh, vl, t, SW_TOK, sv, src, 2 * D);
  const float srh = se_table_scale(rel_h, 2 * SW_WIN - 1, lane), srw = se_table_scale(rel_w, 2 * SW_WIN - 1, lane);
  __syncthreads();

  const float inv_k = 1.0f / sk, inv_v = (1.0f / sv) * (1.0f / 16384.0f);
  const int real_rows = min(SW_WIN, SE_GRID - SW_WIN * wy);  // 14, or 8 in the last row of windows
  float* U = uall + wave * 16 * SW_UROW + fr * SW_UROW;       // the lane's token: U[jh] (h table), U[14 + jw] (w table)
  for (int grp = wave; 16 * grp < SW_WIN * real_rows; grp += SW_WAVES) {  // (wave-uniform; groups of padded queries only are skipped)
    const int tq = min(grp * 16 + fr, SW_TOK - 1);
    const int qy = tq / SW_WIN, qx = tq % SW_WIN;
    const int gy = SW_WIN * wy + qy, gx = SW_WIN * wx + qx;
    const bool real = grp * 16 + fr < SW_TOK && gy < SE_GRID && gx < SE_GRID;
    half8 qh[3], ql[3];
    const float sq = split_q_row<SE_HD>(src(tq), fg, 1.0f, qh, ql);
    // (lane coordinates the optimiser cannot see through: what the bias needs that does not depend on the group -- the split table
    // fragments, the 104 (ky, kx) pairs of the lane's keys -- would otherwise be hoisted out of this loop into ~200 registers)
    int fro = fr, fgo = fg;
    asm volatile("" : "+v"(fro), "+v"(fgo));
    // bias table of the group: U[k position] = q . R[q position - k position + 13]
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) {
      const float* rel = tab ? rel_w : rel_h;
      const float sr = tab ? srw : srh;
      const int qpos = tab ? qx : qy;
      const float inv = (1.0f / sr) * (1.0f / sq);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const f32x4 acc = se_rel_tile(rel, 2 * SW_WIN - 1, tt, sr, qh, ql, fro, fgo);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rho = 16 * tt + 4 * fgo + r, j = qpos + (SW_WIN - 1) - rho;
          if (rho < 2 * SW_WIN - 1 && j >= 0 && j < SW_WIN) U[SW_WIN * tab + j] = acc[r] * inv;
        }
      }
    }
    se_wave_sync();
    // S^T tiles: rows = keys 16 i + fr (A operand from the k image), columns = the group's tokens
    f32x4 s[SW_NT];
    const float inv = inv_k * (1.0f / sq);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < SW_NT; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        half8 ah, al;
        se_k_frag(kh, kl, 16 * i + fr, ks, fg, ah, al);
        acc = mfma3_16(ah, al, qh[ks], ql[ks], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * i + 4 * fgo + r;
        float v = -INFINITY;
        if (key < SW_TOK) {
          const int ky = key / SW_WIN, kx = key - SW_WIN * ky;
          v = (acc[r] * inv) * SE_SCALE + (U[ky] + U[SW_WIN + kx]);
        }
        s[i][r] = v;
        mx = fmaxf(mx, v);
      }
    }
    se_wave_sync();  // the table is read; the next group may write it
    const float pscale = attn_softmax(s, mx);
    const SplitB<SW_VS> p = attn_pack_probs<SW_NT, SW_VS>(s, pscale);
    f32x4 o[SE_HD / 16];
#pragma unroll
    for (int i = 0; i < SE_HD / 16; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < SW_VS; ++st) {
        const HiLo8 a = attn_vt_frag<SW_VROW>(vh, vl, 16 * i + fr, st, fg);
        acc = mfma3_16(a.h, a.l, p.h[st], p.l[st], acc);
      }
      o[i] = acc;
    }
    if (real) {
      attn_store(out + ((size_t)b * SE_NTOK + gy * SE_GRID + gx) * D + SE_HD * h, o, inv_v, fg);
    }
  }
}

// pad: the windowed kernel's padding row, NULL for the global kernel (which has none)
static int se_check(const char* name, const float* qkv, const float* pad, bool has_pad, const float* rel_h, const float* rel_w,
                    const float* out, int B, int heads) {
  SAM6D_REQUIRE(qkv && (pad || !has_pad) && rel_h && rel_w && out, "%s: null pointer", name);
  SAM6D_REQUIRE(B >= 0 && B <= 65535, "%s: needs 0 <= B <= 65535 (B = %d)", name, B);
  SAM6D_REQUIRE(heads >= 1 && heads <= 64, "%s: needs 1 <= heads <= 64 heads of 80 channels (heads = %d)", name, heads);
  SAM6D_REQUIRE(((((size_t)qkv) | ((size_t)pad) | ((size_t)rel_h) | ((size_t)rel_w) | ((size_t)out)) & 15) == 0,
                "%s: pointers must be 16-byte aligned", name);
  return 0;
}

extern "C" int sam6d_sam_window_attention(const float* qkv, const float* pad_qkv, const float* rel_h, const float* rel_w, float* out, int B,
                                          int heads, void* stream) {
  if (int rc = se_check("sam_window_attention", qkv, pad_qkv, true, rel_h, rel_w, out, B, heads)) return rc;
  if (B == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "sam_window_attention", {{(const void*)sam_window_attention_kernel, SW_LDS}})) return rc;
  hipLaunchKernelGGL(sam_window_attention_kernel, dim3(SW_NW * SW_NW, heads, B), dim3(SW_WAVES * 64), SW_LDS, (hipStream_t)stream, qkv,
                     pad_qkv, rel_h, rel_w, out, heads);
  SAM6D_LAUNCH_CHECK("sam_window_attention");
}

// ---- global attention -----------------------------------------------------------------------------------------------------------
#define SG_WAVES 8
#define SG_QB (16 * SG_WAVES)             // queries per workgroup
#define SG_KT 64                          // keys per tile: one row of the grid
#define SG_NREL (2 * SE_GRID - 1)         // 127 table rows
#define SG_VROW 144                       // bytes per v^T row and plane: 64 fp16 + 16 bytes of padding
#define SG_KPLANE (SG_KT * SE_KROW)       // 11 264
#define SG_VPLANE (SE_HD * SG_VROW)       // 11 520
#define SG_UROW 65                        // floats per token of the bias table (64 key rows), odd stride
#define SG_UWAVE (16 * SG_UROW * 4)       // 4 160 bytes per wave
#define SG_LDS (2 * SG_KPLANE + 2 * SG_VPLANE + SG_WAVES * SG_UWAVE + 128)  // 78 976 bytes (the 162 registers, not the LDS, keep it at one workgroup per CU)
#define SG_ITEMS (SG_KT * SE_HD / 4)      // 1 280 float4 (k) or key quads x channels (v) per tile
#define SG_PER ((SG_ITEMS + SG_WAVES * 64 - 1) / (SG_WAVES * 64))  // 3 per thread

__global__ __launch_bounds__(SG_WAVES * 64) void sam_global_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ rel_h,
                                                                             const float* __restrict__ rel_w, float* __restrict__ out,
                                                                             int heads) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* kh = lds;
  unsigned char* kl = lds + SG_KPLANE;
  unsigned char* vh = lds + 2 * SG_KPLANE;
  unsigned char* vl = vh + SG_VPLANE;
  float* uall = reinterpret_cast<float*>(vl + SG_VPLANE);
  float* red = uall + SG_WAVES * 16 * SG_UROW;  // 2 x 16 floats
  const int h = blockIdx.y, b = blockIdx.z;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const int D = heads * SE_HD;
  const size_t ld = 3 * (size_t)D;
  const float* base = qkv + (size_t)b * SE_NTOK * ld + SE_HD * h;
  const int tok = blockIdx.x * SG_QB + 16 * wave + fr;  // < 4096: the grid is 4096 / SG_QB workgroups wide
  const int qy = tok / SE_GRID, qx = tok % SE_GRID;

  half8 qh[3], ql[3];
  const float sq = split_q_row<SE_HD>(base + (size_t)tok * ld, fg, 1.0f, qh, ql);
  // ---- bias tables of the wave's 16 queries: U[k position] = q . R[q position - k position + 63].  The w table first: the lane keeps
  // the 16 columns it adds in every key tile (key 16 i + 4 fg + r of a tile is grid column 16 i + 4 fg + r) in registers; the h table
  // stays in LDS, one value per tile.
  float* U = uall + wave * 16 * SG_UROW + fr * SG_UROW;
  float uw[4][4];
#pragma unroll
  for (int tab = 1; tab >= 0; --tab) {
    const float* rel = tab ? rel_w : rel_h;
    const float sr = se_table_scale(rel, SG_NREL, lane);
    const int qpos = tab ? qx : qy;
    const float inv = (1.0f / sr) * (1.0f / sq);
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const f32x4 acc = se_rel_tile(rel, SG_NREL, tt, sr, qh, ql, fr, fg);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rho = 16 * tt + 4 * fg + r, j = qpos + (SE_GRID - 1) - rho;
        if (rho < SG_NREL && j >= 0 && j < SE_GRID) U[j] = acc[r] * inv;
      }
    }
    se_wave_sync();
    if (tab) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) uw[i][r] = U[16 * i + 4 * fg + r];
      se_wave_sync();
    }
  }

  float mrun = -INFINITY, lrun = 0.f;
  f32x4 o[SE_HD / 16];
#pragma unroll
  for (int i = 0; i < SE_HD / 16; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < SE_NTOK / SG_KT; ++kt) {
    // ---- the tile's k and v rows into registers, their max |.| through LDS (red alternates between two halves: one barrier)
    const float* kb = base + (size_t)kt * SG_KT * ld + D;
    const float* vb = kb + D;
    float4 kv[SG_PER], vv[SG_PER];
    float mk = 0.f, mv = 0.f;
#pragma unroll
    for (int u = 0; u < SG_PER; ++u) {
      const int e = t + SG_WAVES * 64 * u;
      kv[u] = vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < SG_ITEMS) {
        kv[u] = *reinterpret_cast<const float4*>(kb + (size_t)(e / (SE_HD / 4)) * ld + 4 * (e % (SE_HD / 4)));
        const int d = e % SE_HD, jq = e / SE_HD;
        const float* vp = vb + (size_t)(4 * jq) * ld + d;
        vv[u] = make_float4(vp[0], vp[ld], vp[2 * ld], vp[3 * ld]);
      }
      mk = fmaxf(mk, amax4(kv[u]));
      mv = fmaxf(mv, amax4(vv[u]));
    }
    float* rd = red + 16 * (kt & 1);
    wg_amax_put(mk, mv, rd, wave, lane);
    __syncthreads();  // every wave is through with the previous tile's images
    float sk, sv;
    wg_scales_get(rd, sk, sv);
#pragma unroll
    for (int u = 0; u < SG_PER; ++u) {
      const int e = t + SG_WAVES * 64 * u;
      if (e < SG_ITEMS) {
        half4 hi4, lo4;
        split4(make_float4(kv[u].x * sk, kv[u].y * sk, kv[u].z * sk, kv[u].w * sk), hi4, lo4);
        const size_t ko = (size_t)(e / (SE_HD / 4)) * SE_KROW + 8 * (e % (SE_HD / 4));
        *reinterpret_cast<half4*>(kh + ko) = hi4;
        *reinterpret_cast<half4*>(kl + ko) = lo4;
        split4(make_float4(vv[u].x * sv, vv[u].y * sv, vv[u].z * sv, vv[u].w * sv), hi4, lo4);
        const size_t vo = (size_t)(e % SE_HD) * SG_VROW + 8 * (e / SE_HD);
        *reinterpret_cast<half4*>(vh + vo) = hi4;
        *reinterpret_cast<half4*>(vl + vo) = lo4;
      }
    }
    __syncthreads();

    // ---- S^T tiles of the 64 keys, the bias, online softmax
    const float inv = (1.0f / sk) * (1.0f / sq);
    const float uh = U[kt];
    f32x4 s[4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        half8 ah, al;
        se_k_frag(kh, kl, 16 * i + fr, ks, fg, ah, al);
        acc = mfma3_16(ah, al, qh[ks], ql[ks], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[i][r] = (acc[r] * inv) * SE_SCALE + (uh + uw[i][r]);
        mx = fmaxf(mx, s[i][r]);
      }
    }
    const float mnew = fmaxf(mrun, tok_max(mx));
    const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * SE_LOG2E);  // 0 in the first tile (mrun = -inf)
    mrun = mnew;
    float sum = 0.f;
    half8 ph[2], pl[2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f((s[i][r] - mnew) * SE_LOG2E);
        sum += p;
        _Float16 hi, lo;
        sam6d_split_f16(p * 16384.0f, hi, lo);  // probabilities times 2^14 (fp16-safe), the 2^-14 is in inv_v
        ph[i >> 1][4 * (i & 1) + r] = hi;
        pl[i >> 1][4 * (i & 1) + r] = lo;
      }
    lrun = lrun * alpha + sum;  // (the lane's share of the token's sum; the four lanes are added at the end)
    const float inv_v = (1.0f / sv) * (1.0f / 16384.0f);
#pragma unroll
    for (int i = 0; i < SE_HD / 16; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const HiLo8 a = attn_vt_frag<SG_VROW>(vh, vl, 16 * i + fr, st, fg);
        acc = mfma3_16(a.h, a.l, ph[st], pl[st], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[i][r] = o[i][r] * alpha + acc[r] * inv_v;
    }
  }
  const float rl = 1.0f / tok_sum(lrun);
  attn_store(out + ((size_t)b * SE_NTOK + tok) * D + SE_HD * h, o, rl, fg);
}

extern "C" int sam6d_sam_global_attention(const float* qkv, const float* rel_h, const float* rel_w, float* out, int B, int heads,
                                          void* stream) {
  if (int rc = se_check("sam_global_attention", qkv, nullptr, false, rel_h, rel_w, out, B, heads)) return rc;
  if (B == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "sam_global_attention", {{(const void*)sam_global_attention_kernel, SG_LDS}})) return rc;
  hipLaunchKernelGGL(sam_global_attention_kernel, dim3(SE_NTOK / SG_QB, heads, B), dim3(SG_WAVES * 64), SG_LDS, (hipStream_t)stream, qkv,
                     rel_h, rel_w, out, heads);
  SAM6D_LAUNCH_CHECK("sam_global_attention");
}

// ---- the neck's 3 x 3 convolution as a gather + GEMM -------------------------------------------------------------------------------
// x (B*4096, 256), channel-last map of the 64 x 64 grid -> rows (B*4096, 2304): columns 256 (3 ky + kx) + c of row (y, x) = channel c
// at (y + ky - 1, x + kx - 1), zeros outside the grid (padding = 1).  One wave per (row, tap), four channels per lane.
__global__ __launch_bounds__(256) void sam_neck_gather_kernel(const float* __restrict__ x, float* __restrict__ rows, long total) {
  const long idx = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= total) return;
  const int lane = threadIdx.x & 63;
  const long row = idx / 9;
  const int tap = (int)(idx % 9), p = (int)(row % SE_NTOK);
  const int sy = p / SE_GRID + tap / 3 - 1, sx = p % SE_GRID + tap % 3 - 1;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (sy >= 0 && sy < SE_GRID && sx >= 0 && sx < SE_GRID)
    v = *reinterpret_cast<const float4*>(x + (row - p + sy * SE_GRID + sx) * 256 + 4 * lane);
  *reinterpret_cast<float4*>(rows + row * 2304 + tap * 256 + 4 * lane) = v;
}

extern "C" int sam6d_sam_neck_gather(const float* x, float* rows, int B, void* stream) {
  SAM6D_REQUIRE(x && rows, "sam_neck_gather: null pointer");
  SAM6D_REQUIRE(B >= 0 && B <= 4096, "sam_neck_gather: needs 0 <= B <= 4096 (B = %d)", B);
  SAM6D_REQUIRE(((((size_t)x) | ((size_t)rows)) & 15) == 0, "sam_neck_gather: pointers must be 16-byte aligned");
  if (B == 0) return 0;
  const long total = (long)B * SE_NTOK * 9;
  hipLaunchKernelGGL(sam_neck_gather_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, rows, total);
  SAM6D_LAUNCH_CHECK("sam_neck_gather");
}
