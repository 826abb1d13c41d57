// GeometricStructureEmbedding for gfx950 (PEM/model/transformer.py:288-363, SinusoidalPositionalEmbedding :259-285).
//
// Three launches per call, no (B,n,n,3,256) intermediate ever reaches HBM (the reference materialises 3.8 GB of it at
// B=32):
//   1. geo_knn_kernel     per point: squared distances in the torch-CPU bit recipe (common.h pdist3), sqrt, the k=3
//                         nearest neighbours = entries 1..3 of the 4 smallest by (value, index)  (:318-321)
//   2. geo_index_kernel   per pair (i,j): d_idx = sqrt(pd)/sigma_d and the k angular indices
//                         atan2(clamp(|ref x anc|,1e-8), clamp(ref.anc,-1,1)) * factor_a            (:322-341)
//   3. geo_embed_kernel   per 32 pairs: rows {d, a0, a1, a2} x 256 sinusoid features are GENERATED in LDS
//                         (sin/cos of idx*omega_i, interleaved, :276-283) and contracted with proj_d / proj_a on the
//                         fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32); epilogue
//                         out = (acc_d + b_d) + (max_k acc_a + b_a) entirely in registers (:350-361).
// tests/test_geo_shapes_gpu.py pins every stage off the golden shape (n = 4 .. 256, empty and full pair lists, indices on the range ends).
#include "common.h"
#include "../../include/sam6d_hip.h"


// ---------------------------------------------------------------------------------------------------- 1. kNN
// one wave per (b,i); n <= 256 (4 candidates per lane).  4 rounds of wave arg-min on (bits(dist), index).
__global__ __launch_bounds__(256) void geo_knn_kernel(const float* __restrict__ pts, int n, int k, int* __restrict__ knn,
                                                      long total) {
  if (blockIdx.x == 0 && threadIdx.x == 0) knn[total * k] = 0;  // max |index| flag, raised by geo_index_kernel
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= total) return;
  const int lane = threadIdx.x & 63;
  const long b = w / n;
  const int i = (int)(w % n);
  const float* p = pts + b * n * 3;
  const float x0 = p[i * 3], x1 = p[i * 3 + 1], x2 = p[i * 3 + 2];
  const float sx = sqnorm3(x0, x1, x2);
  unsigned long long key[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = lane + 64 * u;
    if (j < n) {
      const float y0 = p[j * 3], y1 = p[j * 3 + 1], y2 = p[j * 3 + 2];
      const float d = sqrtf(pdist3(x0, x1, x2, sx, y0, y1, y2, sqnorm3(y0, y1, y2)));
      key[u] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)j;
    } else {
      key[u] = ~0ull;
    }
  }
  for (int r = 0; r <= k; ++r) {
    unsigned long long m = key[0];
#pragma unroll
    for (int u = 1; u < 4; ++u) m = key[u] < m ? key[u] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long v = __shfl_xor(m, o, 64);
      m = v < m ? v : m;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (key[u] == m) key[u] = ~0ull;  // remove the winner (keys are unique: the index is part of the key)
    if (r >= 1 && lane == 0) knn[w * k + (r - 1)] = (int)(m & 0xffffffffull);
  }
}

// ------------------------------------------------------------------------------------------------ 2. indices
// idx4[(b,i,j)] = {d_idx, a_idx[0..2]}  (k == 3)
__global__ __launch_bounds__(256) void geo_index_kernel(const float* __restrict__ pts, const int* __restrict__ knn, int n,
                                                        float sigma_d, float factor_a, float4* __restrict__ idx4,
                                                        long total, int* __restrict__ maxflag) {
  // One workgroup = 256 consecutive pairs of ONE cloud (grid.y = cloud).  The cloud's points and neighbour lists (n <= 256:
  // 6 KiB) are staged in LDS once, so every per-pair operand is an LDS read instead of a dependent global gather.
  __shared__ float sp[256 * 3];
  __shared__ int sk[256 * 3];
  const long b = blockIdx.y;
  const float* p = pts + b * n * 3;
  for (int i = threadIdx.x; i < n * 3; i += 256) {
    sp[i] = p[i];
    sk[i] = knn[b * n * 3 + i];
  }
  __syncthreads();
  const int pe = blockIdx.x * 256 + threadIdx.x;  // pair within the cloud
  if (pe >= n * n) return;
  const int i = pe / n, j = pe - i * n;
  const long e = b * n * n + pe;
  const float x0 = sp[i * 3], x1 = sp[i * 3 + 1], x2 = sp[i * 3 + 2];
  const float y0 = sp[j * 3], y1 = sp[j * 3 + 1], y2 = sp[j * 3 + 2];
  const float pd = pdist3(x0, x1, x2, sqnorm3(x0, x1, x2), y0, y1, y2, sqnorm3(y0, y1, y2));
  float out[4];
  out[0] = sqrtf(pd) / sigma_d;
  const float a0 = y0 - x0, a1 = y1 - x1, a2 = y2 - x2;  // anchor vector  p_j - p_i
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int q = sk[i * 3 + r];
    const float r0 = sp[q * 3] - x0, r1 = sp[q * 3 + 1] - x1, r2 = sp[q * 3 + 2] - x2;  // reference vector
    // bit recipes of the torch-CPU kernels the reference runs (pinned by tests/golden/geo_embedding.npz; the bg point
    // at (100,100,100) makes ref/anc long and nearly parallel, so the rounding order is visible in the result):
    //   torch.cross       : fma(u_i, v_j, -rn(u_j * v_i))
    //   linalg.norm(dim=3): sqrt(fma(c2,c2, fma(c1,c1, rn(c0*c0))))
    //   sum(ref*anc, -1)  : (rn(r0*a0) + rn(r1*a1)) + rn(r2*a2)
    const float c0 = fmaf(r1, a2, -(r2 * a1)), c1 = fmaf(r2, a0, -(r0 * a2)), c2 = fmaf(r0, a1, -(r1 * a0));
    float s = sqrtf(fmaf(c2, c2, fmaf(c1, c1, c0 * c0)));
    float c = (r0 * a0 + r1 * a1) + r2 * a2;
    s = fmaxf(s, 1e-8f);
    c = fminf(fmaxf(c, -1.0f + 1e-8f), 1.0f - 1e-8f);  // == clamp(-1, 1) in fp32
    out[r + 1] = atan2f(s, c) * factor_a;
  }
  idx4[e] = make_float4(out[0], out[1], out[2], out[3]);
  // embedding arguments are index * omega with omega <= 1: remember when an index leaves the range of the branch-free
  // sincos (never for radius-normalised clouds: the largest index is the bg-point distance, ~870)
  const float m = amax4(out[0], out[1], out[2], out[3]);
  if (!(m < SAM6D_FAST_SINCOS_LIMIT)) atomicMax(maxflag, 1);
}

// ---------------------------------------------------------------------------------------------- 3. embedding
// 256 threads = 4 waves; block = 32 pairs = 128 generated rows (group g: 0 -> d, 1..3 -> a_k); wave w owns output
// columns [64w, 64w+64).  Per 16-wide K chunk: A tile [128][17] generated, B tile {W_d, W_a}[256][17] staged.
#define GE_P 32
#define GE_BK 16
#define GE_LD 17
__global__ __launch_bounds__(256, 2) void geo_embed_kernel(const float4* __restrict__ idx4, const float* __restrict__ div_term,
                                                           const float* __restrict__ Wd, const float* __restrict__ bd,
                                                           const float* __restrict__ Wa, const float* __restrict__ ba,
                                                           float* __restrict__ out, long total,
                                                           const int* __restrict__ maxflag, int only_if_large,
                                                           const int* __restrict__ list, int compact) {
  if (only_if_large && *maxflag == 0) return;  // fallback launch behind the fp16x3 kernel: nothing to do
  if (list) total = list[0];                   // list mode: see geo_embed_h3_kernel
  // blocks of GE_P pairs, grid-strided: the list-mode launches size their grid for a few thousand listed pairs, not for the worst
  // case (every pair listed), whose ~10^5 workgroups did nothing but exit
  for (long blk = blockIdx.x; blk * GE_P < total; blk += gridDim.x) {
  __shared__ float As[4 * GE_P * GE_LD];       // 128 rows
  __shared__ float Bs[2 * 256 * GE_LD];        // [mat][col][k]
  __shared__ float xs[4 * GE_P];               // embedding index of each generated row
  __shared__ int pid[GE_P];                    // output row of each slot
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long p0 = blk * GE_P;
  if (t < GE_P) {
    const long slot = min(p0 + t, total - 1);
    const long e = list ? (long)list[1 + slot] : slot;
    pid[t] = (int)(compact ? slot : e);
    const float4 v = idx4[e];
    xs[0 * GE_P + t] = v.x;
    xs[1 * GE_P + t] = v.y;
    xs[2 * GE_P + t] = v.z;
    xs[3 * GE_P + t] = v.w;
  }
  f32x16 acc[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][j][r] = 0.f;
  __syncthreads();
  const int grow = t & 127, gf0 = (t >> 7) * 4;  // A generation: row, first of 4 frequencies of this chunk
  const float xrow = xs[grow];
  const int fr = lane & 31, fk = lane >> 5;
  const int wn = wave * 64;
  for (int k0 = 0; k0 < 256; k0 += GE_BK) {
    // stage B: 2 mats x 256 cols x 16 k = 2048 float4, 8 per thread
    float4 wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int id = t + 256 * u;
      const int mat = id >> 10, col = (id >> 2) & 255, k4 = (id & 3) * 4;
      const float* src = (mat ? Wa : Wd) + (size_t)col * 256 + k0 + k4;
      wv[u] = *reinterpret_cast<const float4*>(src);
    }
    float sv[4], cv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float om = xrow * div_term[(k0 >> 1) + gf0 + u];
      sincosf(om, &sv[u], &cv[u]);
    }
    __syncthreads();  // previous chunk consumed
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int id = t + 256 * u;
      const int mat = id >> 10, col = (id >> 2) & 255, k4 = (id & 3) * 4;
      float* dst = Bs + (mat * 256 + col) * GE_LD + k4;
      dst[0] = wv[u].x; dst[1] = wv[u].y; dst[2] = wv[u].z; dst[3] = wv[u].w;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      As[grow * GE_LD + 2 * (gf0 + u)] = sv[u];
      As[grow * GE_LD + 2 * (gf0 + u) + 1] = cv[u];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GE_BK; kk += 2) {
      const float bd0 = Bs[(0 * 256 + wn + fr) * GE_LD + kk + fk];
      const float bd1 = Bs[(0 * 256 + wn + 32 + fr) * GE_LD + kk + fk];
      const float ba0 = Bs[(1 * 256 + wn + fr) * GE_LD + kk + fk];
      const float ba1 = Bs[(1 * 256 + wn + 32 + fr) * GE_LD + kk + fk];
      const float a0 = As[(0 * GE_P + fr) * GE_LD + kk + fk];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bd0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bd1, acc[0][1], 0, 0, 0);
#pragma unroll
      for (int g = 1; g < 4; ++g) {
        const float ag = As[(g * GE_P + fr) * GE_LD + kk + fk];
        acc[g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, ba0, acc[g][0], 0, 0, 0);
        acc[g][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, ba1, acc[g][1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn + j * 32 + fr;
    const float vbd = bd ? bd[col] : 0.f, vba = ba ? ba[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int sl = (r & 3) + 8 * (r >> 2) + 4 * fk;
      if (p0 + sl < total) {
        const long e = pid[sl];
        const float d = acc[0][j][r] + vbd;
        const float a = fmaxf(fmaxf(acc[1][j][r], acc[2][j][r]), acc[3][j][r]) + vba;
        out[e * 256 + col] = d + a;
      }
    }
  }
  __syncthreads();  // the next block of pairs reuses the LDS tiles
  }
}


// ---------------------------------------------------------------------------------------------- 3b. embedding, fp16 x3
// Same contraction on v_mfma_f32_32x32x16_f16 with split operands (gemm.hip explains the arithmetic): 64 pairs
// (256 generated rows) per workgroup of 8 waves; wave (ph, cq) owns pairs [32 ph, +32) x columns [64 cq, +64) for all
// four row groups, so the max over the 3 angular rows and the final add stay in registers.  proj_d / proj_a arrive
// pre-split and pre-tiled: Wp[kc][mat][col][40 halves] = 16 hi | 16 lo | 8 pad halves of (W * 1024)[col][16 kc .. +16]
// (sam6d_split_f16 + a host-side re-tiling at weight-load time); 2^-10 is undone in the epilogue (exact).
#define GH_P 64
#define GH_BK 16
#define GH_LD 24                        // halves per A row in LDS (48 B)
#define GH_BROW 80                      // bytes per weight row image: 16 hi halves | 16 lo halves | 16 B pad
#define GH_BCHUNK (2 * 256 * GH_BROW)   // 40 960 B: one 16-wide K chunk of {proj_d, proj_a}
#define GH_ABYTES (2 * 4 * GH_P * GH_LD * 2)
#define GH_LDS_BYTES (GH_ABYTES + 2 * GH_BCHUNK + 4 * GH_P * 4 + 128 * 4 + GH_P * 4)

__global__ __launch_bounds__(512) void geo_embed_h3_kernel(const float4* __restrict__ idx4, const float* __restrict__ div_term,
                                                           const unsigned char* __restrict__ Wp, const float* __restrict__ bd,
                                                           const float* __restrict__ ba, float* __restrict__ out, long total,
                                                           const int* __restrict__ maxflag, const int* __restrict__ list,
                                                           int compact) {
  if (*maxflag != 0) return;  // an index beyond the fast sincos range: the exact kernel launched next handles the call
  // list mode (fix-up pass behind geo_cheb_kernel): list[0] = number of listed pairs, list[1..] = their flat pair ids
  if (list) total = list[0];
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  for (long blk = blockIdx.x; blk * GH_P < total; blk += gridDim.x) {  // grid-strided blocks of GH_P pairs (see geo_embed_kernel)
  _Float16* Ah = reinterpret_cast<_Float16*>(lds_raw);  // [256][24]
  _Float16* Al = Ah + 4 * GH_P * GH_LD;
  unsigned char* Bb = lds_raw + GH_ABYTES;               // 2 x [512 rows][80 B], filled by LDS-DMA
  float* xs = reinterpret_cast<float*>(Bb + 2 * GH_BCHUNK);  // [4][64]
  float* om = xs + 4 * GH_P;                                 // [128] frequencies (bit-identical copy of div_term)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long p0 = blk * GH_P;
  // weights: the global image of a chunk IS the LDS image (rows of 80 B), so each wave copies 5 x 1 KiB pieces with
  // global_load_lds_dwordx4 (no VGPRs, no ds_write); double-buffered, chunk kc+1 streams in under chunk kc's MFMAs
  auto dma = [&](int kc) {
    const unsigned char* src = Wp + (size_t)kc * GH_BCHUNK + (size_t)(wave * 5) * 1024 + lane * 16;
    unsigned char* dst = Bb + (kc & 1) * GH_BCHUNK + (wave * 5) * 1024;
#pragma unroll
    for (int i = 0; i < 5; ++i)
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + i * 1024),
                                       (void __attribute__((address_space(3)))*)(dst + i * 1024), 16, 0, 0);
  };
  dma(0);
  int* pid = reinterpret_cast<int*>(om + 128);  // [64] flat pair id of each slot (list mode)
  if (t < GH_P) {
    const long slot = min(p0 + t, total - 1);
    const long e = list ? (long)list[1 + slot] : slot;
    const float4 v = idx4[e];
    xs[0 * GH_P + t] = v.x;
    xs[1 * GH_P + t] = v.y;
    xs[2 * GH_P + t] = v.z;
    xs[3 * GH_P + t] = v.w;
    pid[t] = (int)(compact ? slot : e);  // compact: listed pair i -> output row i (no bias: see sam6d_geo_outliers)
  }
  if (t >= 256 && t < 384) om[t - 256] = div_term[t - 256];
  f32x16 acc[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][j][r] = 0.f;
  __syncthreads();
  const int grow = t & 255, gf0 = (t >> 8) * 4;  // A generation: row, first of the 4 frequencies of this chunk
  const float xrow = xs[grow];
  const int fr = lane & 31, fk = lane >> 5;
  const int ph = wave & 1, wn = (wave >> 1) * 64;
  half8 ahi, alo;
  auto produce1 = [&](int kc, int u) {  // one sin/cos pair of chunk kc's sinusoid row, split into fp16 hi/lo
    float sv, cv;
    fast_sincosf(xrow * om[kc * 8 + gf0 + u], &sv, &cv);
    _Float16 sh, sl, ch, cl;
    sam6d_split_f16(sv, sh, sl);
    sam6d_split_f16(cv, ch, cl);
    ahi[2 * u] = sh;
    ahi[2 * u + 1] = ch;
    alo[2 * u] = sl;
    alo[2 * u + 1] = cl;
  };
#pragma unroll
  for (int u = 0; u < 4; ++u) produce1(0, u);
  for (int kc = 0; kc < 256 / GH_BK; ++kc) {
    // global_load_lds completion is counted by vmcnt, but the compiler does not tie the LDS image to it: without this wait
    // the barrier below is a bare s_barrier and another wave can read a weight row whose DMA is still in flight
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // chunk kc-1 consumed; every wave's DMA pieces of chunk kc have landed
    *reinterpret_cast<half8*>(&Ah[grow * GH_LD + 2 * gf0]) = ahi;
    *reinterpret_cast<half8*>(&Al[grow * GH_LD + 2 * gf0]) = alo;
    __syncthreads();  // A rows and every wave's DMA pieces visible
    const bool more = kc + 1 < 256 / GH_BK;
    if (more) dma(kc + 1);
    const unsigned char* Bc = Bb + (kc & 1) * GH_BCHUNK;
    // the ~45 VALU instructions of one sin/cos pair of the NEXT chunk are issued behind each row group's 6 MFMAs, so
    // they run while the matrix pipe is busy (an MFMA holds the issue port for 8 of its 32 cycles)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const half8 ah = *reinterpret_cast<const half8*>(&Ah[(g * GH_P + ph * 32 + fr) * GH_LD + 8 * fk]);
      const half8 al = *reinterpret_cast<const half8*>(&Al[(g * GH_P + ph * 32 + fr) * GH_LD + 8 * fk]);
      const int mt = g ? 1 : 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned char* row = Bc + (size_t)(mt * 256 + wn + 32 * j + fr) * GH_BROW + 16 * fk;
        const half8 bh = *reinterpret_cast<const half8*>(row);
        const half8 bl = *reinterpret_cast<const half8*>(row + 32);
        acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[g][j], 0, 0, 0);
        acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[g][j], 0, 0, 0);
        acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[g][j], 0, 0, 0);
      }
      if (more) produce1(kc + 1, g);
    }
  }
  const float unscale = 1.0f / 1024.0f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn + j * 32 + fr;
    const float vbd = bd ? bd[col] : 0.f, vba = ba ? ba[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int sl = ph * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      if (p0 + sl < total) {
        const long e = list ? (long)pid[sl] : p0 + sl;
        const float d = acc[0][j][r] * unscale + vbd;
        const float a = fmaxf(fmaxf(acc[1][j][r], acc[2][j][r]), acc[3][j][r]) * unscale + vba;
        out[e * 256 + col] = d + a;
      }
    }
  }
  __syncthreads();  // the next block of pairs reuses the LDS images
  }
}

// x -> (hi, lo) fp16 pair of x*scale: hi = fp16(x*scale), lo = fp16(x*scale - hi)   (weight packing, load time)
__global__ void split_f16_kernel(const float* __restrict__ x, long n, float scale, _Float16* __restrict__ hi,
                                 _Float16* __restrict__ lo) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  _Float16 h, l;
  sam6d_split_f16(x[e] * scale, h, l);
  hi[e] = h;
  lo[e] = l;
}

extern "C" int sam6d_split_f16(const float* x, long n, float scale, void* hi, void* lo, void* stream) {
  SAM6D_REQUIRE(x && hi && lo && n >= 0, "split_f16: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, scale,
                     reinterpret_cast<_Float16*>(hi), reinterpret_cast<_Float16*>(lo));
  SAM6D_LAUNCH_CHECK("split_f16");
}

static int h3_reserve_lds() {
  static unsigned long long attr_done = 0;
  return sam6d_reserve_lds(&attr_done, "geo_embed_h3", {{(const void*)geo_embed_h3_kernel, GH_LDS_BYTES}});
}

extern "C" int sam6d_geo_embed_h3(const float* idx_ws, long pairs, const float* div_term, const void* w_packed, const float* bd,
                                  const float* ba, int hidden, const int* flag, float* out, void* stream) {
  SAM6D_REQUIRE(idx_ws && div_term && w_packed && bd && ba && out && flag, "geo_embed_h3: null pointer");
  SAM6D_REQUIRE(hidden == 256 && pairs >= 0, "geo_embed_h3: hidden_dim must be 256");
  SAM6D_REQUIRE((((size_t)idx_ws | (size_t)w_packed) & 15) == 0, "geo_embed_h3: idx_ws/weights must be 16-byte aligned");
  if (pairs == 0) return 0;
  if (int rc = h3_reserve_lds()) return rc;
  hipLaunchKernelGGL(geo_embed_h3_kernel, dim3((unsigned)((pairs + GH_P - 1) / GH_P)), dim3(512), GH_LDS_BYTES,
                     (hipStream_t)stream, reinterpret_cast<const float4*>(idx_ws), div_term,
                     reinterpret_cast<const unsigned char*>(w_packed), bd, ba, out, pairs, flag, (const int*)nullptr, 0);
  SAM6D_LAUNCH_CHECK("geo_embed_h3");
}



// pos[pair] = -1 when all four indices of the pair lie in [0, xmax] (Chebyshev range), else its slot in list[1..]; list[0] = count
// zeroes the list counter (a kernel rather than hipMemsetAsync: one launch path for everything on the stream)
__global__ void geo_list_reset_kernel(int* __restrict__ list) { list[0] = 0; }

// One workgroup classifies GCL_PER = 4096 pairs and reserves its list slots with ONE atomic (every out-of-range pair doing its own
// atomicAdd on the single counter serialised ~13 000 atomics: 150 us for a 10 us pass; the bg token alone puts an out-of-range
// pair into every 197-pair row).  The order of the list entries is arbitrary; consumers address rows through pos[].
#define GCL_PPT 16
#define GCL_PER (256 * GCL_PPT)
__global__ __launch_bounds__(256) void geo_classify_kernel(const float4* __restrict__ idx4, long total, float xmax, float xmax_a,
                                                           int* __restrict__ pos, int* __restrict__ list) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long e0 = (long)blockIdx.x * GCL_PER + t;
  unsigned int out_mask = 0u;
#pragma unroll
  for (int i = 0; i < GCL_PPT; ++i) {
    const long e = e0 + (long)i * 256;
    if (e < total) {
      const float4 v = idx4[e];
      const bool ok = v.x >= 0.f && v.x <= xmax && v.y >= 0.f && v.y <= xmax_a && v.z >= 0.f && v.z <= xmax_a && v.w >= 0.f &&
                      v.w <= xmax_a;  // x: the distance index, y z w: the angular ones
      if (!ok) out_mask |= 1u << i;
    }
  }
  const int cnt = __popc(out_mask);
  int incl = cnt;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (t == 0) {
    const int all = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = all > 0 ? atomicAdd(list, all) : 0;
  }
  __syncthreads();
  int p = s_base + (incl - cnt);
  for (int w = 0; w < wave; ++w) p += s_wave[w];
#pragma unroll
  for (int i = 0; i < GCL_PPT; ++i) {
    const long e = e0 + (long)i * 256;
    if (e < total) {
      if ((out_mask >> i) & 1u) {
        list[1 + p] = (int)e;
        pos[e] = p;
        ++p;
      } else {
        pos[e] = -1;
      }
    }
  }
}

// ------------------------------------------------------------------------------------- 3c. embedding, Chebyshev basis
// proj_d(sinusoid(x)) and proj_a(sinusoid(x)) are, per output column, smooth 1-D functions of the scalar index x
// (a sum of 128 sin/cos pairs with frequencies <= 1 rad per unit).  On [0, xmax] each is reproduced to ~1e-11 by its
// degree-31 Chebyshev interpolant (weight-load time, float64), so the 256-deep sinusoid contraction collapses to a
// 32-deep one against T_0..T_31(2x/xmax - 1):  8x fewer MFMAs and no sin/cos at all.  The basis is generated per scalar
// by the three-term recurrence in fp64 (exact to fp32), split into fp16 hi/lo and contracted on v_mfma_f32_32x32x16_f16
// with the same 3-product split arithmetic as above.  With the contraction this cheap the kernel is bound by the HBM
// write of E (1 KiB per pair).
// Pairs with an index outside [0, xmax] (the bg token at (100,100,100): d_idx ~ 870; 2n-1 of n^2 pairs) are appended to
// a list and recomputed by geo_embed_h3_kernel in list mode.
// Persistent workgroups (one per CU): the two coefficient matrices stay in LDS (72 KiB), the generated A tile is
// double-buffered so that the recurrence for tile i+1 runs under the MFMAs / stores of tile i.
#define GC_K 32
#define GC_ROW 144                       // bytes per row image: 32 hi halves | 32 lo halves | 16 B pad
#define GC_WBYTES (2 * 256 * GC_ROW)     // 73 728
#define GC_ABYTES (4 * GH_P * GC_ROW)    // 36 864 per buffer
#define GC_LDS_BYTES (GC_WBYTES + 2 * GC_ABYTES)
__global__ __launch_bounds__(512) void geo_cheb_kernel(const float4* __restrict__ idx4, const unsigned char* __restrict__ Wc,
                                                       const float* __restrict__ bd, const float* __restrict__ ba,
                                                       float* __restrict__ out, long total, float xmax,
                                                       const int* __restrict__ maxflag, const int* __restrict__ pos) {
  if (*maxflag != 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned char* Bw = lds_raw;
  unsigned char* At = lds_raw + GC_WBYTES;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int i = t; i < GC_WBYTES / 16; i += 512)
    reinterpret_cast<uint4*>(Bw)[i] = reinterpret_cast<const uint4*>(Wc)[i];
  const long ntiles = (total + GH_P - 1) / GH_P;
  const int grow = t & 255, ghalf = t >> 8;  // generation: row (group g = grow >> 6, pair slot = grow & 63), which 16 orders
  const int fr = lane & 31, fk = lane >> 5;
  const int ph = wave & 1, wn = (wave >> 1) * 64;
  const double inv = 2.0 / (double)xmax;
  auto generate = [&](long tile, int buf) {
    const long e = min(tile * GH_P + (grow & 63), total - 1);
    const float4 v = idx4[e];
    const int g = grow >> 6;
    const float x = g == 0 ? v.x : g == 1 ? v.y : g == 2 ? v.z : v.w;
    const bool inside = x >= 0.f && x <= xmax;  // false for NaN too
    const double u = inside ? (double)x * inv - 1.0 : 0.0;  // listed pairs: a harmless in-range value, row never stored
    const double u2 = u + u;
    double t0 = 1.0, t1 = u;
    unsigned char* row = At + buf * GC_ABYTES + grow * GC_ROW;
    half8 hi[2], lo[2];
#pragma unroll
    for (int p = 0; p < GC_K; ++p) {
      const double tp = p == 0 ? 1.0 : p == 1 ? u : __builtin_fma(u2, t1, -t0);
      if (p >= 2) {
        t0 = t1;
        t1 = tp;
      }
      if ((p >> 4) == ghalf) {  // wave-uniform: threads 0..255 keep orders 0..15, threads 256..511 orders 16..31
        const float f = (float)tp;
        const _Float16 h = (_Float16)f;
        hi[(p >> 3) & 1][p & 7] = h;
        lo[(p >> 3) & 1][p & 7] = (_Float16)(f - (float)h);
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *reinterpret_cast<half8*>(row + (ghalf * 16 + q * 8) * 2) = hi[q];
      *reinterpret_cast<half8*>(row + 64 + (ghalf * 16 + q * 8) * 2) = lo[q];
    }
  };
  long tile = blockIdx.x;
  if (tile < ntiles) generate(tile, 0);
  __syncthreads();
  const float unscale = 1.0f / 1024.0f;
  int buf = 0;
  for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    if (tile + gridDim.x < ntiles) generate(tile + gridDim.x, buf ^ 1);
    f32x16 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][j][r] = 0.f;
    const unsigned char* Ab = At + buf * GC_ABYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8 bh[2][2], bl[2][2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const unsigned char* row = Bw + (size_t)(mt * 256 + wn + 32 * j + fr) * GC_ROW + (ks * 16 + fk * 8) * 2;
          bh[mt][j] = *reinterpret_cast<const half8*>(row);
          bl[mt][j] = *reinterpret_cast<const half8*>(row + 64);
        }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const unsigned char* row = Ab + (size_t)(g * GH_P + ph * 32 + fr) * GC_ROW + (ks * 16 + fk * 8) * 2;
        const half8 ah = *reinterpret_cast<const half8*>(row);
        const half8 al = *reinterpret_cast<const half8*>(row + 64);
        const int mt = g ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[mt][j], acc[g][j], 0, 0, 0);
          acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[mt][j], acc[g][j], 0, 0, 0);
          acc[g][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[mt][j], acc[g][j], 0, 0, 0);
        }
      }
    }
    const long p0 = tile * GH_P;
    // rows of listed pairs (pos >= 0) belong to the sinusoid kernel: the two kernels never store to the same address
    unsigned keepmask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long e = p0 + ph * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      if (e < total && pos[e] < 0) keepmask |= 1u << r;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = wn + j * 32 + fr;
      const float vbd = bd[col], vba = ba[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long e = p0 + ph * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
        if ((keepmask >> r) & 1u) {
          const float d = acc[0][j][r] * unscale + vbd;
          const float a = fmaxf(fmaxf(acc[1][j][r], acc[2][j][r]), acc[3][j][r]) * unscale + vba;
          out[e * 256 + col] = d + a;
        }
      }
    }
    __syncthreads();  // every wave is done with buffer `buf`; the next tile's rows (other buffer) are complete
  }
}

extern "C" int sam6d_geo_embed_cheb(const float* idx_ws, long pairs, const void* w_cheb, float xmax, const float* div_term,
                                    const void* w_packed, const float* bd, const float* ba, int hidden, const int* flag,
                                    int* pos_ws, int* list_ws, float* out, void* stream) {
  SAM6D_REQUIRE(idx_ws && w_cheb && div_term && w_packed && bd && ba && out && flag && list_ws && pos_ws,
                "geo_embed_cheb: null pointer");
  SAM6D_REQUIRE(hidden == 256 && pairs >= 0 && pairs < 2147483647L, "geo_embed_cheb: hidden_dim must be 256, pairs < 2^31");
  SAM6D_REQUIRE(xmax > 0.f, "geo_embed_cheb: xmax must be positive");
  SAM6D_REQUIRE((((size_t)idx_ws | (size_t)w_packed | (size_t)w_cheb) & 15) == 0,
                "geo_embed_cheb: idx_ws/weights must be 16-byte aligned");
  if (pairs == 0) return 0;
  if (int rc = h3_reserve_lds()) return rc;
  static unsigned long long cheb_done = 0;
  if (int rc = sam6d_reserve_lds(&cheb_done, "geo_embed_cheb", {{(const void*)geo_cheb_kernel, GC_LDS_BYTES}})) return rc;
  const int n_cu = sam6d_cu_count();  // the persistent grid's size
  SAM6D_REQUIRE(n_cu > 0, "geo_embed_cheb: cannot query the device's CU count (or device ordinal beyond SAM6D_MAX_DEVICES)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(geo_list_reset_kernel, dim3(1), dim3(1), 0, s, list_ws);
  hipLaunchKernelGGL(geo_classify_kernel, dim3((unsigned)((pairs + GCL_PER - 1) / GCL_PER)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(idx_ws), pairs, xmax, xmax, pos_ws, list_ws);
  SAM6D_LAUNCH_CHECK_CONT("geo_embed_cheb(classify)");
  const long ntiles = (pairs + GH_P - 1) / GH_P;
  hipLaunchKernelGGL(geo_cheb_kernel, dim3((unsigned)(ntiles < n_cu ? ntiles : n_cu)), dim3(512), GC_LDS_BYTES, s,
                     reinterpret_cast<const float4*>(idx_ws), reinterpret_cast<const unsigned char*>(w_cheb), bd, ba, out, pairs,
                     xmax, flag, (const int*)pos_ws);
  SAM6D_LAUNCH_CHECK_CONT("geo_embed_cheb");
  hipLaunchKernelGGL(geo_embed_h3_kernel, dim3((unsigned)(ntiles < 2048 ? ntiles : 2048)), dim3(512), GH_LDS_BYTES, s,
                     reinterpret_cast<const float4*>(idx_ws), div_term, reinterpret_cast<const unsigned char*>(w_packed), bd, ba,
                     out, pairs, flag, (const int*)list_ws, 0);  // list mode: grid-strided over the listed pairs
  SAM6D_LAUNCH_CHECK("geo_embed_cheb(fix-up)");
}

// ------------------------------------------------------------------------------------------ 3d. out-of-range pairs
// The fused RPE attention (rpe.hip) never materialises E: it rebuilds the in-range part from the Chebyshev basis.  Pairs
// with an index outside [0, xmax] get their (bias-free) embedding row from the sinusoid kernels once per call, into the
// compact buffer rows[pos[pair]]; pos[pair] = -1 for in-range pairs.
extern "C" int sam6d_geo_outliers(const float* idx_ws, long pairs, float xmax, const float* div_term, const void* w_packed,
                                  const float* Wd, const float* Wa, const int* flag, int* pos_ws, int* list_ws, float* rows,
                                  void* stream) {
  return sam6d_geo_outliers2(idx_ws, pairs, xmax, xmax, div_term, w_packed, Wd, Wa, flag, pos_ws, list_ws, rows, stream);
}

extern "C" int sam6d_geo_outliers2(const float* idx_ws, long pairs, float xmax, float xmax_a, const float* div_term,
                                   const void* w_packed, const float* Wd, const float* Wa, const int* flag, int* pos_ws, int* list_ws,
                                   float* rows, void* stream) {
  SAM6D_REQUIRE(idx_ws && div_term && w_packed && Wd && Wa && flag && pos_ws && list_ws && rows, "geo_outliers: null pointer");
  SAM6D_REQUIRE(pairs >= 0 && pairs < 2147483647L && xmax > 0.f && xmax_a > 0.f, "geo_outliers: bad sizes");
  SAM6D_REQUIRE((((size_t)idx_ws | (size_t)w_packed | (size_t)Wd | (size_t)Wa) & 15) == 0, "geo_outliers: 16-byte alignment");
  if (pairs == 0) return 0;
  if (int rc = h3_reserve_lds()) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(geo_list_reset_kernel, dim3(1), dim3(1), 0, s, list_ws);
  hipLaunchKernelGGL(geo_classify_kernel, dim3((unsigned)((pairs + GCL_PER - 1) / GCL_PER)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(idx_ws), pairs, xmax, xmax_a, pos_ws, list_ws);
  SAM6D_LAUNCH_CHECK_CONT("geo_outliers(classify)");
  // rows of the listed pairs, bias-free, compact.  The grid covers the worst case (every pair listed); workgroups beyond
  // the device-side count return at once.  Default: fp16x3 sinusoid kernel; *flag != 0: the exact sincosf kernel.
  const long cap = 2048;  // list mode: the kernels stride over the listed pairs (the count lives on the device)
  const long g_h3 = (pairs + GH_P - 1) / GH_P, g_ex = (pairs + GE_P - 1) / GE_P;
  hipLaunchKernelGGL(geo_embed_h3_kernel, dim3((unsigned)(g_h3 < cap ? g_h3 : cap)), dim3(512), GH_LDS_BYTES, s,
                     reinterpret_cast<const float4*>(idx_ws), div_term, reinterpret_cast<const unsigned char*>(w_packed),
                     (const float*)nullptr, (const float*)nullptr, rows, pairs, flag, (const int*)list_ws, 1);
  SAM6D_LAUNCH_CHECK_CONT("geo_outliers(h3 rows)");
  hipLaunchKernelGGL(geo_embed_kernel, dim3((unsigned)(g_ex < cap ? g_ex : cap)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(idx_ws), div_term, Wd, (const float*)nullptr, Wa, (const float*)nullptr, rows,
                     pairs, flag, 1, (const int*)list_ws, 1);
  SAM6D_LAUNCH_CHECK("geo_outliers(exact rows)");
}

static int geo_check(int B, int n, int angle_k, int hidden) {
  SAM6D_REQUIRE(angle_k == 3 && hidden == 256, "geo_embedding: only angle_k=3, hidden_dim=256 (PEM/config/base.yaml:26-31)");
  SAM6D_REQUIRE(B >= 0 && B <= 65535 && n >= 4 && n <= 256, "geo_embedding: need B <= 65535 and 4 <= n <= 256 (got B = %d, n = %d)",
                B, n);
  return 0;
}

extern "C" int sam6d_geo_indices(const float* points, int B, int n, float sigma_d, float factor_a, int angle_k, int* knn_ws,
                                 float* idx_ws, void* stream) {
  SAM6D_REQUIRE(points && knn_ws && idx_ws, "geo_indices: null pointer");
  if (int rc = geo_check(B, n, angle_k, 256)) return rc;
  SAM6D_REQUIRE((((size_t)idx_ws) & 15) == 0, "geo_indices: idx_ws must be 16-byte aligned");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * n, pairs = rows * n;
  hipLaunchKernelGGL(geo_knn_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, points, n, angle_k, knn_ws, rows);
  SAM6D_LAUNCH_CHECK_CONT("geo_indices(knn)");
  hipLaunchKernelGGL(geo_index_kernel, dim3((unsigned)(((long)n * n + 255) / 256), (unsigned)B), dim3(256), 0, s, points, knn_ws,
                     n, sigma_d, factor_a, reinterpret_cast<float4*>(idx_ws), pairs, knn_ws + rows * angle_k);
  SAM6D_LAUNCH_CHECK("geo_indices");
}

extern "C" int sam6d_geo_embed(const float* idx_ws, long pairs, const float* div_term, const float* Wd, const float* bd,
                               const float* Wa, const float* ba, int hidden, const int* flag, int only_if_large, float* out,
                               void* stream) {
  SAM6D_REQUIRE(idx_ws && div_term && Wd && bd && Wa && ba && out && flag, "geo_embed: null pointer");
  SAM6D_REQUIRE(hidden == 256 && pairs >= 0, "geo_embed: hidden_dim must be 256");
  SAM6D_REQUIRE((((size_t)idx_ws | (size_t)Wd | (size_t)Wa) & 15) == 0, "geo_embed: idx_ws/weights must be 16-byte aligned");
  if (pairs == 0) return 0;
  // the fallback launch behind the fp16x3 kernel normally has nothing to do: a bounded grid (the kernel strides over the pairs when it has)
  const long g_all = (pairs + GE_P - 1) / GE_P, g_use = (only_if_large && g_all > 4096) ? 4096 : g_all;
  hipLaunchKernelGGL(geo_embed_kernel, dim3((unsigned)g_use), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(idx_ws), div_term, Wd, bd, Wa, ba, out, pairs, flag, only_if_large,
                     (const int*)nullptr, 0);
  SAM6D_LAUNCH_CHECK("geo_embed");
}

extern "C" int sam6d_geo_embedding(const float* points, int B, int n, const float* div_term, const float* Wd,
                                   const float* bd, const float* Wa, const float* ba, float sigma_d, float factor_a,
                                   int angle_k, int hidden, int* knn_ws, float* idx_ws, float* out, void* stream) {
  if (int rc = geo_check(B, n, angle_k, hidden)) return rc;
  if (int rc = sam6d_geo_indices(points, B, n, sigma_d, factor_a, angle_k, knn_ws, idx_ws, stream)) return rc;
  return sam6d_geo_embed(idx_ws, (long)B * n * n, div_term, Wd, bd, Wa, ba, hidden, knn_ws + (long)B * n * angle_k, 0, out,
                         stream);
}
