// SAM's automatic mask generator after the mask decoder (ISM/segment_anything/automatic_mask_generator.py:266-321 _process_batch,
// ISM/segment_anything/modeling/sam.py:133-162 postprocess_masks, ISM/segment_anything/utils/amg.py:156-176 calculate_stability_score,
// :303-346 batched_mask_to_box, :255-264 uncrop_masks, ISM/model/sam.py:146-148).  Everything those steps compute is a pure function of
// the low-resolution logits, so nothing of the S x S or the full-resolution logit tensors is ever written: one pass over the output
// pixels forms each value from its low-resolution taps in LDS, thresholds it three times and leaves two counts, an area, a box and the
// bit-packed binary mask.
//
// THE VALUE OF A PIXEL (fp32, source order, -ffp-contract=off; a function of (mask, y, x) alone, whatever the tiling):
//   tap(scale, dst, n):  src = max(0, scale * (dst + 0.5f) - 0.5f);  i0 = (int)src;  i1 = i0 + (i0 < n - 1);  l1 = src - i0;  l0 = 1 - l1
//   scales (torch's area_pixel_compute_scale, no scale_factor given): s1h = (float)lh / S, s1w = (float)lw / S, s2h = (float)in_h / out_h,
//   s2w = (float)in_w / out_w
//   G(Y, X)  = h0 * (w0 * low[r0][c0] + w1 * low[r0][c1]) + h1 * (w0 * low[r1][c0] + w1 * low[r1][c1])
//              with (r0, r1, h0, h1) = tap(s1h, Y, lh), (c0, c1, w0, w1) = tap(s1w, X, lw)               -- the first interpolate, S x S grid
//   v(y, x)  = H0 * (W0 * G(Y0, X0) + W1 * G(Y0, X1)) + H1 * (W0 * G(Y1, X0) + W1 * G(Y1, X1))
//              with (Y0, Y1, H0, H1) = tap(s2h, y, in_h), (X0, X1, W0, W1) = tap(s2w, x, in_w)            -- the second, on [:in_h, :in_w]
// which is upsample_bilinear2d's expression (ATen UpSampleBilinear2d.cu) applied twice; the upper tap of the second stage clamps at
// in_h - 1 / in_w - 1, the cropped window's edge.  The four G values are recomputed per pixel from LDS (16 reads); a band's S-grid rows
// would need 27 rows x 1024 floats at 480 <- 768, more LDS than the ten low-resolution rows they come from.
//
// Tiling: workgroup (band, mask), 256 threads; a band is `band` output rows (16 unless the low-resolution rows of 16 would not fit 48 KB
// of LDS).  Thread t owns columns t, t + 256, ...: the six column taps stay in registers down the band, the row taps of the band sit in
// LDS.  A wave's 64 predicates become two words of the packed mask through one ballot.  Per-band partial counts and box corners go to
// a workspace; a second small kernel adds them up in band order (integers: any order gives the same result).
#include "common.h"
#include "../../include/sam6d_hip.h"

#define AMG_THREADS 256
#define AMG_BAND 16
#define AMG_LDS_BYTES (48 * 1024)
#define AMG_BIG 0x7fffffff

// amg_tap: common.h (segresize.hip samples with the same tap)

// first and last low-resolution row that output rows [y0, y1) read
__host__ __device__ __forceinline__ void amg_band_rows(int y0, int y1, int lh, int S, int in_h, int out_h, int& r_lo, int& r_hi) {
  const float s1h = (float)lh / (float)S, s2h = (float)in_h / (float)out_h;
  int a, b, c, d;
  float f, g;
  amg_tap(s2h, y0, in_h, a, b, f, g);
  amg_tap(s1h, a, lh, r_lo, d, f, g);
  amg_tap(s2h, y1 - 1, in_h, a, b, f, g);
  amg_tap(s1h, b, lh, c, r_hi, f, g);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(AMG_THREADS) void amg_stats_kernel(const float* __restrict__ low, const unsigned char* __restrict__ live, int lh,
                                                                int lw, int S, int in_h, int in_w, int out_h, int out_w, int band,
                                                                int cap_rows, float thr, float thr_hi, float thr_lo,
                                                                unsigned* __restrict__ bits, float* __restrict__ logits_out,
                                                                int* __restrict__ partial) {
  extern __shared__ float L[];          // the band's low-resolution rows, (nrows, lw)
  __shared__ int4 row_i[AMG_BAND];      // per output row of the band: LDS offsets of rows r0, r1 of Y0 and of Y1
  __shared__ float4 row_h[AMG_BAND];    // ... their weights h0, h1 (Y0), h0, h1 (Y1)
  __shared__ float2 row_H[AMG_BAND];    // ... H0, H1
  __shared__ int red[AMG_THREADS / 64][8];
  const int m = blockIdx.y, bnd = blockIdx.x, t = threadIdx.x;
  if (!live[m]) return;  // workgroup-uniform: a mask the IoU filter dropped costs one byte read
  const int y_beg = bnd * band, y_end = min(out_h, y_beg + band);
  const float s1h = (float)lh / (float)S, s1w = (float)lw / (float)S;
  const float s2h = (float)in_h / (float)out_h, s2w = (float)in_w / (float)out_w;
  int r_lo, r_hi;
  amg_band_rows(y_beg, y_end, lh, S, in_h, out_h, r_lo, r_hi);
  const int nrows = min(r_hi - r_lo + 1, cap_rows);
  const float* src = low + ((size_t)m * lh + r_lo) * lw;
  for (int i = t; i < nrows * lw; i += AMG_THREADS) L[i] = src[i];
  if (t < y_end - y_beg) {
    int Y0, Y1, a0, a1, b0, b1;
    float H0, H1, ha0, ha1, hb0, hb1;
    amg_tap(s2h, y_beg + t, in_h, Y0, Y1, H0, H1);
    amg_tap(s1h, Y0, lh, a0, a1, ha0, ha1);
    amg_tap(s1h, Y1, lh, b0, b1, hb0, hb1);
    const int top = nrows - 1;
    row_i[t] = make_int4(min(max(a0 - r_lo, 0), top) * lw, min(max(a1 - r_lo, 0), top) * lw, min(max(b0 - r_lo, 0), top) * lw,
                         min(max(b1 - r_lo, 0), top) * lw);
    row_h[t] = make_float4(ha0, ha1, hb0, hb1);
    row_H[t] = make_float2(H0, H1);
  }
  __syncthreads();

  int n_hi = 0, n_lo = 0, area = 0, x_min = AMG_BIG, x_max = -1, y_min = AMG_BIG, y_max = -1;
  const int wd = (out_w + 31) >> 5, wpad = (out_w + 63) & ~63;
  unsigned* brow = bits + (size_t)m * out_h * wd;
  for (int x = t; x < wpad; x += AMG_THREADS) {  // wave-uniform trip count (wpad is a multiple of 64)
    const bool active = x < out_w;
    int X0, X1, ca0, ca1, cb0, cb1;
    float W0, W1, wa0, wa1, wb0, wb1;
    amg_tap(s2w, active ? x : out_w - 1, in_w, X0, X1, W0, W1);
    amg_tap(s1w, X0, lw, ca0, ca1, wa0, wa1);
    amg_tap(s1w, X1, lw, cb0, cb1, wb0, wb1);
    for (int y = y_beg; y < y_end; ++y) {
      const int4 ri = row_i[y - y_beg];
      const float4 rh = row_h[y - y_beg];
      const float2 rH = row_H[y - y_beg];
      const float* A0 = L + ri.x;
      const float* A1 = L + ri.y;
      const float* B0 = L + ri.z;
      const float* B1 = L + ri.w;
      const float g00 = rh.x * (wa0 * A0[ca0] + wa1 * A0[ca1]) + rh.y * (wa0 * A1[ca0] + wa1 * A1[ca1]);
      const float g01 = rh.x * (wb0 * A0[cb0] + wb1 * A0[cb1]) + rh.y * (wb0 * A1[cb0] + wb1 * A1[cb1]);
      const float g10 = rh.z * (wa0 * B0[ca0] + wa1 * B0[ca1]) + rh.w * (wa0 * B1[ca0] + wa1 * B1[ca1]);
      const float g11 = rh.z * (wb0 * B0[cb0] + wb1 * B0[cb1]) + rh.w * (wb0 * B1[cb0] + wb1 * B1[cb1]);
      const float v = rH.x * (W0 * g00 + W1 * g01) + rH.y * (W0 * g10 + W1 * g11);
      const bool on = active && v > thr;
      const unsigned long long word = __ballot(on);
      const int w0 = (x & ~63) >> 5;
      if ((t & 63) == 0 && w0 < wd) brow[(size_t)y * wd + w0] = (unsigned)word;
      if ((t & 63) == 32 && w0 + 1 < wd) brow[(size_t)y * wd + w0 + 1] = (unsigned)(word >> 32);
      if (active) {
        if (logits_out) logits_out[((size_t)m * out_h + y) * out_w + x] = v;
        n_hi += v > thr_hi;
        n_lo += v > thr_lo;
        if (on) {
          ++area;
          x_min = min(x_min, x);
          x_max = max(x_max, x);
          y_min = min(y_min, y);
          y_max = max(y_max, y);
        }
      }
    }
  }
  n_hi = wave_sum_i(n_hi);
  n_lo = wave_sum_i(n_lo);
  area = wave_sum_i(area);
  x_min = wave_min_i(x_min);
  y_min = wave_min_i(y_min);
  x_max = wave_max_i(x_max);
  y_max = wave_max_i(y_max);
  if ((t & 63) == 0) {
    int* r = red[t >> 6];
    r[0] = n_hi, r[1] = n_lo, r[2] = area, r[3] = x_min, r[4] = y_min, r[5] = x_max, r[6] = y_max;
  }
  __syncthreads();
  if (t == 0) {
    int* p = partial + ((size_t)m * gridDim.x + bnd) * 8;
    for (int w = 1; w < AMG_THREADS / 64; ++w) {
      red[0][0] += red[w][0], red[0][1] += red[w][1], red[0][2] += red[w][2];
      red[0][3] = min(red[0][3], red[w][3]), red[0][4] = min(red[0][4], red[w][4]);
      red[0][5] = max(red[0][5], red[w][5]), red[0][6] = max(red[0][6], red[w][6]);
    }
    for (int k = 0; k < 7; ++k) p[k] = red[0][k];
  }
}

// band partials -> n_hi, n_lo, area, box; an empty mask gets batched_mask_to_box's [0, 0, 0, 0]
__global__ __launch_bounds__(64) void amg_reduce_kernel(const int* __restrict__ partial, const unsigned char* __restrict__ live, int M,
                                                        int nbands, int* __restrict__ n_hi, int* __restrict__ n_lo, int* __restrict__ area,
                                                        int* __restrict__ box) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= M || !live[m]) return;
  int hi = 0, lo = 0, ar = 0, x0 = AMG_BIG, y0 = AMG_BIG, x1 = -1, y1 = -1;
  for (int b = 0; b < nbands; ++b) {
    const int* p = partial + ((size_t)m * nbands + b) * 8;
    hi += p[0], lo += p[1], ar += p[2];
    x0 = min(x0, p[3]), y0 = min(y0, p[4]), x1 = max(x1, p[5]), y1 = max(y1, p[6]);
  }
  n_hi[m] = hi, n_lo[m] = lo, area[m] = ar;
  const bool empty = ar == 0;
  box[4 * m + 0] = empty ? 0 : x0;
  box[4 * m + 1] = empty ? 0 : y0;
  box[4 * m + 2] = empty ? 0 : x1;
  box[4 * m + 3] = empty ? 0 : y1;
}

// rows of output per workgroup and the most low-resolution rows a band touches (the same fp32 taps as the kernel, on the host)
static int amg_plan(int lh, int lw, int S, int in_h, int out_h, int* cap_rows) {
  for (int band = AMG_BAND; band >= 1; band >>= 1) {
    int cap = 0;
    for (int y0 = 0; y0 < out_h; y0 += band) {
      int lo, hi;
      amg_band_rows(y0, y0 + band < out_h ? y0 + band : out_h, lh, S, in_h, out_h, lo, hi);
      if (hi - lo + 1 > cap) cap = hi - lo + 1;
    }
    if ((size_t)cap * lw * sizeof(float) <= AMG_LDS_BYTES) {
      *cap_rows = cap;
      return band;
    }
  }
  return 0;
}

static bool amg_sizes_ok(int lh, int lw, int S, int in_h, int in_w, int out_h, int out_w) {
  return lh > 0 && lw > 0 && lh <= 4096 && lw <= 4096 && S > 0 && S <= 16384 && in_h > 0 && in_w > 0 && in_h <= S && in_w <= S && out_h > 0 &&
         out_w > 0 && out_h <= 16384 && out_w <= 16384;
}

extern "C" size_t sam6d_amg_mask_stats_workspace_bytes(int M, int lh, int lw, int S, int in_h, int out_h) {
  if (M <= 0 || !amg_sizes_ok(lh, lw, S, in_h, 1, out_h, 1)) return 0;
  int cap = 0;
  const int band = amg_plan(lh, lw, S, in_h, out_h, &cap);
  if (band == 0) return 0;
  return (size_t)M * cdiv(out_h, band) * 8 * sizeof(int);
}

extern "C" int sam6d_amg_mask_stats(const float* low, const unsigned char* live, int M, int lh, int lw, int S, int in_h, int in_w, int out_h,
                                    int out_w, float mask_threshold, float stability_score_offset, int* n_hi, int* n_lo, int* area, int* box,
                                    unsigned* bits, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
  SAM6D_REQUIRE(M >= 0 && M <= 65535, "amg_mask_stats: M <= 65535 (got %d)", M);
  SAM6D_REQUIRE(amg_sizes_ok(lh, lw, S, in_h, in_w, out_h, out_w), "amg_mask_stats: bad sizes: low %d x %d, S %d, input %d x %d, output %d x %d",
                lh, lw, S, in_h, in_w, out_h, out_w);
  if (M == 0) return 0;
  SAM6D_REQUIRE(low && live && n_hi && n_lo && area && box && bits && ws, "amg_mask_stats: null pointer");
  int cap = 0;
  const int band = amg_plan(lh, lw, S, in_h, out_h, &cap);
  if (band == 0) {
    sam6d_set_error("amg_mask_stats: one output row of %d <- %d <- %d reads more low-resolution rows than fit %d bytes of LDS", out_h, in_h, lh,
                    AMG_LDS_BYTES);
    return SAM6D_ENOTIMPL;
  }
  const int nbands = cdiv(out_h, band);
  SAM6D_REQUIRE(ws_bytes >= (size_t)M * nbands * 8 * sizeof(int), "amg_mask_stats: workspace too small");
  // `masks > (thr + offset)`: the sum is formed in double (two Python floats) and compared in the tensor's fp32
  const float thr_hi = (float)((double)mask_threshold + (double)stability_score_offset);
  const float thr_lo = (float)((double)mask_threshold - (double)stability_score_offset);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(amg_stats_kernel, dim3(nbands, M), dim3(AMG_THREADS), (size_t)cap * lw * sizeof(float), s, low, live, lh, lw, S, in_h, in_w,
                     out_h, out_w, band, cap, mask_threshold, thr_hi, thr_lo, bits, logits_out, (int*)ws);
  SAM6D_LAUNCH_CHECK_CONT("amg_mask_stats");
  hipLaunchKernelGGL(amg_reduce_kernel, dim3(cdiv(M, 64)), dim3(64), 0, s, (const int*)ws, live, M, nbands, n_hi, n_lo, area, box);
  SAM6D_LAUNCH_CHECK("amg_mask_stats");
}

// ---- survivors: packed rows -> (K, H, W) masks in the image frame ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void amg_unpack_kernel(const unsigned* __restrict__ bits, const long long* __restrict__ idx, long n_src,
                                                         int out_h, int out_w, int x0, int y0, int H, int W, T* __restrict__ out) {
  const int k = blockIdx.y;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int cy = y - y0, cx = x - x0;
  const long row = idx[k];
  unsigned v = 0;
  if (row >= 0 && row < n_src && cy >= 0 && cy < out_h && cx >= 0 && cx < out_w) {
    const int wd = (out_w + 31) >> 5;
    v = (bits[((size_t)row * out_h + cy) * wd + (cx >> 5)] >> (cx & 31)) & 1u;
  }
  out[(size_t)k * H * W + p] = (T)v;
}

extern "C" int sam6d_amg_unpack_masks(const unsigned* bits, const long long* idx, long n_src, int K, int out_h, int out_w, int x0, int y0,
                                      int H, int W, int as_f32, void* out, void* stream) {
  SAM6D_REQUIRE(K >= 0 && K <= 65535, "amg_unpack_masks: K <= 65535 (got %d)", K);
  SAM6D_REQUIRE(out_h > 0 && out_w > 0 && H > 0 && W > 0 && n_src >= 0 && (long)H * W <= 2147483647L, "amg_unpack_masks: bad sizes");
  SAM6D_REQUIRE(x0 >= 0 && y0 >= 0 && x0 + out_w <= W && y0 + out_h <= H, "amg_unpack_masks: crop %d x %d at (%d, %d) leaves the %d x %d image",
                out_h, out_w, x0, y0, H, W);
  if (K == 0) return 0;
  SAM6D_REQUIRE(bits && idx && out, "amg_unpack_masks: null pointer");
  const dim3 grid((unsigned)(((long)H * W + 255) / 256), K);
  hipStream_t s = (hipStream_t)stream;
  if (as_f32)
    hipLaunchKernelGGL(amg_unpack_kernel<float>, grid, dim3(256), 0, s, bits, idx, n_src, out_h, out_w, x0, y0, H, W, (float*)out);
  else
    hipLaunchKernelGGL(amg_unpack_kernel<unsigned char>, grid, dim3(256), 0, s, bits, idx, n_src, out_h, out_w, x0, y0, H, W,
                       (unsigned char*)out);
  SAM6D_LAUNCH_CHECK("amg_unpack_masks");
}
