// The two resizes `segmentor_width_size` puts round the mask generator (ISM/model/sam.py:77-83 preprocess_resize, :85-100
// postprocess_resize): the image is shrunk to the segmentor's width with cv2.resize before SAM sees it, and every surviving mask is
// blown back up to the image's size with F.interpolate(..., mode="bilinear", align_corners=False).
//
// THE IMAGE (seg_image_resize_kernel) is cv2.resize(src, (w, h)), default INTER_LINEAR, for CV_8UC3 as OpenCV 4.x computes it
// (imgproc/src/resize.cpp): the recipe at the top of rgbprep.hip, for a whole rectangular image with a scale per axis.
//   scale = 1.0 / ((double)n_out / n) per axis; f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s;
//   x: s < 0 -> (0, 0), s >= W - 1 -> (W - 1, 0); a0 = sat_s16(rint((1 - f) * 2048)), a1 = sat_s16(rint(f * 2048)),
//      Hx = src[s] * a0 + src[min(s + 1, W - 1)] * a1 (int32; a1 is 0 wherever s + 1 leaves the row);
//   y: no clamp of (s, f), rows clip(s, 0, H - 1) and clip(s + 1, 0, H - 1), b0 / b1 likewise;
//   out = sat_u8((sat_s16(t0 + t1) + 2) >> 2), t_k = (sat_s16(H_k >> 4) * b_k) >> 16      (the vectorised vertical pass, every column).
// H == 2 h and W == 2 w runs as INTER_AREA, the rounded 2 x 2 mean (p00 + p01 + p10 + p11 + 2) >> 2; equal sizes copy.
// Integers throughout; the coordinates are formed per thread with the float operations named above.  One launch: a thread owns four
// neighbouring output pixels of one row (12 bytes, three whole words where the row's offset allows).  At most 6 MB in, latency-bound.
//
// THE MASKS (seg_masks_resize_kernel): (K, h, w) bytes, any non-zero byte = 1, -> (K, H, W) fp32,
//   v(y, x) = H0 * (W0 * m[Y0][X0] + W1 * m[Y0][X1]) + H1 * (W0 * m[Y1][X0] + W1 * m[Y1][X1])
//   with (Y0, Y1, H0, H1) = amg_tap((float)h / H, y, h), (X0, X1, W0, W1) = amg_tap((float)w / W, x, w)          (common.h)
// in fp32, source order, -ffp-contract=off: upsample_bilinear2d's expression, a function of (mask, y, x) alone.  Enlarging or
// shrinking alike (two taps per axis; torch does not antialias here).
// The launch is bound by its output: 4 bytes written per pixel against 1/9 byte read at 3x.  Workgroup = one wave = (256 columns, band
// of 16 output rows, mask): measured, 1024 columns per workgroup left most of a 1280-wide row's second workgroup idle (0.27 ms
// against 0.18 ms for 200 masks at 960 x 1280).  A thread owns four neighbouring columns, keeps their x taps in registers down the
// band and issues one 16-byte non-temporal store per row (the result is far larger than the caches and nothing here reads it).  The
// y taps are the same for the whole wave.  The horizontal sums of the two source rows, W0 * m[r][X0] + W1 * m[r][X1], stay in
// registers for as long as the band's rows read the same source rows (three output rows at 3x), so a source byte is fetched once
// per row change, through the L1 / L2: the band's few source rows are a few hundred bytes per workgroup, no LDS stage is built.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define SEG_THREADS 256      // the image kernel's workgroup
#define SEG_MASK_THREADS 64  // the mask kernel's
#define SEG_BAND 16
#define SEG_IMG_MAX 4096
#define SEG_MASK_MAX 8192

enum { SEG_COPY = 0, SEG_AREA2 = 1, SEG_LINEAR = 2 };

__global__ __launch_bounds__(SEG_THREADS) void seg_image_resize_kernel(const unsigned char* __restrict__ src, long row_stride, int H, int W,
                                                                       unsigned char* __restrict__ dst, int h, int w, int mode,
                                                                       double scale_x, double scale_y, int dst_words) {
  const int y = blockIdx.y, q = 4 * (blockIdx.x * SEG_THREADS + threadIdx.x);
  if (q >= w) return;
  int v[4][3];
  if (mode == SEG_LINEAR) {
    int sy;
    float fy;
    cv_coord(y, scale_y, sy, fy);
    const unsigned char* ra = src + (size_t)min(max(sy, 0), H - 1) * row_stride;
    const unsigned char* rb = src + (size_t)min(max(sy + 1, 0), H - 1) * row_stride;
    const int b0 = sat_s16f((1.f - fy) * 2048.f), b1 = sat_s16f(fy * 2048.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int sx;
      float fx;
      cv_coord(min(q + k, w - 1), scale_x, sx, fx);
      if (sx < 0) fx = 0.f, sx = 0;
      if (sx >= W - 1) fx = 0.f, sx = W - 1;
      const int a0 = sat_s16f((1.f - fx) * 2048.f), a1 = sat_s16f(fx * 2048.f);
      const int x0 = 3 * sx, x1 = 3 * min(sx + 1, W - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int h0 = (int)ra[x0 + c] * a0 + (int)ra[x1 + c] * a1;
        const int h1 = (int)rb[x0 + c] * a0 + (int)rb[x1 + c] * a1;
        const int t0 = (sat_s16(h0 >> 4) * b0) >> 16, t1 = (sat_s16(h1 >> 4) * b1) >> 16;
        v[k][c] = min(max((sat_s16(t0 + t1) + 2) >> 2, 0), 255);
      }
    }
  } else if (mode == SEG_AREA2) {
    const unsigned char* ra = src + (size_t)(2 * y) * row_stride;
    const unsigned char* rb = ra + row_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x0 = 6 * min(q + k, w - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = ((int)ra[x0 + c] + (int)ra[x0 + 3 + c] + (int)rb[x0 + c] + (int)rb[x0 + 3 + c] + 2) >> 2;
    }
  } else {
    const unsigned char* ra = src + (size_t)y * row_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[k][c] = ra[3 * min(q + k, w - 1) + c];
  }
  const size_t px = (size_t)y * w + q;
  unsigned char* o = dst + 3 * px;
  if (dst_words && (px & 3) == 0 && q + 3 < w) {  // 12 bytes from a 4-byte boundary
    unsigned* o32 = (unsigned*)o;
    o32[0] = (unsigned)v[0][0] | ((unsigned)v[0][1] << 8) | ((unsigned)v[0][2] << 16) | ((unsigned)v[1][0] << 24);
    o32[1] = (unsigned)v[1][1] | ((unsigned)v[1][2] << 8) | ((unsigned)v[2][0] << 16) | ((unsigned)v[2][1] << 24);
    o32[2] = (unsigned)v[2][2] | ((unsigned)v[3][0] << 8) | ((unsigned)v[3][1] << 16) | ((unsigned)v[3][2] << 24);
  } else {
    for (int k = 0; k < 4 && q + k < w; ++k)
      for (int c = 0; c < 3; ++c) o[3 * k + c] = (unsigned char)v[k][c];
  }
}

extern "C" int sam6d_image_resize_linear(const unsigned char* src, long row_stride, int H, int W, int channels, unsigned char* dst, int h,
                                         int w, void* stream) {
  SAM6D_REQUIRE(channels == 3, "image_resize_linear: the image must have 3 channels (got %d)", channels);
  SAM6D_REQUIRE(H >= 1 && W >= 1 && H <= SEG_IMG_MAX && W <= SEG_IMG_MAX, "image_resize_linear: H and W must be 1 .. %d (got %d x %d)",
                SEG_IMG_MAX, H, W);
  SAM6D_REQUIRE(h >= 1, "image_resize_linear: the output has %d rows: h must be at least 1 (cv2.resize raises for an empty size)", h);
  SAM6D_REQUIRE(w >= 1 && h <= SEG_IMG_MAX && w <= SEG_IMG_MAX, "image_resize_linear: h and w must be 1 .. %d (got %d x %d)", SEG_IMG_MAX, h, w);
  SAM6D_REQUIRE(src && dst, "image_resize_linear: null pointer");
  SAM6D_REQUIRE(row_stride >= 3L * W, "image_resize_linear: row_stride %ld is below 3 W = %d", row_stride, 3 * W);
  const unsigned char* src_end = src + (size_t)(H - 1) * row_stride + 3 * (size_t)W;
  const unsigned char* dst_end = dst + 3 * (size_t)h * w;
  SAM6D_REQUIRE(dst_end <= src || src_end <= dst, "image_resize_linear: the output must not alias the input");
  const int mode = (H == h && W == w) ? SEG_COPY : ((H == 2 * h && W == 2 * w) ? SEG_AREA2 : SEG_LINEAR);
  const double scale_x = 1.0 / ((double)w / (double)W), scale_y = 1.0 / ((double)h / (double)H);
  const dim3 grid(cdiv(cdiv(w, 4), SEG_THREADS), h);
  hipLaunchKernelGGL(seg_image_resize_kernel, grid, dim3(SEG_THREADS), 0, (hipStream_t)stream, src, row_stride, H, W, dst, h, w, mode, scale_x,
                     scale_y, ((uintptr_t)dst & 3) == 0 ? 1 : 0);
  SAM6D_LAUNCH_CHECK("image_resize_linear");
}

// ---- masks ----------------------------------------------------------------------------------------------------------------------------
// the four columns' horizontal sums of one source row
__device__ __forceinline__ void seg_row_sums(const unsigned char* __restrict__ row, const int (&c0)[4], const int (&c1)[4],
                                             const float (&w0)[4], const float (&w1)[4], float (&s)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = w0[j] * (row[c0[j]] ? 1.0f : 0.0f) + w1[j] * (row[c1[j]] ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(SEG_MASK_THREADS) void seg_masks_resize_kernel(const unsigned char* __restrict__ masks, int h, int w, int H, int W,
                                                                       int vec, float* __restrict__ out) {
  const int x = 4 * (blockIdx.x * SEG_MASK_THREADS + threadIdx.x);
  if (x >= W) return;
  const int y_beg = blockIdx.y * SEG_BAND, y_end = min(H, y_beg + SEG_BAND);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  int c0[4], c1[4];
  float w0[4], w1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) amg_tap(sw, min(x + j, W - 1), w, c0[j], c1[j], w0[j], w1[j]);
  const unsigned char* m = masks + (size_t)blockIdx.z * h * w;
  float* o = out + ((size_t)blockIdx.z * H + y_beg) * W + x;
  const bool wide = vec && x + 3 < W;
  float top[4], bot[4];
  int r_top = -1, r_bot = -1;  // the source rows `top` and `bot` hold
  for (int y = y_beg; y < y_end; ++y, o += W) {
    int Y0, Y1;
    float H0, H1;
    amg_tap(sh, y, h, Y0, Y1, H0, H1);  // the same for every thread of the workgroup
    if (Y0 != r_top) {
      if (Y0 == r_bot) {
#pragma unroll
        for (int j = 0; j < 4; ++j) top[j] = bot[j];
      } else {
        seg_row_sums(m + (size_t)Y0 * w, c0, c1, w0, w1, top);
      }
      r_top = Y0;
    }
    if (Y1 != r_bot) {
      if (Y1 == r_top) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bot[j] = top[j];
      } else {
        seg_row_sums(m + (size_t)Y1 * w, c0, c1, w0, w1, bot);
      }
      r_bot = Y1;
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = H0 * top[j] + H1 * bot[j];
    if (wide) {  // non-temporal: up to 1.7 GB written once and read by nobody here (measured: 0.32 ms against 0.48 with plain stores)
      __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(o));
    } else {
      for (int j = 0; j < 4 && x + j < W; ++j) o[j] = v[j];
    }
  }
}

extern "C" int sam6d_masks_resize_bilinear(const unsigned char* masks, int K, int h, int w, int H, int W, float* out, void* stream) {
  SAM6D_REQUIRE(K >= 0 && K <= 65535, "masks_resize_bilinear: K must be 0 .. 65535 (got %d)", K);
  SAM6D_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1 && h <= SEG_MASK_MAX && w <= SEG_MASK_MAX && H <= SEG_MASK_MAX && W <= SEG_MASK_MAX,
                "masks_resize_bilinear: sizes must be 1 .. %d (got %d x %d -> %d x %d)", SEG_MASK_MAX, h, w, H, W);
  if (K == 0) return 0;
  SAM6D_REQUIRE(masks && out, "masks_resize_bilinear: null pointer");
  SAM6D_REQUIRE(((uintptr_t)out & 3) == 0, "masks_resize_bilinear: out must be 4-byte aligned");
  const int vec = (W % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;  // every thread's four floats start on a 16-byte boundary
  const dim3 grid(cdiv(cdiv(W, 4), SEG_MASK_THREADS), cdiv(H, SEG_BAND), K);
  hipLaunchKernelGGL(seg_masks_resize_kernel, grid, dim3(SEG_MASK_THREADS), 0, (hipStream_t)stream, masks, h, w, H, W, vec, out);
  SAM6D_LAUNCH_CHECK("masks_resize_bilinear");
}
