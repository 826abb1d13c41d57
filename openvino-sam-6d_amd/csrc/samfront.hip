// SAM's image front: the (H, W, 3) uint8 image -> what the image encoder is called on, in one launch.
//
// Reference: ResizeLongestSide.apply_image (ISM/segment_anything/utils/transforms.py:26-31: torchvision's resize of a PIL image, i.e.
// Pillow's ImagingResample with the bilinear filter), the predictor's channel flip (predictor.py:56-58) and Sam.preprocess
// (modeling/sam.py:164-173).  For 8-bit pixels Pillow's resample is integer arithmetic: per axis a table of first source index and
// 22-bit fixed-point coefficients per output index (built in float64 on the host, sam6d_hip/samfront.py `tables`), and per pass
//     byte = min(((1 << 21) + sum_j pixel[lo + j] * k[j]) >> 22, 255)           (pixels and coefficients are never negative)
// horizontal pass first, its result rounded to a byte before the vertical pass reads it.  Then (float(byte) - mean) / std in fp32 (one
// subtraction, one correctly rounded division: the library is built with -ffp-contract=off) and zeros, not normalised zeros, below
// and to the right of the resized image.  A pass whose axis keeps its size is skipped by Pillow; its table is then (k = 1 << 22, 0) per
// output, which returns the pixel, so the kernel has no such case.
//
// One workgroup owns a band of SF_BAND = 16 output rows (one row of patches) and up to SF_CW = 256 output columns.  It runs the horizontal
// pass for the source rows the band needs -- at most 15 s + 2 max(s, 1) + 2 rows at vertical scale s = H / oh, 82 for the 9 taps the
// entry point admits -- and keeps them as bytes in LDS, one plane per channel (SF_PITCH bytes per source row), then runs the vertical
// pass from LDS, normalises and stores.  The intermediate image never reaches memory.  A thread owns four neighbouring output columns
// in both passes: one 32-bit LDS word per source row and channel, one 16-byte store per output row and channel.  Its horizontal taps
// (4 x SF_TAPS coefficients) stay in registers for all source rows; the vertical taps are uniform over a wave and come through the
// scalar cache.  Tables are trusted to be what `tables` makes (first index + taps within the axis), but every index derived from them is
// clamped to the image and to the staged rows, so a wrong table gives wrong pixels, never an access outside the buffers.
// No float arithmetic before the normalisation, no MFMA, no scratch.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define SF_BAND 16
#define SF_CW 256
#define SF_TAPS 9
#define SF_PITCH (3 * SF_CW + 16)  // + 16: source rows that differ by one start four banks apart
#define SF_ROWS_MAX 83             // SF_ROWS_MAX * SF_PITCH <= 64 KiB
#define SF_HALF (1 << 21)
#define SF_SHIFT 22

// table of an axis with `out` outputs and `taps` columns: lo[out], count[out], k[out][taps] (zeros behind the count)
__global__ __launch_bounds__(256) void sam_front_kernel(const unsigned char* __restrict__ img, long row_stride, long image_stride, int H,
                                                        int W, int reverse, const int* __restrict__ xtab, int xtaps, int ow,
                                                        const int* __restrict__ ytab, int ytaps, int oh, float m0, float m1, float m2,
                                                        float s0, float s1, float s2, int side, float* __restrict__ out, int layout,
                                                        int rows_max) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sf_rows[];
  const int q = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r0 = blockIdx.y * SF_BAND, c0 = blockIdx.x * SF_CW, b = blockIdx.z;
  const int x0 = c0 + 4 * q;
  const int rv = min(SF_BAND, oh - r0);         // rows of the band inside the resized image
  const bool inside = rv > 0 && c0 < ow;        // (uniform over the workgroup)
  int y0 = 0, nr = 1;
  if (inside) {
    const int rl = r0 + rv - 1;
    y0 = min(max(ytab[r0], 0), H - 1);
    nr = max(min(min(ytab[rl] + ytab[oh + rl] - y0, rows_max), H - y0), 1);
  }
  // ---- horizontal pass: source rows y0 .. y0 + nr - 1, the thread's four columns, bytes into LDS
  if (inside && x0 < ow) {
    int lo[4], k[4][SF_TAPS];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool real = x0 + i < ow;
      const int xi = real ? x0 + i : ow - 1;
      lo[i] = min(max(xtab[xi], 0), W - 1);
#pragma unroll
      for (int j = 0; j < SF_TAPS; ++j) k[i][j] = (real && j < xtaps) ? xtab[2 * ow + xi * xtaps + j] : 0;
    }
    const unsigned char* base = img + (long)b * image_stride + (long)y0 * row_stride;
    for (int rc = g; rc < 3 * nr; rc += 4) {
      const int row = rc / 3, c = rc - 3 * row;
      const unsigned char* src = base + (long)row * row_stride + (reverse ? 2 - c : c);
      unsigned packed = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int ss = SF_HALF;
#pragma unroll
        for (int j = 0; j < SF_TAPS; ++j)
          if (j < xtaps) ss += (int)src[3 * min(lo[i] + j, W - 1)] * k[i][j];
        packed |= (unsigned)min(ss >> SF_SHIFT, 255) << (8 * i);
      }
      *reinterpret_cast<unsigned*>(sf_rows + row * SF_PITCH + c * SF_CW + 4 * q) = packed;
    }
  }
  __syncthreads();
  // ---- vertical pass from LDS, normalise, store: (output row, channel) pairs dealt to the four waves
  const int gp = side / 16;  // patches per row
  if (x0 >= side) return;    // (the last column range of a side that is no multiple of SF_CW)
  for (int u = g; u < 3 * SF_BAND; u += 4) {
    const int r = u / 3, c = u - 3 * r;
    const int orow = r0 + r;
    float4 o = {0.f, 0.f, 0.f, 0.f};
    if (inside && r < rv && x0 < ow) {
      const int yl = ytab[orow] - y0;
      int a0 = SF_HALF, a1 = SF_HALF, a2 = SF_HALF, a3 = SF_HALF;
#pragma unroll
      for (int j = 0; j < SF_TAPS; ++j)
        if (j < ytaps) {
          const int kk = ytab[2 * oh + orow * ytaps + j];
          const int rr = min(max(yl + j, 0), nr - 1);
          const unsigned p = *reinterpret_cast<const unsigned*>(sf_rows + rr * SF_PITCH + c * SF_CW + 4 * q);
          a0 += (int)(p & 255u) * kk;
          a1 += (int)((p >> 8) & 255u) * kk;
          a2 += (int)((p >> 16) & 255u) * kk;
          a3 += (int)(p >> 24) * kk;
        }
      const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
      o.x = ((float)min(a0 >> SF_SHIFT, 255) - mean) / sd;
      o.y = x0 + 1 < ow ? ((float)min(a1 >> SF_SHIFT, 255) - mean) / sd : 0.f;
      o.z = x0 + 2 < ow ? ((float)min(a2 >> SF_SHIFT, 255) - mean) / sd : 0.f;
      o.w = x0 + 3 < ow ? ((float)min(a3 >> SF_SHIFT, 255) - mean) / sd : 0.f;
    }
    float* dst;
    if (layout == SAM6D_SAM_FRONT_ROWS)
      dst = out + ((long)b * gp * gp + (long)gp * blockIdx.y + (x0 >> 4)) * 768 + c * 256 + r * 16 + (x0 & 15);
    else
      dst = out + (((long)b * 3 + c) * side + orow) * side + x0;
    *reinterpret_cast<float4*>(dst) = o;
  }
}

extern "C" int sam6d_sam_front(const unsigned char* img, long row_stride, long image_stride, int B, int H, int W, int reverse,
                               const int* xtab, int xtaps, const int* ytab, int ytaps, float mean0, float mean1, float mean2, float std0,
                               float std1, float std2, int side, float* out, int layout, void* stream) {
  SAM6D_REQUIRE(img && xtab && ytab && out, "sam_front: null pointer");
  SAM6D_REQUIRE(H >= 1 && W >= 1 && H <= 4096 && W <= 4096, "sam_front: H and W must be 1 .. 4096 (got %d x %d)", H, W);
  SAM6D_REQUIRE(side >= 16 && side <= 1024 && side % 16 == 0, "sam_front: side must be a multiple of 16, 16 .. 1024 (got %d)", side);
  SAM6D_REQUIRE(B >= 0 && B <= 65535, "sam_front: B must be 0 .. 65535");
  SAM6D_REQUIRE(layout == SAM6D_SAM_FRONT_X || layout == SAM6D_SAM_FRONT_ROWS, "sam_front: layout must be 0 (x) or 1 (rows)");
  SAM6D_REQUIRE(row_stride >= 3L * W && image_stride >= 0, "sam_front: row_stride must be >= 3 W and image_stride >= 0");
  SAM6D_REQUIRE((((size_t)out) & 15) == 0 && ((((size_t)xtab) | ((size_t)ytab)) & 3) == 0,
                "sam_front: out must be 16-byte aligned and the tables 4-byte aligned");
  // ResizeLongestSide.get_preprocess_shape (transforms.py:91-102), in double as there
  const double scale = side * 1.0 / (H > W ? H : W);
  const int oh = (int)(H * scale + 0.5), ow = (int)(W * scale + 0.5);
  SAM6D_REQUIRE(oh >= 1 && ow >= 1, "sam_front: a %d x %d image resizes to %d x %d at side %d", H, W, oh, ow, side);
  if (xtaps < 1 || xtaps > SF_TAPS || ytaps < 1 || ytaps > SF_TAPS) {
    sam6d_set_error("sam_front: %d and %d taps per output are not implemented (1 .. %d are: shrinking by up to 4)", xtaps, ytaps, SF_TAPS);
    return SAM6D_ENOTIMPL;
  }
  const double sy = (double)H / oh;
  int rows = (int)(15.0 * sy + 2.0 * (sy > 1.0 ? sy : 1.0) + 3.0);
  rows = rows < H ? rows : H;
  if (rows > SF_ROWS_MAX) {
    sam6d_set_error("sam_front: a band of %d output rows needs %d source rows at vertical scale %.3f (%d fit)", SF_BAND, rows, sy,
                    SF_ROWS_MAX);
    return SAM6D_ENOTIMPL;
  }
  if (B == 0) return 0;
  hipLaunchKernelGGL(sam_front_kernel, dim3(cdiv(side, SF_CW), side / SF_BAND, B), dim3(256), (size_t)rows * SF_PITCH, (hipStream_t)stream,
                     img, row_stride, image_stride, H, W, reverse ? 1 : 0, xtab, xtaps, ow, ytab, ytaps, oh, mean0, mean1, mean2, std0,
                     std1, std2, side, out, layout, rows);
  SAM6D_LAUNCH_CHECK("sam_front");
}
