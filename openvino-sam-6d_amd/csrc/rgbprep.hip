// The `rgb` input of Net.forward built on the device (PEM/run_inference_custom_pytorch.py:344-350 for proposals, :207-212 for
// templates): crop img[y1:y2, x1:x2], reverse the channels, zero the pixels outside the mask, cv2.resize(..., (S, S), INTER_LINEAR),
// then ToTensor + Normalize (:151-153).  Every item of a batch in one launch.
//
// The resize restates OpenCV 4.x cv::resize for CV_8UC3 (imgproc/src/resize.cpp), INTER_LINEAR in 11-bit fixed point:
//   inv_scale = (double)S / w, scale = 1 / inv_scale (double, per axis);
//   fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (sx, fx) = (0, 0); sx >= w - 1 -> (w - 1, 0);
//   a0 = sat_s16(rint((1 - fx) * 2048)), a1 = sat_s16(rint(fx * 2048)); Hx = src[sx] * a0 + src[sx + 1] * a1 (int32);
//   y: the same fy / sy without the clamp, rows clip(sy, 0, h - 1) and clip(sy + 1, 0, h - 1), weights b0 / b1;
//   out = sat_u8((sat_s16(t0 + t1) + 2) >> 2), t_k = (sat_s16(H_k >> 4) * b_k) >> 16.
// That last line is the form of OpenCV's vectorised vertical pass (VResizeLinearVec_32s8u), which covers every pixel of an S = 224
// row on x86; its scalar row tail, (H0 * b0 + H1 * b1 + 2^21) >> 22, can differ by one level and is not reproduced.  A crop of exactly
// 2S x 2S takes OpenCV's INTER_AREA fast path instead: out = (p00 + p01 + p10 + p11 + 2) >> 2.  A crop of S x S is copied.
// Parity is pinned against the numpy restatement in tests/cv2_linear.py and a float64 bilinear, not against OpenCV itself.
//
// Latency-bound byte work, no MFMA.  Workgroup = (block of output rows, item); each wave owns one output row at a time: it stages the
// two source rows it reads (reversed, masked, one packed u32 per pixel) into its own LDS slice, then every lane produces four
// adjacent output columns from the x taps the workgroup built in LDS, and stores them as 16-byte fp32 vectors (coalesced planes).
#include "common.h"
#include "../../include/sam6d_hip.h"

#define RGB_MAX_LDS (64 * 1024)

struct XTap {
  int sx;
  int a;  // a0 in the low 16 bits, a1 in the high 16 bits
};

// sat_s16, sat_s16f, cv_coord: common.h (segresize.hip resizes whole images by the same recipe)

// mask_mode: 0 = no mask (rgb_mask_flag False), 1 = (mask > 0) & (depth > 0) (get_test_data :318), 2 = mask == 255 (_get_template :201)
__device__ __forceinline__ unsigned load_px(const unsigned char* __restrict__ img, int C, int W, int r, int c,
                                            const unsigned char* __restrict__ m, const float* __restrict__ depth, int mask_mode) {
  const size_t p = (size_t)r * W + c;
  bool keep = true;
  if (mask_mode == 1) keep = m[p] > 0 && depth[p] > 0.f;
  else if (mask_mode == 2) keep = m[p] == 255;
  if (!keep) return 0u;
  if (C == 1) {
    const unsigned g = img[p];
    return g | (g << 8) | (g << 16);
  }
  const unsigned char* q = img + p * 3;
  return (unsigned)q[2] | ((unsigned)q[1] << 8) | ((unsigned)q[0] << 16);  // [:, :, ::-1]
}

__device__ __forceinline__ int ch8(unsigned v, int c) { return (int)((v >> (8 * c)) & 255u); }

__device__ __forceinline__ float normalize_px(int v, int c) {
  // transforms.ToTensor then Normalize (torch CPU, fp32): (v / 255 - mean[c]) / std[c] on the already reversed channels
  const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  const float stdv = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
  return ((float)v / 255.f - mean) / stdv;
}

__global__ __launch_bounds__(256) void rgb_crop_resize_kernel(const unsigned char* __restrict__ img, long img_stride, int C, int H,
                                                              int W, const unsigned char* __restrict__ masks, const float* __restrict__ depth,
                                                              int mask_mode, const int* __restrict__ bbox, int S, int rows_per_wg,
                                                              int row_words, float* __restrict__ out, unsigned char* __restrict__ out_u8,
                                                              int* __restrict__ status) {
  extern __shared__ unsigned lds_u32[];
  XTap* taps = (XTap*)lds_u32;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned* rowA = lds_u32 + 2 * S + wave * 2 * row_words;
  unsigned* rowB = rowA + row_words;
  const int i = blockIdx.y;
  const int r0 = bbox[i * 4], r1 = bbox[i * 4 + 1], c0 = bbox[i * 4 + 2], c1 = bbox[i * 4 + 3];
  const bool bad = r0 < 0 || c0 < 0 || r1 > H || c1 > W || r1 < r0 || c1 < c0;
  if (status && blockIdx.x == 0 && threadIdx.x == 0) status[i] = bad ? 1 : 0;
  const int h = bad ? 0 : r1 - r0, w = bad ? 0 : c1 - c0;  // an empty (or rejected) crop: every pixel masked out
  const bool area2 = h == 2 * S && w == 2 * S;             // OpenCV: INTER_LINEAR at exactly 1/2 on both axes runs as INTER_AREA
  const unsigned char* im = img + (size_t)i * img_stride;
  const unsigned char* m = masks ? masks + (size_t)i * H * W : nullptr;
  const double scale_x = w > 0 ? 1.0 / ((double)S / (double)w) : 0.0, scale_y = h > 0 ? 1.0 / ((double)S / (double)h) : 0.0;

  if (w > 0 && !area2) {
    for (int dx = threadIdx.x; dx < S; dx += blockDim.x) {
      int sx;
      float fx;
      cv_coord(dx, scale_x, sx, fx);
      if (sx < 0) fx = 0.f, sx = 0;
      if (sx >= w - 1) fx = 0.f, sx = w - 1;
      const int a0 = sat_s16f((1.f - fx) * 2048.f), a1 = sat_s16f(fx * 2048.f);
      taps[dx].sx = sx;
      taps[dx].a = (a0 & 0xffff) | (a1 << 16);
    }
  }
  __syncthreads();

  const int dy_end = min(S, (blockIdx.x + 1) * rows_per_wg);
  float* oi = out + (size_t)i * 3 * S * S;
  for (int dy0 = blockIdx.x * rows_per_wg; dy0 < dy_end; dy0 += nw) {  // every wave runs the same trip count (barriers below)
    const int dy = dy0 + wave;
    const bool row_on = dy < dy_end && h > 0 && w > 0;
    int ya = 0, yb = 0, b0 = 0, b1 = 0;
    if (row_on) {
      if (area2) {
        ya = 2 * dy;
        yb = ya + 1;
      } else {
        int sy;
        float fy;
        cv_coord(dy, scale_y, sy, fy);
        ya = min(max(sy, 0), h - 1);
        yb = min(max(sy + 1, 0), h - 1);
        b0 = sat_s16f((1.f - fy) * 2048.f);
        b1 = sat_s16f(fy * 2048.f);
      }
      for (int x = lane; x < w; x += 64) {
        rowA[x] = load_px(im, C, W, r0 + ya, c0 + x, m, depth, mask_mode);
        rowB[x] = load_px(im, C, W, r0 + yb, c0 + x, m, depth, mask_mode);
      }
    }
    __syncthreads();
    if (dy < dy_end) {
      for (int q = lane * 4; q < S; q += 256) {
        int v[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int dx = q + k;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[k][c] = 0;
          if (!row_on || dx >= S) continue;
          if (area2) {
            const unsigned p00 = rowA[2 * dx], p01 = rowA[2 * dx + 1], p10 = rowB[2 * dx], p11 = rowB[2 * dx + 1];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[k][c] = (ch8(p00, c) + ch8(p01, c) + ch8(p10, c) + ch8(p11, c) + 2) >> 2;
          } else {
            const XTap t = taps[dx];
            const int a0 = (int)(short)(t.a & 0xffff), a1 = t.a >> 16;
            const int sx1 = a1 != 0 ? t.sx + 1 : t.sx;  // OpenCV reads the second tap only inside the row
            const unsigned pa0 = rowA[t.sx], pa1 = rowA[sx1], pb0 = rowB[t.sx], pb1 = rowB[sx1];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int h0 = ch8(pa0, c) * a0 + (a1 != 0 ? ch8(pa1, c) * a1 : 0);
              const int h1 = ch8(pb0, c) * a0 + (a1 != 0 ? ch8(pb1, c) * a1 : 0);
              const int t0 = (sat_s16(h0 >> 4) * b0) >> 16, t1 = (sat_s16(h1 >> 4) * b1) >> 16;
              v[k][c] = min(max((sat_s16(t0 + t1) + 2) >> 2, 0), 255);
            }
          }
        }
        const size_t o = (size_t)dy * S + q;
        if ((S & 3) == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float4 f;
            f.x = normalize_px(v[0][c], c);
            f.y = normalize_px(v[1][c], c);
            f.z = normalize_px(v[2][c], c);
            f.w = normalize_px(v[3][c], c);
            *(float4*)(oi + (size_t)c * S * S + o) = f;
          }
          if (out_u8) {
            unsigned* o8 = (unsigned*)(out_u8 + ((size_t)i * S * S + o) * 3);
            o8[0] = (unsigned)v[0][0] | ((unsigned)v[0][1] << 8) | ((unsigned)v[0][2] << 16) | ((unsigned)v[1][0] << 24);
            o8[1] = (unsigned)v[1][1] | ((unsigned)v[1][2] << 8) | ((unsigned)v[2][0] << 16) | ((unsigned)v[2][1] << 24);
            o8[2] = (unsigned)v[2][2] | ((unsigned)v[3][0] << 8) | ((unsigned)v[3][1] << 16) | ((unsigned)v[3][2] << 24);
          }
        } else {
          for (int k = 0; k < 4 && q + k < S; ++k)
            for (int c = 0; c < 3; ++c) {
              oi[(size_t)c * S * S + o + k] = normalize_px(v[k][c], c);
              if (out_u8) out_u8[((size_t)i * S * S + o + k) * 3 + c] = (unsigned char)v[k][c];
            }
        }
      }
    }
    __syncthreads();  // the next row's staging overwrites this wave's slice
  }
}

extern "C" int sam6d_rgb_crop_resize(const unsigned char* images, long image_stride, int channels, int H, int W, const unsigned char* masks,
                                     const float* depth, int mask_mode, int N, const int* bbox, int img_size, float* out,
                                     unsigned char* out_u8, int* status, void* stream) {
  SAM6D_REQUIRE(images && bbox && out, "rgb_crop_resize: null pointer");
  SAM6D_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "rgb_crop_resize: mask_mode must be 0, 1 or 2");
  SAM6D_REQUIRE(mask_mode == 0 || masks, "rgb_crop_resize: masks required for mask_mode %d", mask_mode);
  SAM6D_REQUIRE(mask_mode != 1 || depth, "rgb_crop_resize: depth required for mask_mode 1");
  SAM6D_REQUIRE(channels == 1 || channels == 3, "rgb_crop_resize: channels must be 1 or 3");
  SAM6D_REQUIRE(N >= 0 && H > 0 && W > 0 && image_stride >= 0 && img_size > 0 && img_size <= 1024, "rgb_crop_resize: bad sizes");
  if (N == 0) return 0;
  // one u32 per pixel of the two staged rows of each wave, plus the x taps: 4 waves while that fits in 64 KiB, else fewer
  const int row_words = W + 1;
  int nw = 4;
  while (nw > 1 && (size_t)(2 * img_size + nw * 2 * row_words) * 4 > RGB_MAX_LDS) nw >>= 1;
  const size_t lds = (size_t)(2 * img_size + nw * 2 * row_words) * 4;
  SAM6D_REQUIRE(lds <= RGB_MAX_LDS, "rgb_crop_resize: image width %d too large for the staged rows", W);
  const int rows_per_wg = 16;
  const dim3 grid((unsigned)cdiv(img_size, rows_per_wg), (unsigned)N);
  hipLaunchKernelGGL(rgb_crop_resize_kernel, grid, dim3(64 * nw), lds, (hipStream_t)stream, images, image_stride, channels, H, W, masks,
                     depth, mask_mode, bbox, img_size, rows_per_wg, row_words, out, out_u8, status);
  SAM6D_LAUNCH_CHECK("rgb_crop_resize");
}
