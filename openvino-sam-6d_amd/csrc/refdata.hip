// ISM's reference data from a template set: what stands between the rendered templates (rgb (T,H,W,3|4) u8, mask (T,H,W) u8) and the
// DINOv2 encoder in ISM/run_inference_custom.py:129-155 (custom templates) and ISM/provider/bop.py:60-83 (BOP templates):
//   boxes   PIL's Image.getbbox() of every mask (or alpha band), on the device: (left, upper, right + 1, lower + 1) over the pixels
//           != 0, (0,0,0,0) for an image without one.  One workgroup per image, per-thread min / max, wave reduction, one LDS step:
//           no atomics and no workspace, so the result does not depend on any order.
//   crops   CropResizePad(224) (ISM/utils/bbox_utils.py:89-126) of every template and its mask in one launch, each template reading
//           its OWN image through its own box (read from the device, no read-back).  The index recipe is crop_source of crop_index.h,
//           the one dino_crop_kernel uses.  Two flavours of the pixel value:
//             custom  rgb = fl32(u8 / 255) * fl32(mask / 255), padding 0           (run_inference_custom.py:138-140; no Normalize there)
//             bop     rgb = (fl32(u8 / 255) - mean) / std, padding (0 - mean) / std (bop.py:72-81: T.Normalize after the padding)
//           and mask = fl32(mask / 255), padding 0, in both.  np.array(u8) / 255 is float64 rounded to fp32 by .float(); for all 256
//           values that equals the fp32 division written here (tests/test_refdata_host.py).  A pure gather: bit-exact.
#include "common.h"
#include "crop_index.h"
#include "../../include/sam6d_hip.h"

#define TPL_BBOX_THREADS 512
#define TPL_BBOX_WAVES (TPL_BBOX_THREADS / 64)

struct TplBox {
  int x0, y0, x1, y1;  // inclusive; x1 = -1: no pixel seen
  __device__ __forceinline__ void take(int y, int x) {
    x0 = min(x0, x);
    y0 = min(y0, y);
    x1 = max(x1, x);
    y1 = max(y1, y);
  }
  __device__ __forceinline__ void merge(const TplBox& o) {
    x0 = min(x0, o.x0);
    y0 = min(y0, o.y0);
    x1 = max(x1, o.x1);
    y1 = max(y1, o.y1);
  }
};

// Pixel p = y W + x of image t is the byte band + t image_stride + p pixel_stride (rows follow one another: a (T,H,W) tensor or one
// band of an interleaved (T,H,W,C) tensor).  With pixel_stride 1 the image is read as 16-byte words between its first and last
// 16-byte boundary and byte by byte before and after; a strided band is read byte by byte.
__global__ __launch_bounds__(TPL_BBOX_THREADS) void tpl_bbox_kernel(const unsigned char* __restrict__ band, int H, int W, long pixel_stride,
                                                                   long image_stride, long long* __restrict__ boxes) {
  __shared__ TplBox red[TPL_BBOX_WAVES];
  const int t = blockIdx.x, tid = threadIdx.x;
  const unsigned char* img = band + (size_t)t * image_stride;
  const int n = H * W;
  TplBox b = {0x7fffffff, 0x7fffffff, -1, -1};
  int head = 0, words = 0;
  if (pixel_stride == 1) {
    head = (int)((16 - ((uintptr_t)img & 15)) & 15);
    if (head > n) head = n;
    words = (n - head) / 16;
    const uint4* w4 = reinterpret_cast<const uint4*>(img + head);
    for (int k = tid; k < words; k += TPL_BBOX_THREADS) {
      const uint4 v = w4[k];
      if ((v.x | v.y | v.z | v.w) == 0u) continue;
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      const int p0 = head + 16 * k;
      int y = p0 / W, x = p0 - y * W;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if ((w[e >> 2] >> (8 * (e & 3))) & 0xffu) b.take(y, x);
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
  }
  // the bytes the words do not cover: [0, head) and [head + 16 words, n); all of them for a strided band (head = words = 0)
  const int tail0 = head + 16 * words;
  for (int q = tid; q < head + (n - tail0); q += TPL_BBOX_THREADS) {
    const int p = q < head ? q : tail0 + (q - head);
    if (img[(size_t)p * pixel_stride]) {
      const int y = p / W;
      b.take(y, p - y * W);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    TplBox c;
    c.x0 = __shfl_xor(b.x0, o, 64);
    c.y0 = __shfl_xor(b.y0, o, 64);
    c.x1 = __shfl_xor(b.x1, o, 64);
    c.y1 = __shfl_xor(b.y1, o, 64);
    b.merge(c);
  }
  if (lane_id() == 0) red[wave_id()] = b;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < TPL_BBOX_WAVES; ++w) b.merge(red[w]);
    const bool any = b.x1 >= 0;
    long long* o = boxes + 4 * (size_t)t;
    o[0] = any ? b.x0 : 0;
    o[1] = any ? b.y0 : 0;
    o[2] = any ? b.x1 + 1 : 0;
    o[3] = any ? b.y1 + 1 : 0;
  }
}

extern "C" int sam6d_template_boxes(const unsigned char* band, int T, int H, int W, long pixel_stride, long image_stride, long long* boxes,
                                    void* stream) {
  SAM6D_REQUIRE(band && boxes, "template_boxes: null pointer");
  SAM6D_REQUIRE(T >= 0 && T <= 65535, "template_boxes: T <= 65535 (got %d)", T);
  SAM6D_REQUIRE(H > 0 && W > 0 && (long)H * W <= 2147483647L / 4, "template_boxes: bad image size %d x %d", H, W);
  SAM6D_REQUIRE(pixel_stride >= 1 && pixel_stride <= 64 && image_stride >= 0, "template_boxes: bad strides (pixel %ld, image %ld)",
                pixel_stride, image_stride);
  if (T == 0) return 0;
  hipLaunchKernelGGL(tpl_bbox_kernel, dim3(T), dim3(TPL_BBOX_THREADS), 0, (hipStream_t)stream, band, H, W, pixel_stride, image_stride, boxes);
  SAM6D_LAUNCH_CHECK("template_boxes");
}

// One thread per output pixel of one template.  rgb: channel c of pixel p of template t at rgb + t rgb_image + p rgb_pixel + c;
// mask: pixel p at mask + t mask_image + p mask_pixel.
template <bool BOP>
__global__ __launch_bounds__(256) void tpl_crop_kernel(const unsigned char* __restrict__ rgb, long rgb_pixel, long rgb_image,
                                                       const unsigned char* __restrict__ mask, long mask_pixel, long mask_image,
                                                       const long long* __restrict__ boxes, int H, int W, float* __restrict__ out_rgb,
                                                       float* __restrict__ out_mask) {
  const int t = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= CROP_IMG * CROP_IMG) return;
  const int Y = pix / CROP_IMG, X = pix % CROP_IMG;
  // T.Normalize after the padding (bop.py:81): a padded pixel holds (0 - mean) / std
  float r = BOP ? (0.f - 0.485f) / 0.229f : 0.f, g = BOP ? (0.f - 0.456f) / 0.224f : 0.f, b = BOP ? (0.f - 0.406f) / 0.225f : 0.f;
  float m = 0.f;
  int sy, sx;
  if (crop_source(boxes + 4 * (size_t)t, H, W, Y, X, sy, sx)) {
    const size_t at = (size_t)sy * W + sx;
    if (mask) m = (float)mask[(size_t)t * mask_image + at * mask_pixel] / 255.0f;
    if (out_rgb) {
      const unsigned char* p = rgb + (size_t)t * rgb_image + at * rgb_pixel;
      r = (float)p[0] / 255.0f;
      g = (float)p[1] / 255.0f;
      b = (float)p[2] / 255.0f;
      if (BOP) {  // sub_(mean).div_(std) of T.Normalize, fp32
        r = (r - 0.485f) / 0.229f;
        g = (g - 0.456f) / 0.224f;
        b = (b - 0.406f) / 0.225f;
      } else {    // image * mask[:, :, None] (run_inference_custom.py:140)
        r = r * m;
        g = g * m;
        b = b * m;
      }
    }
  }
  if (out_rgb) {
    float* o = out_rgb + (size_t)t * 3 * CROP_IMG * CROP_IMG + pix;
    o[0] = r;
    o[CROP_IMG * CROP_IMG] = g;
    o[2 * CROP_IMG * CROP_IMG] = b;
  }
  if (out_mask) out_mask[(size_t)t * CROP_IMG * CROP_IMG + pix] = m;
}

extern "C" int sam6d_template_crops(const unsigned char* rgb, long rgb_pixel_stride, long rgb_image_stride, const unsigned char* mask,
                                    long mask_pixel_stride, long mask_image_stride, const long long* boxes, int T, int H, int W,
                                    int flavour, float* out_rgb, float* out_mask, void* stream) {
  SAM6D_REQUIRE(flavour == SAM6D_TEMPLATE_CUSTOM || flavour == SAM6D_TEMPLATE_BOP, "template_crops: unknown flavour %d", flavour);
  SAM6D_REQUIRE(boxes && (out_rgb || out_mask) && (rgb || !out_rgb), "template_crops: null pointer");
  // the mask is read for out_mask, and for the product of the custom flavour
  SAM6D_REQUIRE(mask || !(out_mask || flavour == SAM6D_TEMPLATE_CUSTOM), "template_crops: null pointer (mask)");
  SAM6D_REQUIRE(T >= 0 && T <= 65535, "template_crops: T <= 65535 (got %d)", T);
  SAM6D_REQUIRE(H > 0 && W > 0 && (long)H * W <= 2147483647L / 4, "template_crops: bad image size %d x %d", H, W);
  SAM6D_REQUIRE(!out_rgb || (rgb_pixel_stride >= 3 && rgb_pixel_stride <= 64 && rgb_image_stride >= 0),
                "template_crops: bad rgb strides (pixel %ld, image %ld)", rgb_pixel_stride, rgb_image_stride);
  SAM6D_REQUIRE(!mask || (mask_pixel_stride >= 1 && mask_pixel_stride <= 64 && mask_image_stride >= 0),
                "template_crops: bad mask strides (pixel %ld, image %ld)", mask_pixel_stride, mask_image_stride);
  if (T == 0) return 0;
  const dim3 grid((CROP_IMG * CROP_IMG + 255) / 256, T);
  if (flavour == SAM6D_TEMPLATE_BOP)
    hipLaunchKernelGGL(tpl_crop_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, rgb, rgb_pixel_stride, rgb_image_stride, mask,
                       mask_pixel_stride, mask_image_stride, boxes, H, W, out_rgb, out_mask);
  else
    hipLaunchKernelGGL(tpl_crop_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, rgb, rgb_pixel_stride, rgb_image_stride, mask,
                       mask_pixel_stride, mask_image_stride, boxes, H, W, out_rgb, out_mask);
  SAM6D_LAUNCH_CHECK("template_crops");
}
