// The gather of CropResizePad(224) (ISM/utils/bbox_utils.py:89-126) as one index recipe: which pixel of the image an output pixel of
// the 224 x 224 crop reads, or that it is padding.  One copy, for dino_crop_kernel (csrc/dinov2.hip: one image, N proposals) and
// tpl_crop_kernel (csrc/refdata.hip: every template its own image), so both read the same pixels.
#pragma once
#include <hip/hip_runtime.h>

#define CROP_IMG 224

// F.interpolate(x, scale_factor = s) in the default nearest mode: output size floor(in * s) in double, source index
// min((int) floorf(dst * (float)(1 / s)), in - 1) (ATen upsample_nearest with the scale it was given).
__device__ __forceinline__ int crop_nearest(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// Output pixel (Y, X) of the crop of box = (x1, y1, x2, y2) (int64, exclusive ends) on an H x W image: true and the source pixel
// (sy, sx), or false where the output is padding.  A box with side <= 0, one that lies outside the image or one whose resized crop
// is empty (which raises in the reference) is all padding.
__device__ __forceinline__ bool crop_source(const long long* __restrict__ box, int H, int W, int Y, int X, int& sy, int& sx) {
  const long long bx1 = box[0], by1 = box[1], bx2 = box[2], by2 = box[3];
  // scale_factor = 224 / max(box side) of the (unclamped) box sizes, bbox_utils.py:99-100: a Python number over a tensor, which torch
  // evaluates as tensor.reciprocal() * 224 in fp32 -- two roundings, not one division (for side 3: 74.66667175, not 74.66666412)
  const long long side = (bx2 - bx1) > (by2 - by1) ? (bx2 - bx1) : (by2 - by1);
  const float sf = (1.0f / (float)side) * 224.0f;
  // the slice image[:, y1:y2, x1:x2] (bbox_utils.py:104) ends at the image border
  const int x1 = (int)(bx1 < 0 ? 0 : (bx1 > W ? W : bx1)), x2 = (int)(bx2 < 0 ? 0 : (bx2 > W ? W : bx2));
  const int y1 = (int)(by1 < 0 ? 0 : (by1 > H ? H : by1)), y2 = (int)(by2 < 0 ? 0 : (by2 > H ? H : by2));
  const int cw = x2 - x1, ch = y2 - y1;
  int rw = 0, rh = 0;
  if (side > 0 && cw > 0 && ch > 0) {
    rw = (int)floor((double)cw * (double)sf);
    rh = (int)floor((double)ch * (double)sf);
  }
  if (!(rw > 0 && rh > 0 && rw <= CROP_IMG && rh <= CROP_IMG)) return false;  // (an empty resized crop raises in the reference)
  const float scale1 = (float)(1.0 / (double)sf);
  int py = Y, px = X, pad_t = 0, pad_l = 0;
  if (rw == rh) {
    // square after the resize: no padding (bbox_utils.py:111); the second interpolate maps side rw -> 224.  rw is 223 or 224 for
    // every box side (224 / side is good to 2 ulp), and torch sizes the second output as floor(223 * (224.0 / 223)) = 224, so the
    // 224 pixels written are the reference's (tests/test_dinov2_host.py checks both statements)
    if (rw != CROP_IMG) {
      const float scale2 = (float)(1.0 / (224.0 / (double)rw));
      py = crop_nearest(Y, scale2, rw);
      px = crop_nearest(X, scale2, rw);
    }
  } else {
    pad_t = (CROP_IMG - rh) / 2;
    pad_l = (CROP_IMG - rw) / 2;
  }
  const int ry = py - pad_t, rx = px - pad_l;
  if (!(ry >= 0 && ry < rh && rx >= 0 && rx < rw)) return false;
  sy = y1 + crop_nearest(ry, scale1, ch);
  sx = x1 + crop_nearest(rx, scale1, cw);
  return true;
}
