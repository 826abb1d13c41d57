// What the two translation units that render poses into windows share (verify.hip: the pose check; refine.hip: the point-to-plane
// refinement): a pose's window, and the raster pass of verify.hip's RECIPE b into the windows' z-buffer words.  One copy, so a word of
// refine.hip's z-buffer holds the key sam6d_pose_verify computes for the same view and window, bit for bit.  The kernel is `inline`:
// each translation unit that launches it carries its own code object of it.
#pragma once
#include "raster.h"

#define VF_MAX_N 1024
#define VF_EMPTY (~0ull)

// the limits every entry of verify.hip and refine.hip shares, by name and before a launch or a write
static inline int vf_check(const char* who, int V, int F, int N, int H, int W, float near) {
  SAM6D_REQUIRE(H >= 1 && H <= RS_MAX_HW && W >= 1 && W <= RS_MAX_HW, "%s: H x W = %d x %d is not in 1 .. %d", who, H, W, RS_MAX_HW);
  SAM6D_REQUIRE(N >= 1 && N <= VF_MAX_N, "%s: N = %d is not in 1 .. %d", who, N, VF_MAX_N);
  SAM6D_REQUIRE(F >= 1 && F <= RS_MAX_F, "%s: F = %d is not in 1 .. %d", who, F, RS_MAX_F);
  SAM6D_REQUIRE(V >= 1, "%s: V = %d is not positive", who, V);
  SAM6D_REQUIRE(near > 0.f, "%s: near = %g is not positive", who, (double)near);
  return 0;
}

__device__ __forceinline__ void vf_add(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct VfWin {
  int x0, y0, bw, bh;  // the box clamped to the image; 0 x 0 when empty
  long long off;       // its first word
};

__device__ __forceinline__ VfWin vf_window(const int* __restrict__ box, const long long* __restrict__ offset, int n, int H, int W) {
  const int* b = box + (size_t)n * 4;
  VfWin w;
  w.x0 = max(b[0], 0);
  w.y0 = max(b[1], 0);
  const int x1 = min(b[2], W - 1), y1 = min(b[3], H - 1);
  w.bw = x1 >= w.x0 ? x1 - w.x0 + 1 : 0;  // x0 >= 0 and x1 <= W - 1: no overflow
  w.bh = y1 >= w.y0 ? y1 - w.y0 + 1 : 0;
  if (w.bw == 0 || w.bh == 0) w.bw = w.bh = 0;
  w.off = offset[n];
  return w;
}

// the face's pixel box clamped to the window
__device__ __forceinline__ void vf_clamp(RsFace& f, const VfWin& w) {
  f.x0 = max(f.x0, w.x0);
  f.y0 = max(f.y0, w.y0);
  f.x1 = min(f.x1, w.x0 + w.bw - 1);
  f.y1 = min(f.y1, w.y0 + w.bh - 1);
}

__device__ __forceinline__ void vf_offer(const RsFace& f, int face, int x, int y, const VfWin& w, unsigned long long* __restrict__ zbuf,
                                         long long total) {
  long long w0, w1, w2;
  if (!rs_cover(f, x, y, w0, w1, w2)) return;
  float l0, l1, l2;
  const float d = rs_weights(f, w0, w1, w2, l0, l1, l2);
  const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)face;
  const long long word = w.off + (long long)(y - w.y0) * w.bw + (x - w.x0);
  if ((unsigned long long)word >= (unsigned long long)total) return;  // also a negative offset
  __hip_atomic_fetch_min(zbuf + word, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(F / 64), N), one wave each: raster_faces_kernel into the pose's window.  `inline` gives the kernel and its host stub
// the linkage of a template's instance, one definition per library; clang honours it and only warns that another compiler would not
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(64) void verify_faces_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int F,
                                                                 const float* __restrict__ view, RsCam cam, int wave_area,
                                                                 const int* __restrict__ box, const long long* __restrict__ offset,
                                                                 long long total, unsigned long long* __restrict__ zbuf,
                                                                 int* __restrict__ counts) {
  const int n = blockIdx.y, lane = threadIdx.x;
  const int face = blockIdx.x * 64 + lane;
  const float* M = view + (size_t)n * 12;
  const VfWin w = vf_window(box, offset, n, cam.H, cam.W);
  RsFace f;
  f.live = false;
  f.dropped = false;
  f.x0 = f.y0 = 0;
  f.x1 = f.y1 = -1;
  if (face < F) rs_setup(f, vert, V, faces, face, M, cam);
  const int dropped = __popcll(__ballot(f.dropped));
  if (lane == 0 && dropped) vf_add(counts + (size_t)n * 8 + 7, dropped);
  if (w.bw == 0) return;  // (uniform over the wave)
  vf_clamp(f, w);
  const bool boxed = f.live && f.x0 <= f.x1 && f.y0 <= f.y1;
  const int bw = f.x1 - f.x0 + 1, bh = f.y1 - f.y0 + 1;  // at most 2048 each: the product fits an int
  const bool big = boxed && bw * bh >= wave_area;
  if (boxed && !big)
    for (int y = f.y0; y <= f.y1; ++y)
      for (int x = f.x0; x <= f.x1; ++x) vf_offer(f, face, x, y, w, zbuf, total);
  unsigned long long todo = __ballot(big);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int gface = blockIdx.x * 64 + src;
    RsFace g;
    rs_setup(g, vert, V, faces, gface, M, cam);  // the same code on the same inputs as the owner lane ran: the same face
    vf_clamp(g, w);
    const int gw = g.x1 - g.x0 + 1, cnt = gw * (g.y1 - g.y0 + 1);
    for (int i = lane; i < cnt; i += 64) vf_offer(g, gface, g.x0 + i % gw, g.y0 + i / gw, w, zbuf, total);
  }
}
#pragma clang diagnostic pop
