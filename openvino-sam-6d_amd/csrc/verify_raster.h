// What the two translation units that render poses into windows share (verify.hip: the pose check; refine.hip: the point-to-plane
// refinement), one copy of each:
//   vf_window, VfWindowSink, verify_faces_kernel   a pose's window, and the raster pass of verify.hip's RECIPE b into the windows' z-buffer
//                                                  words: raster.h's rs_faces_pass, the pass sam6d_render_views runs, through a sink
//                                                  that clamps to the window -- so a word holds the key that entry computes for the
//                                                  same view and pixel, and refine.hip's z-buffer the keys of sam6d_pose_verify;
//   vf_first_pose, vf_word                         the walk from a window word to its pose and pixel (classify, accumulate);
//   vf_each_pose                                   the loop over the poses present in a wave, for their per-pose reductions.
// The kernel is `inline`: each translation unit that launches it carries its own code object of it.
#pragma once
#include "raster.h"

#define VF_MAX_N 1024
#define VF_EMPTY (~0ull)

// the limits every entry of verify.hip and refine.hip shares, by name and before a launch or a write
static inline int vf_check(const char* who, int V, int F, int N, int H, int W, float near) {
  return rs_limits(who, V, F, "N", N, VF_MAX_N, H, W, near);
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

// the z-buffer words of one window: a face's pixel box is clamped to the window, pixel (y, x) is word off + (y - y0) * bw + (x - x0)
struct VfWindowSink {
  VfWin w;
  unsigned long long* zbuf;
  long long total;
  __device__ __forceinline__ void clamp(RsFace& f) const {
    f.x0 = max(f.x0, w.x0);
    f.y0 = max(f.y0, w.y0);
    f.x1 = min(f.x1, w.x0 + w.bw - 1);
    f.y1 = min(f.y1, w.y0 + w.bh - 1);
  }
  __device__ __forceinline__ void put(int x, int y, unsigned long long key) const {
    const long long word = w.off + (long long)(y - w.y0) * w.bw + (x - w.x0);
    if ((unsigned long long)word >= (unsigned long long)total) return;  // also a negative offset
    __hip_atomic_fetch_min(zbuf + word, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

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
  rs_faces_pass(f, face, vert, V, faces, M, cam, wave_area, VfWindowSink{w, zbuf, total});
}
#pragma clang diagnostic pop

// ---- from a window word to its pose and pixel: one thread per window word of all poses, the grid sized by the sum of the windows
// the last pose whose window starts at or before word `base`, by bisection (a workgroup's first word: every thread searches the same)
__device__ __forceinline__ int vf_first_pose(const long long* __restrict__ offset, int N, long long base) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offset[mid] <= base) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct VfPixel {
  int n;                   // the word's pose
  int x, y;
  size_t p;                // y * W + x
  unsigned long long key;  // the word
  __device__ __forceinline__ float r() const { return __uint_as_float((unsigned)(key >> 32)); }  // the rendered depth: nothing is recomputed
  __device__ __forceinline__ unsigned face() const { return (unsigned)(key & 0xffffffffull); }
};

// Word i of a workgroup whose first word belongs to pose nb (vf_first_pose): steps forward from nb to the word's pose, px.n (nb for a
// word at or beyond total) -> true when the word holds a pixel, with the rest of px set.  An empty word, and a word whose index within
// its pose is outside the window (inconsistent boxes and offsets), hold none.
__device__ __forceinline__ bool vf_word(const unsigned long long* __restrict__ zbuf, long long total, const int* __restrict__ box,
                                        const long long* __restrict__ offset, int N, int H, int W, long long i, int nb, VfPixel& px) {
  int n = nb;
  bool pixel = false;
  if (i < total) {
    while (n + 1 < N && offset[n + 1] <= i) ++n;
    const VfWin w = vf_window(box, offset, n, H, W);
    const long long local = i - w.off;
    px.key = zbuf[i];
    if (px.key != VF_EMPTY && local >= 0 && local < (long long)w.bw * w.bh) {
      px.y = w.y0 + (int)(local / w.bw);
      px.x = w.x0 + (int)(local % w.bw);
      px.p = (size_t)px.y * W + px.x;
      pixel = true;
    }
  }
  px.n = n;
  return pixel;
}

// The poses present in a wave, one after the other (uniform): `has` marks the lanes with something to reduce, n is the lane's pose.
// Calls each(lead, pn, mine, m): pose pn, the lanes of it (`mine`, as a ballot m) and the first of them, lead.  `each` captures by
// value: behind references the compiler reloads what the body's atomics might have changed (classify built 17 instructions longer).
template <class Each>
__device__ __forceinline__ void vf_each_pose(bool has, int n, const Each& each) {
  unsigned long long pending = __ballot(has);
  while (pending) {
    const int lead = __ffsll((long long)pending) - 1;
    const int pn = __shfl(n, lead, 64);
    const bool mine = has && n == pn;
    const unsigned long long m = __ballot(mine);
    pending &= ~m;
    each(lead, pn, mine, m);
  }
}
