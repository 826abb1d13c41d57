// What the two translation units of the template renderer share (raster.hip: visibility and the vertex-colour / grey resolve;
// texture.hip: the textured resolve): the face setup, coverage and weights of raster.hip's RECIPE as device functions, so that both
// resolve kernels recompute the winner's weights with the very code the visibility pass ran, and the host side of the visibility
// pass with the refusals in front of it.
#pragma once
#include "common.h"

#define RS_MAX_HW 2048
#define RS_MAX_T 1024
#define RS_MAX_F (1 << 24)
#define RS_WAVE_AREA 256
#define RS_GAIN 25.330296f
#define RS_SNAP_LIMIT 16777216.0f

struct RsCam {
  float fx, fy, cx, cy, near;
  int H, W;
};

struct RsFace {
  int X[3], Y[3];  // snapped screen coordinates, vertices 1 and 2 swapped where the winding asked for it
  float z[3];      // camera depth in that order
  long long area2;
  int b0, b1, b2;  // 0 where the edge opposite the vertex owns its points (top-left), else -1
  int x0, x1, y0, y1;  // pixel bounding box clamped to the image; empty when x0 > x1 or y0 > y1
  bool live;       // not dropped and area2 != 0
  bool dropped;
  bool swapped;
};

__device__ __forceinline__ float rs_row(const float* m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

__device__ __forceinline__ int rs_snap(float f, float a, float z, float c) {
  float u = (f * (a / z) + c) * 256.0f;
  u = u >= -RS_SNAP_LIMIT ? u : -RS_SNAP_LIMIT;
  u = u <= RS_SNAP_LIMIT ? u : RS_SNAP_LIMIT;
  return (int)floorf(u + 0.5f);
}

__device__ __forceinline__ int rs_owner(int ax, int ay, int bx, int by) { return (by < ay || (by == ay && bx > ax)) ? 0 : -1; }

__device__ __forceinline__ void rs_setup(RsFace& f, const float* __restrict__ vert, int V, const int* __restrict__ faces, int face,
                                         const float* __restrict__ M, const RsCam& cam) {
  f.live = false;
  f.dropped = false;
  f.swapped = false;
  f.x0 = f.y0 = 0;
  f.x1 = f.y1 = -1;
  int id[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = faces[(size_t)face * 3 + k];
    ok = ok && (unsigned)id[k] < (unsigned)V;
  }
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = vert[(size_t)id[k] * 3], y = vert[(size_t)id[k] * 3 + 1], z = vert[(size_t)id[k] * 3 + 2];
      const float px = rs_row(M, x, y, z), py = rs_row(M + 4, x, y, z), pz = rs_row(M + 8, x, y, z);
      ok = ok && (pz >= cam.near);
      f.z[k] = pz;
      f.X[k] = rs_snap(cam.fx, px, pz, cam.cx);
      f.Y[k] = rs_snap(cam.fy, py, pz, cam.cy);
    }
  }
  if (!ok) {
    f.dropped = true;
    return;
  }
  long long a2 = (long long)(f.X[1] - f.X[0]) * (f.Y[2] - f.Y[0]) - (long long)(f.X[2] - f.X[0]) * (f.Y[1] - f.Y[0]);
  if (a2 == 0) return;
  if (a2 < 0) {
    int t = f.X[1]; f.X[1] = f.X[2]; f.X[2] = t;
    t = f.Y[1]; f.Y[1] = f.Y[2]; f.Y[2] = t;
    const float s = f.z[1]; f.z[1] = f.z[2]; f.z[2] = s;
    a2 = -a2;
    f.swapped = true;
  }
  f.area2 = a2;
  f.b0 = rs_owner(f.X[1], f.Y[1], f.X[2], f.Y[2]);
  f.b1 = rs_owner(f.X[2], f.Y[2], f.X[0], f.Y[0]);
  f.b2 = rs_owner(f.X[0], f.Y[0], f.X[1], f.Y[1]);
  const int xmin = min(f.X[0], min(f.X[1], f.X[2])), xmax = max(f.X[0], max(f.X[1], f.X[2]));
  const int ymin = min(f.Y[0], min(f.Y[1], f.Y[2])), ymax = max(f.Y[0], max(f.Y[1], f.Y[2]));
  // the pixels whose centre 256 j + 128 lies in [min, max], clamped to the image before anything is addressed
  f.x0 = max((xmin + 127) >> 8, 0);
  f.x1 = min((xmax - 128) >> 8, cam.W - 1);
  f.y0 = max((ymin + 127) >> 8, 0);
  f.y1 = min((ymax - 128) >> 8, cam.H - 1);
  f.live = true;
}

__device__ __forceinline__ long long rs_edge(int ax, int ay, int bx, int by, int px, int py) {
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// the edge values of pixel (x, y); true when the centre is covered
__device__ __forceinline__ bool rs_cover(const RsFace& f, int x, int y, long long& w0, long long& w1, long long& w2) {
  const int px = 256 * x + 128, py = 256 * y + 128;
  w0 = rs_edge(f.X[1], f.Y[1], f.X[2], f.Y[2], px, py);
  w1 = rs_edge(f.X[2], f.Y[2], f.X[0], f.Y[0], px, py);
  w2 = rs_edge(f.X[0], f.Y[0], f.X[1], f.Y[1], px, py);
  return (w0 + f.b0 >= 0) && (w1 + f.b1 >= 0) && (w2 + f.b2 >= 0);
}

// perspective-correct weights l and the depth from the edge values
__device__ __forceinline__ float rs_weights(const RsFace& f, long long w0, long long w1, long long w2, float& l0, float& l1, float& l2) {
  const float q0 = (float)w0 / f.z[0], q1 = (float)w1 / f.z[1], q2 = (float)w2 / f.z[2];
  const float qs = (q0 + q1) + q2;
  l0 = q0 / qs;
  l1 = q1 / qs;
  l2 = q2 / qs;
  return (float)f.area2 / qs;
}

__device__ __forceinline__ float rs_mix(float l0, float l1, float l2, float a0, float a1, float a2) { return (l0 * a0 + l1 * a1) + l2 * a2; }

// The refusals every entry shares (defined in raster.hip), by name and before a launch or a write: the limits above, near, wave_area,
// `pointers` (the entry's own non-null test) and the workspace's size and alignment.  -> 0 or SAM6D_EINVAL with the error text set.
int rs_check(const char* who, int V, int F, int T, int H, int W, float near, int wave_area, bool pointers, const void* workspace,
             size_t workspace_bytes);

// Host side of the visibility pass, one copy for every entry (defined in raster.hip): fills the z-buffer with ~0 and n_dropped with
// 0 in stream order, then launches raster_faces_kernel.  zbuf: T*H*W 64-bit words.  `who` names the entry in an error text.
// -> 0, or the hipError_t with sam6d_set_error() called.
int rs_visibility(const char* who, const float* vertices, int V, const int* faces, int F, const float* view, int T, const RsCam& cam,
                  int wave_area, unsigned long long* zbuf, int* n_dropped, hipStream_t s);
