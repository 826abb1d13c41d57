// What the translation units that stand on the triangle rasteriser share (raster.hip: visibility and the vertex-colour / grey resolve;
// texture.hip: the textured resolve; verify.hip and refine.hip through verify_raster.h: poses rendered into windows), one copy of each
// step of raster.hip's RECIPE as device functions:
//   rs_setup, rs_cover, rs_weights   the face setup, coverage and weights;
//   rs_offer, rs_faces_pass          the visibility pass of one wave over 64 faces -- thread path and wave path -- writing through a Sink
//                                    (the image's z-buffer in raster.hip, a pose's window in verify_raster.h);
//   rs_to_camera, rs_face_normal     a vertex in camera space and the face normal (P1-P0) x (P2-P0) (the resolve core, refine.hip's pairs);
//   rs_resolve_pixel, rs_tone        the resolve of one pixel up to the lighting term v, and the tone step, for both resolve kernels.
// So every user recomputes a winner's weights with the very code the visibility pass ran.  The host side: the refusals every entry
// shares (rs_limits, rs_check) and the visibility pass (rs_visibility), defined in raster.hip.
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

// ---- the visibility pass.  A Sink says where a key goes: clamp(f) narrows a set-up face's pixel box to what the sink holds,
// put(x, y, key) offers the key to the word of pixel (x, y) with a 64-bit atomic min at agent scope.
template <class Sink>
__device__ __forceinline__ void rs_offer(const RsFace& f, int face, int x, int y, const Sink& sink) {
  long long w0, w1, w2;
  if (!rs_cover(f, x, y, w0, w1, w2)) return;
  float l0, l1, l2;
  const float d = rs_weights(f, w0, w1, w2, l0, l1, l2);
  sink.put(x, y, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)face);
}

// One wave (a workgroup of 64, grid.x over the faces) and the face each lane set up, `face` = blockIdx.x * 64 + lane: a face whose
// clamped box has fewer than wave_area pixels is walked by its lane (the thread path); the rest are taken one after the other by
// the whole wave, 64 pixels of the box at a time (the wave path).  Both paths call rs_offer() on a face set up by rs_setup().
template <class Sink>
__device__ __forceinline__ void rs_faces_pass(RsFace& f, int face, const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                              const float* __restrict__ M, const RsCam& cam, int wave_area, const Sink& sink) {
  const int lane = threadIdx.x;
  sink.clamp(f);
  const bool boxed = f.live && f.x0 <= f.x1 && f.y0 <= f.y1;
  const int bw = f.x1 - f.x0 + 1, bh = f.y1 - f.y0 + 1;  // at most 2048 each: the product fits an int
  const bool big = boxed && bw * bh >= wave_area;
  if (boxed && !big)
    for (int y = f.y0; y <= f.y1; ++y)
      for (int x = f.x0; x <= f.x1; ++x) rs_offer(f, face, x, y, sink);
  unsigned long long todo = __ballot(big);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int gface = blockIdx.x * 64 + src;
    RsFace g;
    rs_setup(g, vert, V, faces, gface, M, cam);  // the same code on the same inputs as the owner lane ran: the same face
    sink.clamp(g);
    const int gw = g.x1 - g.x0 + 1, n = gw * (g.y1 - g.y0 + 1);
    for (int i = lane; i < n; i += 64) rs_offer(g, gface, g.x0 + i % gw, g.y0 + i / gw, sink);
  }
}

// ---- the resolve
// RECIPE camera: an object-space vertex through the view matrix M
__device__ __forceinline__ void rs_to_camera(const float* __restrict__ M, const float* __restrict__ v, float (&P)[3]) {
  P[0] = rs_row(M, v[0], v[1], v[2]);
  P[1] = rs_row(M + 4, v[0], v[1], v[2]);
  P[2] = rs_row(M + 8, v[0], v[1], v[2]);
}

// RECIPE shading: the face normal (P1-P0) x (P2-P0) of camera-space vertices in stored order, not normalised
__device__ __forceinline__ void rs_face_normal(const float (&P)[3][3], float (&n)[3]) {
  const float e1x = P[1][0] - P[0][0], e1y = P[1][1] - P[0][1], e1z = P[1][2] - P[0][2];
  const float e2x = P[2][0] - P[0][0], e2y = P[2][1] - P[0][1], e2z = P[2][2] - P[0][2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

struct RsOut {
  unsigned char* mask;
  int* face;
  float* depth;
  float* xyz;
  unsigned char* rgb;
};

struct RsHit {
  int face;
  float l0, m1, m2;  // the weights in the face's stored vertex order
  float v;           // the lighting term
};

// Pixel i of the T views, the part both resolve kernels share.  A background pixel: writes all five outputs -> false.  Else recomputes
// the winner's setup and weights, writes mask, face, depth and xyz, computes the lighting term of RECIPE shading -> true with `h` set;
// rgb is the caller's (its albedo, then rs_tone).
__device__ __forceinline__ bool rs_resolve_pixel(size_t i, const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                                 const float* __restrict__ view, const RsCam& cam, const float* normals,
                                                 const float* __restrict__ light, const unsigned long long* __restrict__ zbuf,
                                                 const RsOut& out, RsHit& h) {
  const size_t hw = (size_t)cam.H * cam.W;
  const int t = (int)(i / hw), p = (int)(i % hw), y = p / cam.W, x = p % cam.W;
  const unsigned long long key = zbuf[i];
  if (key == ~0ull) {
    out.mask[i] = 0;
    out.face[i] = -1;
    out.depth[i] = 0.f;
    out.xyz[i * 3] = out.xyz[i * 3 + 1] = out.xyz[i * 3 + 2] = 0.f;
    out.rgb[i * 3] = out.rgb[i * 3 + 1] = out.rgb[i * 3 + 2] = 0;
    return false;
  }
  const int face = (int)(unsigned)(key & 0xffffffffull);
  const float* M = view + (size_t)t * 12;
  RsFace f;
  rs_setup(f, vert, V, faces, face, M, cam);
  long long w0, w1, w2;
  rs_cover(f, x, y, w0, w1, w2);
  float l0, l1, l2;
  const float d = rs_weights(f, w0, w1, w2, l0, l1, l2);
  // the weights in the face's stored order (a winding swap exchanged vertices 1 and 2): every attribute is mixed in that order
  const float m1 = f.swapped ? l2 : l1, m2 = f.swapped ? l1 : l2;
  const int* fv = faces + (size_t)face * 3;
  const float* a = vert + (size_t)fv[0] * 3;
  const float* b = vert + (size_t)fv[1] * 3;
  const float* c = vert + (size_t)fv[2] * 3;
  out.mask[i] = 255;
  out.face[i] = face;
  out.depth[i] = d;
#pragma unroll
  for (int k = 0; k < 3; ++k) out.xyz[i * 3 + k] = rs_mix(l0, m1, m2, a[k], b[k], c[k]);
  // ---- shading (the package's own)
  float P[3][3];  // camera-space vertices, stored order
#pragma unroll
  for (int k = 0; k < 3; ++k) rs_to_camera(M, vert + (size_t)fv[k] * 3, P[k]);
  float Pc[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Pc[k] = rs_mix(l0, m1, m2, P[0][k], P[1][k], P[2][k]);
  if (normals) {
    float no[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) no[k] = rs_mix(l0, m1, m2, normals[(size_t)fv[0] * 3 + k], normals[(size_t)fv[1] * 3 + k], normals[(size_t)fv[2] * 3 + k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (M[4 * k] * no[0] + M[4 * k + 1] * no[1]) + M[4 * k + 2] * no[2];
  } else {
    rs_face_normal(P, n);
  }
  const float facing = (n[0] * Pc[0] + n[1] * Pc[1]) + n[2] * Pc[2];
  if (facing > 0.f) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
  const float* lp = light + (size_t)t * 3;
  const float Lx = lp[0] - Pc[0], Ly = lp[1] - Pc[1], Lz = lp[2] - Pc[2];
  const float d2 = (Lx * Lx + Ly * Ly) + Lz * Lz;
  const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  const float ndl = (n[0] * Lx + n[1] * Ly) + n[2] * Lz;
  float cs = ndl / (sqrtf(nn) * sqrtf(d2));
  cs = cs > 0.f ? cs : 0.f;
  h.face = face;
  h.l0 = l0;
  h.m1 = m1;
  h.m2 = m2;
  h.v = RS_GAIN * cs / d2;
  return true;
}

// RECIPE shading, the last step: a linear value clamped to [0, 1] by comparisons, through the 4096-entry sRGB table
__device__ __forceinline__ unsigned char rs_tone(float lin, const unsigned char* __restrict__ lut) {
  lin = lin > 0.f ? lin : 0.f;
  lin = lin < 1.f ? lin : 1.f;
  return lut[(int)(lin * 4095.0f + 0.5f)];
}

// The limits every entry of the family shares (defined in raster.hip), by name and before a launch or a write: H, W, the number of
// views or poses (`count`, named `count_name` in the text, at most `count_max`), F, V and near.  -> 0 or SAM6D_EINVAL, error text set.
int rs_limits(const char* who, int V, int F, const char* count_name, int count, int count_max, int H, int W, float near);

// The refusals the two render entries share (defined in raster.hip): rs_limits, wave_area, `pointers` (the entry's own non-null test)
// and the workspace's size and alignment.  -> 0 or SAM6D_EINVAL with the error text set.
int rs_check(const char* who, int V, int F, int T, int H, int W, float near, int wave_area, bool pointers, const void* workspace,
             size_t workspace_bytes);

// Host side of the visibility pass, one copy for every entry (defined in raster.hip): fills the z-buffer with ~0 and n_dropped with
// 0 in stream order, then launches raster_faces_kernel.  zbuf: T*H*W 64-bit words.  `who` names the entry in an error text.
// -> 0, or the hipError_t with sam6d_set_error() called.
int rs_visibility(const char* who, const float* vertices, int V, const int* faces, int F, const float* view, int T, const RsCam& cam,
                  int wave_area, unsigned long long* zbuf, int* n_dropped, hipStream_t s);
