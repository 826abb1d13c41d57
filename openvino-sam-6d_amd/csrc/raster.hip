// Template rendering (Render/render_custom_templates.py:55-106: BlenderProc's render() and render_nocs() of one CAD model from the
// predefined camera poses) as a deterministic triangle rasteriser: T views of one mesh -> mask, visible face, depth, object-space xyz
// and a shaded rgb.  The geometry (mask, face, depth, xyz) is defined by the recipe below and restated in numpy, float32 operation by
// operation, in tests/raster_ref.py; the shading is the package's own (parity unpinned against Cycles, equal in kind only).
//
// RECIPE.  All float arithmetic is IEEE fp32 in the order written (the library is built with -ffp-contract=off and this file has no
// fused multiply-add); only + - * /, sqrt, floor and comparisons run on the device.
//   camera   per view a row-major 3x4 matrix M (object -> camera; x right, y down, z forward) and a light position in that frame.
//            P = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3] for r = 0, 1, 2.
//   near     a face with an index outside [0, V) or with a vertex whose P.z >= near is false (nearer, or NaN) is dropped whole and
//            counted in n_dropped[view]; there is no clipper.
//   snap     s = f * (P.x / P.z) + c;  u = s * 256;  u = u >= -2^24 ? u : -2^24;  u = u <= 2^24 ? u : 2^24;  X = (int)floor(u + 0.5):
//            screen coordinates in 1/256 pixel, pixel (i, j) has its centre at (256 j + 128, 256 i + 128).
//   cover    area2 = (X1-X0)*(Y2-Y0) - (X2-X0)*(Y1-Y0) in int64.  area2 == 0 covers nothing; area2 < 0 swaps vertices 1 and 2 (both
//            windings are drawn).  Edge a->b at the centre p: E = (bx-ax)*(py-ay) - (by-ay)*(px-ax); w0 = E_12, w1 = E_20, w2 = E_01,
//            so w0 + w1 + w2 = area2.  p is covered when every w_i > 0, or w_i == 0 on an edge with by < ay or (by == ay and bx > ax):
//            the top-left rule (y points down), which gives a centre on a shared edge to exactly one of the two faces.
//   depth    q_i = (float)w_i / z_i;  qs = (q0 + q1) + q2;  depth = (float)area2 / qs;  l_i = q_i / qs (perspective-correct weights);
//            an attribute is (l0*a0 + l1*a1) + l2*a2 with the l_i back in the face's stored vertex order.
//   visible  per pixel the minimum over the covering faces of (bits(depth) << 32) | face id: depth is positive, so its bit pattern
//            orders as the value does, and on a depth tie the lower face id wins.
//   xyz      the attribute of the object-space vertices (CAD units); background 0.
//   shading  n = the attribute of the vertex normals taken through M's 3x3 part, or without normals the face normal
//            (P1-P0) x (P2-P0); Pc = the attribute of the camera-space vertices; n is negated when n . Pc > 0 (towards the camera);
//            L = light - Pc, d2 = |L|^2, c = (n . L) / (sqrt(|n|^2) * sqrt(d2)), c = c > 0 ? c : 0 (a NaN gives 0);
//            v = GAIN * c / d2; per channel lin = albedo * v clamped to [0, 1] by comparisons, rgb = lut[(int)(lin * 4095 + 0.5)],
//            lut = the 4096-entry sRGB transfer table the host builds in float64.  albedo = the attribute of the vertex colours / 255,
//            or base_color when colorize is set or the mesh has none.  GAIN = 1000 / (4 pi^2) = 25.330296: the script's 1000 W point
//            light (:78) as Blender turns watts into the radiance of a diffuse surface, W / (4 pi^2 r^2).
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  The z-buffer (workspace, T*H*W 64-bit words) is filled with ~0 by a memset that
// precedes the raster kernel in stream order.  The raster kernel touches it with one operation only: a 64-bit vector atomic min at
// agent scope (every workgroup on every XCD meets at the same L2 line).  The set of (key, pixel) pairs offered is decided by the
// recipe -- each covered (face, pixel) pair offers its key exactly once, from whichever path owns the face -- and min is commutative,
// associative and idempotent, so the word a pixel ends with is the minimum of its set in whatever order the atomics land.  Nothing
// reads the buffer inside that launch.  The resolve kernel runs after the kernel boundary, reads the winner's face id, recomputes the
// same setup and the same weights at the pixel with the same device functions, and is the only writer of every output element.
// n_dropped is an integer atomicAdd of ones: order-free as well.
//
// WORK.  One launch, one wave per 64 faces of a view.  Every lane sets up its own face; a face whose clamped bounding box has fewer
// than wave_area pixels is walked by its lane (the thread path: a dense scan is mostly triangles of a few pixels); the rest are
// taken one after the other by the whole wave, 64 pixels of the box at a time (the wave path: a low-poly mesh is a few triangles of
// tens of thousands of pixels).  Both paths call rs_offer() on a face set up by rs_setup(): the arithmetic is one piece of code.
//
// FILES.  Every step of the RECIPE is a device function in raster.h: setup, coverage and weights; the pass of the WORK paragraph
// (rs_faces_pass, which verify_raster.h runs into a pose's window as well); the resolve of a pixel up to the lighting term and the tone
// step (rs_resolve_pixel, rs_tone), shared with texture.hip, whose resolve kernel takes the albedo from a texture image instead.  This
// file keeps the image sink, the two kernels' own lines (the drop count; the vertex-colour / grey albedo) and the host side:
// rs_limits, rs_check and visibility (rs_visibility) for both render entries.
#include "raster.h"
#include "../../include/sam6d_hip.h"

// the z-buffer of one view: word y * W + x, every pixel of the face's box (rs_setup clamped it to the image)
struct RsImageSink {
  unsigned long long* z;
  int W;
  __device__ __forceinline__ void clamp(RsFace&) const {}
  __device__ __forceinline__ void put(int x, int y, unsigned long long key) const {
    __hip_atomic_fetch_min(z + (size_t)y * W + x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// grid (ceil(F / 64), T), one wave each
__global__ __launch_bounds__(64) void raster_faces_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int F,
                                                          const float* __restrict__ view, RsCam cam, int wave_area,
                                                          unsigned long long* __restrict__ zbuf, int* __restrict__ n_dropped) {
  const int t = blockIdx.y, lane = threadIdx.x;
  const int face = blockIdx.x * 64 + lane;
  const float* M = view + (size_t)t * 12;
  RsFace f;
  f.live = false;
  f.dropped = false;
  f.x0 = f.y0 = 0;
  f.x1 = f.y1 = -1;
  if (face < F) rs_setup(f, vert, V, faces, face, M, cam);
  if (f.dropped) atomicAdd(n_dropped + t, 1);
  rs_faces_pass(f, face, vert, V, faces, M, cam, wave_area, RsImageSink{zbuf + (size_t)t * cam.H * cam.W, cam.W});
}

struct RsShade {
  const float* normals;
  const unsigned char* colors;
  const float* light;
  const unsigned char* lut;
  float base_color;
  int colorize;
};

// one thread per pixel of every view: the only writer of the outputs
__global__ __launch_bounds__(256) void raster_resolve_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                                             const float* __restrict__ view, RsCam cam, RsShade sh, int T,
                                                             const unsigned long long* __restrict__ zbuf, unsigned char* __restrict__ mask,
                                                             int* __restrict__ face_out, float* __restrict__ depth, float* __restrict__ xyz,
                                                             unsigned char* __restrict__ rgb) {
  const size_t hw = (size_t)cam.H * cam.W, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw * (size_t)T) return;
  RsHit h;
  if (!rs_resolve_pixel(i, vert, V, faces, view, cam, sh.normals, sh.light, zbuf, RsOut{mask, face_out, depth, xyz, rgb}, h)) return;
  const int* fv = faces + (size_t)h.face * 3;
  const bool grey = sh.colorize || !sh.colors;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float alb = sh.base_color;
    if (!grey)
      alb = rs_mix(h.l0, h.m1, h.m2, (float)sh.colors[(size_t)fv[0] * 3 + k] / 255.0f, (float)sh.colors[(size_t)fv[1] * 3 + k] / 255.0f,
                   (float)sh.colors[(size_t)fv[2] * 3 + k] / 255.0f);
    rgb[i * 3 + k] = rs_tone(alb * h.v, sh.lut);
  }
}

extern "C" size_t sam6d_render_views_workspace_bytes(int T, int H, int W) {
  if (T < 1 || T > RS_MAX_T || H < 1 || H > RS_MAX_HW || W < 1 || W > RS_MAX_HW) return 0;
  return (size_t)T * H * W * sizeof(unsigned long long);
}

int rs_limits(const char* who, int V, int F, const char* count_name, int count, int count_max, int H, int W, float near) {
  SAM6D_REQUIRE(H >= 1 && H <= RS_MAX_HW && W >= 1 && W <= RS_MAX_HW, "%s: H x W = %d x %d is not in 1 .. %d", who, H, W, RS_MAX_HW);
  SAM6D_REQUIRE(count >= 1 && count <= count_max, "%s: %s = %d is not in 1 .. %d", who, count_name, count, count_max);
  SAM6D_REQUIRE(F >= 1 && F <= RS_MAX_F, "%s: F = %d is not in 1 .. %d", who, F, RS_MAX_F);
  SAM6D_REQUIRE(V >= 1, "%s: V = %d is not positive", who, V);
  SAM6D_REQUIRE(near > 0.f, "%s: near = %g is not positive", who, (double)near);
  return 0;
}

int rs_check(const char* who, int V, int F, int T, int H, int W, float near, int wave_area, bool pointers, const void* workspace,
             size_t workspace_bytes) {
  const int bad = rs_limits(who, V, F, "T", T, RS_MAX_T, H, W, near);
  if (bad) return bad;
  SAM6D_REQUIRE(wave_area >= 0, "%s: wave_area = %d is negative", who, wave_area);
  SAM6D_REQUIRE(pointers && workspace, "%s: null pointer", who);
  const size_t need = sam6d_render_views_workspace_bytes(T, H, W);
  SAM6D_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes is below sam6d_render_views_workspace_bytes = %zu", who, workspace_bytes,
                need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  return 0;
}

int rs_visibility(const char* who, const float* vertices, int V, const int* faces, int F, const float* view, int T, const RsCam& cam,
                  int wave_area, unsigned long long* zbuf, int* n_dropped, hipStream_t s) {
  hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)T * cam.H * cam.W * sizeof(unsigned long long), s);
  if (e == hipSuccess) e = hipMemsetAsync(n_dropped, 0, (size_t)T * sizeof(int), s);
  if (e != hipSuccess) {
    sam6d_set_error("%s: memset failed: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(raster_faces_kernel, dim3((F + 63) / 64, T), dim3(64), 0, s, vertices, V, faces, F, view, cam,
                     wave_area ? wave_area : RS_WAVE_AREA, zbuf, n_dropped);
  e = hipGetLastError();
  if (e != hipSuccess) sam6d_set_error("%s (faces): launch failed: %s", who, hipGetErrorString(e));
  return (int)e;
}

extern "C" int sam6d_render_views(const float* vertices, int V, const int* faces, int F, const float* normals, const unsigned char* colors,
                                  const float* view, const float* light, int T, float fx, float fy, float cx, float cy, int H, int W,
                                  float near, float base_color, int colorize, const unsigned char* srgb_lut, int wave_area,
                                  unsigned char* mask, int* face, float* depth, float* xyz, unsigned char* rgb, int* n_dropped,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  const int bad = rs_check("render_views", V, F, T, H, W, near, wave_area,
                           vertices && faces && view && light && srgb_lut && mask && face && depth && xyz && rgb && n_dropped, workspace,
                           workspace_bytes);
  if (bad) return bad;
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  const RsShade sh = {normals, colors, light, srgb_lut, base_color, colorize};
  unsigned long long* zbuf = (unsigned long long*)workspace;
  const int err = rs_visibility("render_views", vertices, V, faces, F, view, T, cam, wave_area, zbuf, n_dropped, s);
  if (err) return err;
  const size_t px = (size_t)T * H * W;  // at most 2^32: 2^24 blocks
  hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, vertices, V, faces, view, cam, sh, T, zbuf,
                     mask, face, depth, xyz, rgb);
  SAM6D_LAUNCH_CHECK("render_views (resolve)");
}
