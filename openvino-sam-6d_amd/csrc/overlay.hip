// The two result pictures of the reference's inference scripts, built on the device: vis_ism.png (ISM/run_inference_custom.py:48-84,
// `visualize`: the best detection's mask blended over the grey image, its edge in white) and vis_pem.png
// (PEM/run_inference_custom.py:110-134 over PEM/utils/draw_utils.py:5-97, `draw_detections`: the projected box and 512 model points of
// every pose), each pasted to the right of the input image (ISM :79-84, PEM :128-133) without the PNG round trip.  Both are defined by
// the integer recipes below and restated in numpy in tests/overlay_ref.py; every comparison is bit for bit.
//
// WHAT IS THE REFERENCE'S AND WHAT IS THE PACKAGE'S OWN.  The reference's: the grey conversion, the blend expression and its
// truncation, "later paint wins", the paint order ground - pillars - top - points per instance, the shades int(0.3 c) / int(0.6 c) / c,
// the truncating int32 cast of the projection, the box corners (built on the host) and the side-by-side layout.  The package's own,
// equal in kind only: the edge of a mask (skimage's canny is not restated), the shape of a thick line (NOT cv2.line's polygon fill),
// the shape of a filled disc (NOT cv2.circle's), and the rule for a point at or behind the camera plane (the reference has none and
// divides by zero).
//
// RECIPE.  All device arithmetic is integer, or IEEE fp32 in the order written (the library is built with -ffp-contract=off and this
// file has no fused multiply-add).  canvas is (H, 2W, 3) u8: columns 0 .. W-1 are rgb unchanged, columns W .. 2W-1 the picture.
//
//  a. mask overlay (sam6d_overlay_masks), per pixel (y, x) of the right half:
//   grey     g = (4899 R + 9617 G + 1868 B + 8192) >> 14: the 8-bit RGB2GRAY fixed point OpenCV publishes (14-bit coefficients of
//            0.299, 0.587, 0.114, rounded); (255,0,0) -> 76, (0,255,0) -> 150, (0,0,255) -> 29.  A restatement: cv2 was not at hand
//            where this was built, so it is NOT pinned against cv2.
//   blend    masks (M,H,W), non-zero = inside, are drawn in the order given, later over earlier: with m the LAST mask that covers the
//            pixel, channel c = lut[m][c][g]; without one, c = g.  lut (M,3,256) u8 is built on the host with the reference's own
//            expression (ISM :70-72: alpha * col + (1 - alpha) * v in float64, truncated by the assignment into a uint8 array); the
//            kernel only looks up.
//   edge     edge0(y, x) = mask(y, x) and at least one of the four neighbours INSIDE THE IMAGE is not mask (an image border alone
//            makes no edge); edge(y, x) = OR of edge0(y + dy, x + dx), dy, dx in {0, 1}, 0 outside the image: exactly
//            scipy.ndimage.binary_dilation(edge0, np.ones((2, 2))) (ISM :63; its origin is the lower-right cell).  A pixel in the
//            edge of ANY drawn mask is 255 in all channels (ISM :73).  draw_edge = 0 leaves the edges out.
//   A pure gather: one thread per pixel is the only writer of its six canvas bytes; no atomics.
//
//  b. pose overlay (sam6d_draw_detections), instance i = 0 .. N-1 with R, t, K row-major:
//   project  P_r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r];  q_r = (K[r][0] P_0 + K[r][1] P_1) + K[r][2] P_2;  uf = q_0 / q_2,
//            vf = q_1 / q_2;  u = (int)uf, v = (int)vf: truncation toward zero, the reference's dtype=np.int32 cast (draw_utils.py:13-16).
//   skip     a point is skipped when q_2 > 0 is false (at or behind the camera plane, or NaN), or when -8192 <= uf <= 8191 or
//            -8192 <= vf <= 8191 is false (compared in fp32, before the conversion; a NaN fails).  An edge is skipped when either
//            endpoint is.  Every skipped primitive (edge or point; the eight corners are not primitives) adds one to n_skipped[i].
//   paint    stage 0: the ground edges (4,5) (5,7) (6,4) (7,6) in (c * 3) / 10; stage 1: the pillars (k, k+4) in (c * 6) / 10; stage 2:
//            the top edges (0,1) (1,3) (2,0) (3,2) in c; stage 3: the P points in c (draw_utils.py:51-97).  The integer quotients are
//            Python's int(c * 0.3) and int(c * 0.6) for every c in 0 .. 255 (tests/test_overlay_host.py checks all 256).  Later paint
//            wins: the painter's key of a primitive is 4 i + stage + 1 and a pixel shows the largest key offered to it.  All
//            primitives of one stage of one instance have one colour, so their mutual order cannot show.
//   line     pixel p is in the line A -> B of thickness T when, with d = B - A, L2 = d . d, w = p - A, s = w . d:
//              s <= 0:   4 |w|^2 <= T^2                        (the round cap at A; a zero-length edge is this disc)
//              s >= L2:  4 |p - B|^2 <= T^2                    (the round cap at B)
//              else      4 (d.x w.y - d.y w.x)^2 <= T^2 L2     (distance to the line at most T / 2)
//            an integer predicate, so how the pixels are visited cannot change the result.  With coordinates in -8192 .. 8191 and
//            pixels in 0 .. 8191 every difference is below 2^14 in magnitude, the cross product below 2^29, its square below 2^58 and
//            four times it below 2^60; T^2 L2 is below 2^37: everything is kept in int64.
//   disc     pixel p is in the point c of radius r when dx^2 + dy^2 <= r^2 (r = 1: the five-pixel plus).
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  The key buffer (workspace, H*W 32-bit words) is zeroed by a memset that precedes
// the paint kernel in stream order.  The paint kernel touches it with one operation only: a 32-bit vector atomic max at agent scope
// (every workgroup on every XCD meets at the same L2 line).  The set of (key, pixel) pairs offered is decided by the recipe -- the
// walk below visits a superset of each predicate's support and offers exactly the pixels the predicate accepts -- and max is
// commutative, associative and idempotent, so the word a pixel ends with is the maximum of its set in whatever order the atomics
// land, and however often a pair is offered.  Nothing reads the buffer inside that launch.  The resolve kernel runs after the kernel
// boundary and is the only writer of every canvas byte: key 0 gives the input pixel, another key the colour of instance (key-1) >> 2
// in the shade of stage (key-1) & 3.  n_skipped is an integer atomicAdd of ones: order-free as well.
//
// WORK.  One workgroup of four waves per instance.  The eight corners are projected once into LDS.  Lanes stride over the P points.
// Each wave takes the edges e = wave, wave + 4, wave + 8 and walks an edge's major axis (the one with the larger |d|), clipped to the
// image and extended by ceil(T / 2) + 1 beyond both endpoints, one major coordinate per lane; at each, with the coordinate clamped to
// the segment, the minor coordinate of the line is c = A.n + floor(((m - A.m) d.n) / d.m) and the candidates c - (T+1) .. c + (T+1),
// clipped to the image, are tested with the predicate.  That is a superset of the predicate's support: a pixel of the band lies
// within T / 2 of the line, so within T sqrt(2) / 2 along the minor axis (|slope| <= 1) plus the floor's 1; a pixel of a cap lies
// within T / 2 of the endpoint on both axes.  O(length) per edge, where a bounding-box scan of a screen diagonal would test every pixel
// of the image; nothing is sized by the longest edge of the batch.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define OV_MAX_HW 8192
#define OV_MAX_M 4096
#define OV_MAX_N 65535
#define OV_MAX_P 65536
#define OV_MAX_T 15
#define OV_MAX_R 15
#define OV_COORD_LO -8192.0f
#define OV_COORD_HI 8191.0f

// the left half of the canvas: the input pixel
__device__ __forceinline__ void ov_copy_left(const unsigned char* __restrict__ src, unsigned char* __restrict__ row, int x) {
  row[(size_t)x * 3] = src[0];
  row[(size_t)x * 3 + 1] = src[1];
  row[(size_t)x * 3 + 2] = src[2];
}

// ---------------------------------------------------------------------------------------------------------- a. mask overlay
// edge0 of mask m at (y, x), which is inside the image and inside the mask
__device__ __forceinline__ bool ov_edge0_inside(const unsigned char* __restrict__ m, int y, int x, int H, int W) {
  const unsigned char* p = m + (size_t)y * W + x;
  bool e = false;
  if (y > 0) e = e || p[-(ptrdiff_t)W] == 0;
  if (y + 1 < H) e = e || p[W] == 0;
  if (x > 0) e = e || p[-1] == 0;
  if (x + 1 < W) e = e || p[1] == 0;
  return e;
}

// one thread per pixel: the only writer of the pixel's six canvas bytes
__global__ __launch_bounds__(256) void overlay_masks_kernel(const unsigned char* __restrict__ rgb, long row_stride, int H, int W,
                                                            const unsigned char* __restrict__ masks, int M,
                                                            const unsigned char* __restrict__ lut, int draw_edge,
                                                            unsigned char* __restrict__ canvas) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i % W);
  const unsigned char* src = rgb + (size_t)y * row_stride + (size_t)x * 3;
  unsigned char* row = canvas + (size_t)y * 2 * W * 3;
  ov_copy_left(src, row, x);
  const int g = (4899 * (int)src[0] + 9617 * (int)src[1] + 1868 * (int)src[2] + 8192) >> 14;
  const bool y1 = y + 1 < H, x1 = x + 1 < W;
  int last = -1;
  bool edge = false;
  for (int m = M - 1; m >= 0 && !edge; --m) {
    const unsigned char* mk = masks + (size_t)m * H * W;
    const unsigned char* p = mk + (size_t)y * W + x;
    const bool c00 = p[0] != 0;
    if (c00 && last < 0) last = m;
    if (!draw_edge) {
      if (last >= 0) break;
      continue;
    }
    // the 2 x 2 block whose edge0 dilates onto this pixel: a cell outside the mask or the image has no edge0
    if (c00 && ov_edge0_inside(mk, y, x, H, W)) edge = true;
    if (!edge && x1 && p[1] != 0 && ov_edge0_inside(mk, y, x + 1, H, W)) edge = true;
    if (!edge && y1 && p[W] != 0 && ov_edge0_inside(mk, y + 1, x, H, W)) edge = true;
    if (!edge && y1 && x1 && p[(size_t)W + 1] != 0 && ov_edge0_inside(mk, y + 1, x + 1, H, W)) edge = true;
  }
  unsigned char* dst = row + (size_t)(W + x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int v = g;
    if (last >= 0) v = lut[((size_t)last * 3 + c) * 256 + g];
    if (edge) v = 255;
    dst[c] = (unsigned char)v;
  }
}

extern "C" int sam6d_overlay_masks(const unsigned char* rgb, long row_stride, int H, int W, const unsigned char* masks, int M,
                                   const unsigned char* lut, int draw_edge, unsigned char* canvas, void* stream) {
  SAM6D_REQUIRE(H >= 1 && H <= OV_MAX_HW && W >= 1 && W <= OV_MAX_HW, "overlay_masks: H x W = %d x %d is not in 1 .. %d", H, W, OV_MAX_HW);
  SAM6D_REQUIRE(M >= 0 && M <= OV_MAX_M, "overlay_masks: M = %d is not in 0 .. %d", M, OV_MAX_M);
  SAM6D_REQUIRE(row_stride >= 3L * W, "overlay_masks: row_stride = %ld is below 3 W = %ld", row_stride, 3L * W);
  SAM6D_REQUIRE(rgb && canvas && (M == 0 || (masks && lut)), "overlay_masks: null pointer");
  const size_t px = (size_t)H * W;  // at most 2^26: 2^18 blocks
  hipLaunchKernelGGL(overlay_masks_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb, row_stride, H, W,
                     masks, M, lut, draw_edge, canvas);
  SAM6D_LAUNCH_CHECK("overlay_masks");
}

// ---------------------------------------------------------------------------------------------------------- b. pose overlay
struct OvPose {
  float R[9], t[3], K[9];
};

// (u, v) of a model point; false when the point is skipped
__device__ __forceinline__ bool ov_project(const OvPose& q, const float* __restrict__ p, int& u, int& v) {
  const float x = p[0], y = p[1], z = p[2];
  const float P0 = ((q.R[0] * x + q.R[1] * y) + q.R[2] * z) + q.t[0];
  const float P1 = ((q.R[3] * x + q.R[4] * y) + q.R[5] * z) + q.t[1];
  const float P2 = ((q.R[6] * x + q.R[7] * y) + q.R[8] * z) + q.t[2];
  const float q0 = (q.K[0] * P0 + q.K[1] * P1) + q.K[2] * P2;
  const float q1 = (q.K[3] * P0 + q.K[4] * P1) + q.K[5] * P2;
  const float q2 = (q.K[6] * P0 + q.K[7] * P1) + q.K[8] * P2;
  u = v = 0;
  if (!(q2 > 0.f)) return false;
  const float uf = q0 / q2, vf = q1 / q2;
  if (!(uf >= OV_COORD_LO && uf <= OV_COORD_HI && vf >= OV_COORD_LO && vf <= OV_COORD_HI)) return false;
  u = (int)uf;
  v = (int)vf;
  return true;
}

__device__ __forceinline__ void ov_offer(unsigned* __restrict__ keys, int W, int x, int y, unsigned key) {
  __hip_atomic_fetch_max(keys + (size_t)y * W + x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the thick-line predicate of the recipe at pixel (px, py)
__device__ __forceinline__ bool ov_in_line(int ax, int ay, int bx, int by, int px, int py, long long T2) {
  const long long dx = bx - ax, dy = by - ay, wx = px - ax, wy = py - ay;
  const long long L2 = dx * dx + dy * dy, s = wx * dx + wy * dy;
  if (s <= 0) return 4 * (wx * wx + wy * wy) <= T2;
  if (s >= L2) {
    const long long ex = px - bx, ey = py - by;
    return 4 * (ex * ex + ey * ey) <= T2;
  }
  const long long cr = dx * wy - dy * wx;
  return 4 * (cr * cr) <= T2 * L2;
}

__device__ __forceinline__ long long ov_floor_div(long long a, long long b) {  // b != 0
  long long q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}

// one wave walks the edge A -> B along its major axis
__device__ __forceinline__ void ov_walk_edge(int ax, int ay, int bx, int by, int T, int H, int W, unsigned key, int lane,
                                             unsigned* __restrict__ keys) {
  const int adx = abs(bx - ax), ady = abs(by - ay);
  const bool xmajor = adx >= ady;
  // (m, n) = (major, minor) coordinates
  const int am = xmajor ? ax : ay, an = xmajor ? ay : ax, bm = xmajor ? bx : by, bn = xmajor ? by : bx;
  const int size_m = xmajor ? W : H, size_n = xmajor ? H : W;
  const int ext = (T + 1) / 2 + 1, reach = T + 1;
  const int seg_lo = min(am, bm), seg_hi = max(am, bm);
  const int lo = max(seg_lo - ext, 0), hi = min(seg_hi + ext, size_m - 1);
  const long long dm = bm - am, dn = bn - an, T2 = (long long)T * T;
  for (int m = lo + lane; m <= hi; m += 64) {
    const int mc = min(max(m, seg_lo), seg_hi);
    const int c = dm == 0 ? an : an + (int)ov_floor_div((long long)(mc - am) * dn, dm);
    const int n0 = max(c - reach, 0), n1 = min(c + reach, size_n - 1);
    for (int n = n0; n <= n1; ++n) {
      const int px = xmajor ? m : n, py = xmajor ? n : m;
      if (ov_in_line(ax, ay, bx, by, px, py, T2)) ov_offer(keys, W, px, py, key);
    }
  }
}

// grid (N), four waves: instance blockIdx.x
__global__ __launch_bounds__(256) void draw_paint_kernel(const float* __restrict__ R, const float* __restrict__ t, const float* __restrict__ K,
                                                         const float* __restrict__ box, const float* __restrict__ pts, int P, int T,
                                                         int radius, int H, int W, unsigned* __restrict__ keys,
                                                         int* __restrict__ n_skipped) {
  __shared__ int cu[8], cv[8], cok[8];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  OvPose q;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    q.R[k] = R[(size_t)i * 9 + k];
    q.K[k] = K[(size_t)i * 9 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) q.t[k] = t[(size_t)i * 3 + k];
  if (tid < 8) {
    int u, v;
    cok[tid] = ov_project(q, box + tid * 3, u, v) ? 1 : 0;
    cu[tid] = u;
    cv[tid] = v;
  }
  __syncthreads();
  const unsigned base = 4u * (unsigned)i + 1u;
  // ---- stages 0 .. 2: the twelve edges, three per wave
  for (int e = wave; e < 12; e += 4) {
    const int stage = e >> 2, k = e & 3;
    const int nxt = (0x2031 >> (4 * k)) & 15;  // {1, 3, 0, 2}[k]
    const int a = stage == 0 ? 4 + k : k;
    const int b = stage == 0 ? 4 + nxt : (stage == 1 ? k + 4 : nxt);
    if (!(cok[a] && cok[b])) {
      if (lane == 0) atomicAdd(n_skipped + i, 1);
      continue;
    }
    ov_walk_edge(cu[a], cv[a], cu[b], cv[b], T, H, W, base + (unsigned)stage, lane, keys);
  }
  // ---- stage 3: the points
  const int r2 = radius * radius;
  for (int j = tid; j < P; j += 256) {
    int u, v;
    if (!ov_project(q, pts + (size_t)j * 3, u, v)) {
      atomicAdd(n_skipped + i, 1);
      continue;
    }
    const int y0 = max(v - radius, 0), y1 = min(v + radius, H - 1), x0 = max(u - radius, 0), x1 = min(u + radius, W - 1);
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x)
        if ((x - u) * (x - u) + (y - v) * (y - v) <= r2) ov_offer(keys, W, x, y, base + 3u);
  }
}

// one thread per pixel: the only writer of the pixel's six canvas bytes
__global__ __launch_bounds__(256) void draw_resolve_kernel(const unsigned char* __restrict__ rgb, long row_stride, int H, int W,
                                                           const unsigned* __restrict__ keys, const unsigned char* __restrict__ colors,
                                                           unsigned char* __restrict__ canvas) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i % W);
  const unsigned char* src = rgb + (size_t)y * row_stride + (size_t)x * 3;
  unsigned char* row = canvas + (size_t)y * 2 * W * 3;
  ov_copy_left(src, row, x);
  unsigned char* dst = row + (size_t)(W + x) * 3;
  const unsigned key = keys[i];
  if (key == 0) {
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    return;
  }
  const unsigned inst = (key - 1) >> 2, stage = (key - 1) & 3;
  const int num = stage == 0 ? 3 : (stage == 1 ? 6 : 10);
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = (unsigned char)(((int)colors[(size_t)inst * 3 + c] * num) / 10);
}

extern "C" size_t sam6d_draw_detections_workspace_bytes(int H, int W) {
  if (H < 1 || H > OV_MAX_HW || W < 1 || W > OV_MAX_HW) return 0;
  return (size_t)H * W * sizeof(unsigned);
}

extern "C" int sam6d_draw_detections(const unsigned char* rgb, long row_stride, int H, int W, const float* R, const float* t, const float* K,
                                     int N, const float* box, const float* pts, int P, const unsigned char* colors, int thickness,
                                     int radius, unsigned char* canvas, int* n_skipped, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  SAM6D_REQUIRE(H >= 1 && H <= OV_MAX_HW && W >= 1 && W <= OV_MAX_HW, "draw_detections: H x W = %d x %d is not in 1 .. %d", H, W, OV_MAX_HW);
  SAM6D_REQUIRE(N >= 0 && N <= OV_MAX_N, "draw_detections: N = %d is not in 0 .. %d", N, OV_MAX_N);
  SAM6D_REQUIRE(P >= 0 && P <= OV_MAX_P, "draw_detections: P = %d is not in 0 .. %d", P, OV_MAX_P);
  SAM6D_REQUIRE(thickness >= 1 && thickness <= OV_MAX_T, "draw_detections: thickness = %d is not in 1 .. %d", thickness, OV_MAX_T);
  SAM6D_REQUIRE(radius >= 0 && radius <= OV_MAX_R, "draw_detections: radius = %d is not in 0 .. %d", radius, OV_MAX_R);
  SAM6D_REQUIRE(row_stride >= 3L * W, "draw_detections: row_stride = %ld is below 3 W = %ld", row_stride, 3L * W);
  SAM6D_REQUIRE(rgb && canvas && workspace, "draw_detections: null pointer");
  SAM6D_REQUIRE(N == 0 || (R && t && K && box && colors && n_skipped && (P == 0 || pts)), "draw_detections: null pointer");
  const size_t need = sam6d_draw_detections_workspace_bytes(H, W);
  SAM6D_REQUIRE(workspace_bytes >= need, "draw_detections: workspace of %zu bytes is below sam6d_draw_detections_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 3) == 0, "draw_detections: workspace is not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0, need, s);
  if (e == hipSuccess && N > 0) e = hipMemsetAsync(n_skipped, 0, (size_t)N * sizeof(int), s);
  if (e != hipSuccess) {
    sam6d_set_error("draw_detections: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  unsigned* keys = (unsigned*)workspace;
  if (N > 0) {
    hipLaunchKernelGGL(draw_paint_kernel, dim3(N), dim3(256), 0, s, R, t, K, box, pts, P, thickness, radius, H, W, keys, n_skipped);
    SAM6D_LAUNCH_CHECK_CONT("draw_detections (paint)");
  }
  const size_t px = (size_t)H * W;  // at most 2^26: 2^18 blocks
  hipLaunchKernelGGL(draw_resolve_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, rgb, row_stride, H, W, keys, colors, canvas);
  SAM6D_LAUNCH_CHECK("draw_detections (resolve)");
}
