// Checking poses against the depth image the scene was measured with: the CAD model is rendered at each of N poses into a window of
// its own, each window is compared with the observed depth pixel by pixel, all poses are composited into one instance map, and a
// picture is painted from that map.  The reference has no such check: it multiplies the detection score by the PEM score
// (PEM/run_inference_custom_pytorch.py:460-471) and draws the top pose as a box and 512 points (:480-482 over
// PEM/utils/draw_utils.py:75-97).  The check, its classes and its threshold are the package's own.  The geometry is the template
// renderer's (Render/render_custom_templates.py:55-106 as csrc/raster.hip restates it): the raster pass is raster.h's rs_faces_pass,
// the one sam6d_render_views runs, writing into a window instead of an image, so a pixel's coverage and depth are that entry's for
// the same view, bit for bit.  Restated in numpy in tests/verify_ref.py; every comparison is bit for bit.
//
// RECIPE.  All float arithmetic is IEEE fp32 in the order written (the library is built with -ffp-contract=off and this file has no
// fused multiply-add), everything else is integer.  Camera, near plane, snap, coverage and depth are raster.hip's RECIPE.
//
//  a. windows (sam6d_pose_windows), per pose n with its view matrix view[n]:
//   box      over the faces that are live (not dropped, area2 != 0) and whose pixel box clamped to the image is not empty: the minimum
//            x0, y0 and the maximum x1, y1 of those boxes, inclusive; [0, 0, -1, -1] when there is no such face.
//   dropped  n_dropped[n] = the faces dropped whole (a vertex with P.z >= near false, or an index outside [0, V)), as in raster.hip.
//
//  b. verify (sam6d_pose_verify).  The window of pose n is box[n] clamped to the image, bw x bh pixels (0 x 0 when empty); its words
//     are offset[n] .. offset[n] + bw * bh - 1 of the z-buffer, word offset[n] + (y - y0) * bw + (x - x0) for pixel (y, x).
//   raster   every face's pixel box is clamped to the window; each covered pixel offers (bits(depth) << 32) | face to its word; the
//            minimum wins (raster.hip's `visible`).
//   classify per window word that is not empty: r = the float whose bits are the key's upper half (nothing is recomputed),
//            o = depth_obs[y][x].  unknown when o > 0 is false (zero, negative, NaN).  Else e = o - r: behind when e > tau (the
//            camera sees through where the model should be), occluded when e < -tau, inlier otherwise.  With masks, inter when
//            masks[n][y][x] != 0.  The pixel offers (bits(r) << 32) | n to the composite word of (y, x): the nearest pose wins, and
//            on a depth tie the lower pose index.
//   area     n_mask[n] = the number of non-zero bytes of masks[n] over the whole image.
//   resolve  ids[y][x] = the lower half of the composite word, -1 where it is empty; depth_out[y][x] = the float of its upper half,
//            0 where it is empty.
//   counts   (N,8) i32: n_render, n_inlier, n_occluded, n_behind, n_unknown, n_mask, n_inter, n_dropped.  Columns 1 .. 4 sum to
//            column 0; columns 5 and 6 are 0 without masks.  total == 0 (no pose has a window): every column is 0, ids is -1 and
//            depth_out 0 everywhere, and no raster pass is launched -- so column 7 is the raster pass's count and 0 in that case
//            (sam6d_pose_windows' n_dropped is the count that does not depend on the other poses).
//
//  c. picture (sam6d_overlay_instances).  canvas is (H, 2W, 3) u8: columns 0 .. W-1 are rgb unchanged, as in overlay.hip.  Per pixel of
//     the right half, with id = ids[y][x] and an id outside [0, N) counted as -1:
//   fill     id >= 0: channel c = (rgb_c * (256 - alpha) + color[id]_c * alpha + 128) >> 8, alpha an integer in 0 .. 256.
//   edge     id >= 0 and one of the four neighbours INSIDE THE IMAGE has another id (counted the same way): color[id]_c unblended.
//            That is the silhouette and the line between two instances; the image border alone is no edge.
//   else     id = -1: rgb_c.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  Every place where workgroups meet is an integer atomic at agent scope: 32-bit
// min / max (the boxes), 32-bit add (the counters), 64-bit min (the z-buffers and the composite), all of them commutative and
// associative, so the word ends with the same value in whatever order they land.  The buffers are initialised by memsets that precede
// the kernels in stream order, nothing reads a buffer in the launch that reduces into it, and every output element has one writer:
// windows_finish_kernel for box, the counters' atomics for counts, verify_resolve_kernel for ids and depth_out, the gather for canvas.
//
// WORK.  windows and raster: one wave per 64 faces of a pose, as raster_faces_kernel; the raster pass has its thread path (a face
// whose clamped box has fewer than wave_area pixels is walked by its lane) and wave path (the rest, 64 pixels at a time).  Counters
// and boxes are reduced inside the wave first (ballot and popcount, shuffles), then at most one atomic per wave and counter.  The
// words all waves of a pose meet at (its box, its counters) lie in one cache line, and 200 poses in a few: windows and classify
// therefore run sixteen waves to a workgroup and reduce once more in LDS, so that one atomic per workgroup and word is left.  (With
// one per wave, the 256 000 waves of an 81 920-face mesh at 200 poses met at 25 cache lines and the windows took 1.9 ms, per workgroup
// 0.23 ms; classify of 200 whole-image windows went from 33 ms to 3.8 ms.)  classify: one thread per window word of all poses -- the
// grid is sized by the sum of the windows, never by the largest; a workgroup finds the pose of its first word in `offset` by
// bisection and its threads step forward from there.  area: 16 bytes per thread and step.
//
// FILES.  raster.h: setup, coverage, weights and the raster pass.  verify_raster.h, shared with refine.hip: the window, its sink and
// verify_faces_kernel; the walk from a window word to its pose and pixel (vf_first_pose, vf_word) and the loop over the poses present
// in a wave (vf_each_pose) that classify runs.  common.h: the integer wave reductions.  The limits are raster.hip's rs_limits.
//
// WHAT THE HOST CANNOT SEE.  box and offset are on the device, so the kernels guard themselves: the window is the box clamped to the
// image, a face's box is clamped to the window, a word at or beyond `total` (or below 0) is never addressed, and a window word whose
// index within its pose is at or beyond bw * bh is skipped.  Inconsistent boxes and offsets give meaningless counts, never an access
// outside the buffers.
#include "verify_raster.h"  // the window and the raster pass of b, shared with refine.hip
#include "../../include/sam6d_hip.h"

// ---------------------------------------------------------------------------------------------------------- a. windows
#define VF_WG 1024  // sixteen waves: what meets at a pose's few words is one offer per workgroup, not one per wave
#define VF_WAVES (VF_WG / 64)

// grid (ceil(F / 1024), N): one wave per 64 faces of a pose, sixteen of them in a workgroup.  box arrives with every bit set: the
// largest unsigned for the minima, -1 for the maxima
__global__ __launch_bounds__(VF_WG) void windows_faces_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int F,
                                                              const float* __restrict__ view, RsCam cam, int* __restrict__ box,
                                                              int* __restrict__ n_dropped) {
  __shared__ int red[VF_WAVES][5];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int face = blockIdx.x * VF_WG + tid;
  RsFace f;
  f.live = false;
  f.dropped = false;
  f.x0 = f.y0 = 0;
  f.x1 = f.y1 = -1;
  if (face < F) rs_setup(f, vert, V, faces, face, view + (size_t)n * 12, cam);
  const bool boxed = f.live && f.x0 <= f.x1 && f.y0 <= f.y1;
  // inside the wave first: ballot and popcount for the counter, shuffles for the box (no boxed face: x0 = y0 = INT_MAX, x1 = y1 = -1)
  const int w_dropped = __popcll(__ballot(f.dropped));
  const int w_x0 = wave_min(boxed ? f.x0 : 0x7fffffff), w_y0 = wave_min(boxed ? f.y0 : 0x7fffffff);
  const int w_x1 = wave_max(boxed ? f.x1 : -1), w_y1 = wave_max(boxed ? f.y1 : -1);
  if (lane == 0) {
    red[wave][0] = w_dropped;
    red[wave][1] = w_x0;
    red[wave][2] = w_y0;
    red[wave][3] = w_x1;
    red[wave][4] = w_y1;
  }
  __syncthreads();
  if (tid != 0) return;
  int dropped = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
  for (int w = 0; w < VF_WAVES; ++w) {
    dropped += red[w][0];
    x0 = min(x0, red[w][1]);
    y0 = min(y0, red[w][2]);
    x1 = max(x1, red[w][3]);
    y1 = max(y1, red[w][4]);
  }
  if (dropped) vf_add(n_dropped + n, dropped);
  if (x1 < 0) return;  // no boxed face in the workgroup
  int* b = box + (size_t)n * 4;
  __hip_atomic_fetch_min((unsigned*)b, (unsigned)x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // x0, y0 >= 0: ordered as unsigned
  __hip_atomic_fetch_min((unsigned*)b + 1, (unsigned)y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(b + 2, x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(b + 3, y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per pose: a pose without a boxed face gets [0, 0, -1, -1]
__global__ __launch_bounds__(256) void windows_finish_kernel(int* __restrict__ box, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int* b = box + (size_t)n * 4;
  if (b[2] < 0 || b[3] < 0) {
    b[0] = b[1] = 0;
    b[2] = b[3] = -1;
  }
}

// vf_check, the limits every entry of this file shares: verify_raster.h

extern "C" int sam6d_pose_windows(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy,
                                  float cx, float cy, int H, int W, float near, int* box, int* n_dropped, void* stream) {
  const int bad = vf_check("pose_windows", V, F, N, H, W, near);
  if (bad) return bad;
  SAM6D_REQUIRE(vertices && faces && view && box && n_dropped, "pose_windows: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  hipError_t e = hipMemsetAsync(box, 0xff, (size_t)N * 4 * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(n_dropped, 0, (size_t)N * sizeof(int), s);
  if (e != hipSuccess) {
    sam6d_set_error("pose_windows: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(windows_faces_kernel, dim3((F + VF_WG - 1) / VF_WG, N), dim3(VF_WG), 0, s, vertices, V, faces, F, view, cam, box, n_dropped);
  SAM6D_LAUNCH_CHECK_CONT("pose_windows (faces)");
  hipLaunchKernelGGL(windows_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, s, box, N);
  SAM6D_LAUNCH_CHECK("pose_windows (finish)");
}

// ---------------------------------------------------------------------------------------------------------- b. verify
// the window, its sink and verify_faces_kernel (the raster pass), the word walk and the per-pose loop: verify_raster.h

// one thread per window word of all poses, sixteen waves in a workgroup.  Most workgroups lie inside one window: the counts of the
// pose of the workgroup's first word are gathered in LDS and leave as one atomic per counter and workgroup; a wave's counts for
// another pose (a window that begins inside the workgroup) leave as one atomic per counter and wave.
__global__ __launch_bounds__(VF_WG) void verify_classify_kernel(const unsigned long long* __restrict__ zbuf, long long total,
                                                                const int* __restrict__ box, const long long* __restrict__ offset, int N,
                                                                int H, int W, const float* __restrict__ depth_obs,
                                                                const unsigned char* __restrict__ masks, float tau, int composite,
                                                                unsigned long long* __restrict__ comp, int* __restrict__ counts) {
  __shared__ int wg[6];  // n_render, n_inlier, n_occluded, n_behind, n_unknown, n_inter of pose nb
  const long long base = (long long)blockIdx.x * VF_WG, i = base + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 6) wg[threadIdx.x] = 0;
  const int nb = vf_first_pose(offset, N, base);
  int cls = 0, inter = 0;  // cls: 0 nothing to count, 1 inlier, 2 occluded, 3 behind, 4 unknown
  VfPixel px;
  if (vf_word(zbuf, total, box, offset, N, H, W, i, nb, px)) {
    const float o = depth_obs[px.p];
    if (!(o > 0.f)) cls = 4;
    else {
      const float e = o - px.r();
      cls = e > tau ? 3 : (e < -tau ? 2 : 1);
    }
    if (masks) inter = masks[(size_t)px.n * H * W + px.p] != 0;
    if (composite)
      __hip_atomic_fetch_min(comp + px.p, (px.key & 0xffffffff00000000ull) | (unsigned)px.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();  // wg is zero
  // per pose present in the wave: ballot and popcount, then one add per counter
  int* const wg_of_nb = wg;
  vf_each_pose(cls != 0, px.n, [=](int lead, int pn, bool mine, unsigned long long m) {
    const int c[6] = {(int)__popcll(m),
                      (int)__popcll(__ballot(mine && cls == 1)),
                      (int)__popcll(__ballot(mine && cls == 2)),
                      (int)__popcll(__ballot(mine && cls == 3)),
                      (int)__popcll(__ballot(mine && cls == 4)),
                      (int)__popcll(__ballot(mine && inter))};
    if (lane != lead) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (!c[k]) continue;
      if (pn == nb) atomicAdd(&wg_of_nb[k], c[k]);
      else vf_add(counts + (size_t)pn * 8 + (k < 5 ? k : 6), c[k]);
    }
  });
  __syncthreads();
  if (threadIdx.x < 6 && wg[threadIdx.x]) vf_add(counts + (size_t)nb * 8 + (threadIdx.x < 5 ? threadIdx.x : 6), wg[threadIdx.x]);
}

// the bytes of a 32-bit word that are not zero
__device__ __forceinline__ int vf_nonzero_bytes(unsigned w) {
  return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u);
}

#define VF_AREA_STEPS 8
// grid (ceil(chunks / (256 * VF_AREA_STEPS)), N): chunk c of pose n is the 16 bytes at the 16-byte aligned address
// (masks[n] rounded down) + 16 c; a chunk that lies wholly inside masks[n] is one 16-byte load, the two at the ends go byte by byte
__global__ __launch_bounds__(256) void verify_mask_area_kernel(const unsigned char* __restrict__ masks, long long hw, int* __restrict__ counts) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const unsigned char* m = masks + (size_t)n * hw;
  const long long lead = (long long)((uintptr_t)m & 15);  // bytes of chunk 0 that lie before masks[n]
  const long long chunks = (hw + lead + 15) / 16;
  int cnt = 0;
  for (int k = 0; k < VF_AREA_STEPS; ++k) {
    const long long c = ((long long)blockIdx.x * VF_AREA_STEPS + k) * 256 + threadIdx.x;
    if (c >= chunks) break;
    const long long b0 = c * 16 - lead, b1 = b0 + 16;  // byte range within masks[n]
    if (b0 >= 0 && b1 <= hw) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(m + b0);
      cnt += (vf_nonzero_bytes(v[0]) + vf_nonzero_bytes(v[1])) + (vf_nonzero_bytes(v[2]) + vf_nonzero_bytes(v[3]));
    } else {
      const long long e0 = b0 < 0 ? 0 : b0, e1 = b1 > hw ? hw : b1;
      for (long long b = e0; b < e1; ++b) cnt += m[b] != 0;
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0 && cnt) vf_add(counts + (size_t)n * 8 + 5, cnt);
}

// one thread per pixel: the only writer of ids and depth_out
__global__ __launch_bounds__(256) void verify_resolve_kernel(const unsigned long long* __restrict__ comp, int hw, int* __restrict__ ids,
                                                             float* __restrict__ depth_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const unsigned long long key = comp[i];
  const bool empty = key == VF_EMPTY;
  if (ids) ids[i] = empty ? -1 : (int)(unsigned)(key & 0xffffffffull);
  if (depth_out) depth_out[i] = empty ? 0.f : __uint_as_float((unsigned)(key >> 32));
}

extern "C" size_t sam6d_pose_verify_workspace_bytes(long total, int H, int W) {
  if (H < 1 || H > RS_MAX_HW || W < 1 || W > RS_MAX_HW || total < 0 || total > (long)VF_MAX_N * H * W) return 0;
  return ((size_t)total + (size_t)H * W) * sizeof(unsigned long long);
}

extern "C" int sam6d_pose_verify(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy,
                                 float cx, float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset,
                                 long total, const float* depth_obs, const unsigned char* masks, float tau, int* counts, int* ids,
                                 float* depth_out, void* workspace, size_t workspace_bytes, void* stream) {
  const int bad = vf_check("pose_verify", V, F, N, H, W, near);
  if (bad) return bad;
  SAM6D_REQUIRE(wave_area >= 0, "pose_verify: wave_area = %d is negative", wave_area);
  SAM6D_REQUIRE(tau >= 0.f && tau <= 3.4028234e38f, "pose_verify: tau = %g is not a finite number >= 0", (double)tau);
  SAM6D_REQUIRE(total >= 0 && total <= (long)N * H * W, "pose_verify: total = %ld is not in 0 .. N H W = %ld", total, (long)N * H * W);
  SAM6D_REQUIRE(vertices && faces && view && box && offset && depth_obs && counts && workspace, "pose_verify: null pointer");
  const size_t need = sam6d_pose_verify_workspace_bytes(total, H, W);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_verify: workspace of %zu bytes is below sam6d_pose_verify_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "pose_verify: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  const int hw = H * W;  // at most 2^22
  unsigned long long* zbuf = (unsigned long long*)workspace;
  unsigned long long* comp = zbuf + total;
  const int composite = (ids || depth_out) ? 1 : 0;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * 8 * sizeof(int), s);
  if (e == hipSuccess && (total > 0 || composite)) e = hipMemsetAsync(workspace, 0xff, composite ? need : (size_t)total * 8, s);
  if (e != hipSuccess) {
    sam6d_set_error("pose_verify: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (total > 0) {
    hipLaunchKernelGGL(verify_faces_kernel, dim3((F + 63) / 64, N), dim3(64), 0, s, vertices, V, faces, F, view, cam,
                       wave_area ? wave_area : RS_WAVE_AREA, box, offset, (long long)total, zbuf, counts);
    SAM6D_LAUNCH_CHECK_CONT("pose_verify (faces)");
    // total <= 2^32: at most 2^22 blocks
    hipLaunchKernelGGL(verify_classify_kernel, dim3((unsigned)((total + VF_WG - 1) / VF_WG)), dim3(VF_WG), 0, s, zbuf, (long long)total, box, offset, N,
                       H, W, depth_obs, masks, tau, composite, comp, counts);
    SAM6D_LAUNCH_CHECK_CONT("pose_verify (classify)");
    if (masks) {
      const int chunks = hw / 16 + 2;
      hipLaunchKernelGGL(verify_mask_area_kernel, dim3((chunks + 256 * VF_AREA_STEPS - 1) / (256 * VF_AREA_STEPS), N), dim3(256), 0, s, masks,
                         (long long)hw, counts);
      SAM6D_LAUNCH_CHECK_CONT("pose_verify (mask area)");
    }
  }
  if (!composite) return 0;
  hipLaunchKernelGGL(verify_resolve_kernel, dim3((hw + 255) / 256), dim3(256), 0, s, comp, hw, ids, depth_out);
  SAM6D_LAUNCH_CHECK("pose_verify (resolve)");
}

// ---------------------------------------------------------------------------------------------------------- c. picture
// one thread per pixel: the only writer of the pixel's six canvas bytes
__global__ __launch_bounds__(256) void overlay_instances_kernel(const unsigned char* __restrict__ rgb, long row_stride, int H, int W,
                                                                const int* __restrict__ ids, const unsigned char* __restrict__ colors, int N,
                                                                int alpha, unsigned char* __restrict__ canvas) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i % W;
  const unsigned char* src = rgb + (size_t)y * row_stride + (size_t)x * 3;
  unsigned char* row = canvas + (size_t)y * 2 * W * 3;
  unsigned char* left = row + (size_t)x * 3;
  unsigned char* dst = row + (size_t)(W + x) * 3;
  left[0] = src[0];
  left[1] = src[1];
  left[2] = src[2];
  const int* p = ids + i;
  const auto norm = [N](int v) { return (unsigned)v < (unsigned)N ? v : -1; };
  const int id = norm(p[0]);
  if (id < 0) {
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    return;
  }
  bool edge = false;
  if (y > 0) edge = edge || norm(p[-W]) != id;
  if (y + 1 < H) edge = edge || norm(p[W]) != id;
  if (x > 0) edge = edge || norm(p[-1]) != id;
  if (x + 1 < W) edge = edge || norm(p[1]) != id;
  const unsigned char* col = colors + (size_t)id * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = edge ? col[c] : (unsigned char)(((int)src[c] * (256 - alpha) + (int)col[c] * alpha + 128) >> 8);
}

extern "C" int sam6d_overlay_instances(const unsigned char* rgb, long row_stride, int H, int W, const int* ids, const unsigned char* colors,
                                       int N, int alpha, unsigned char* canvas, void* stream) {
  SAM6D_REQUIRE(H >= 1 && H <= RS_MAX_HW && W >= 1 && W <= RS_MAX_HW, "overlay_instances: H x W = %d x %d is not in 1 .. %d", H, W, RS_MAX_HW);
  SAM6D_REQUIRE(N >= 1 && N <= VF_MAX_N, "overlay_instances: N = %d is not in 1 .. %d", N, VF_MAX_N);
  SAM6D_REQUIRE(alpha >= 0 && alpha <= 256, "overlay_instances: alpha = %d is not in 0 .. 256", alpha);
  SAM6D_REQUIRE(row_stride >= 3L * W, "overlay_instances: row_stride = %ld is below 3 W = %ld", row_stride, 3L * W);
  SAM6D_REQUIRE(rgb && ids && colors && canvas, "overlay_instances: null pointer");
  hipLaunchKernelGGL(overlay_instances_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, rgb, row_stride, H, W, ids, colors,
                     N, alpha, canvas);
  SAM6D_LAUNCH_CHECK("overlay_instances");
}
