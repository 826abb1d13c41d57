// All-pairs VSD: the counts of BOP's Visible Surface Discrepancy (Hodan et al., "BOP Challenge 2020 on 6D Object Localization",
// section 2.2) of every estimate a[i] against every ground truth b[j] of one object, from ONE render per pose.  The reference has no
// evaluation code: it writes its poses (PEM/run_inference_custom_pytorch.py:460-471) and leaves the scoring to bop_toolkit.  For every
// (i, j) the counts are, bit for bit, what sam6d_pose_vsd (poseerr.hip) gives for est = a[i], gt = b[j]; they are pinned against the
// numpy restatement tests/vsdpairs_ref.py and against that entry on the expanded pairs, NOT against bop_toolkit.
//
// RECIPE.  In terms of poseerr.hip RECIPE b, whose per-pixel quantities these are operation for operation: IEEE fp32 in the order
// written (the library is built with -ffp-contract=off and this file has no fused multiply-add), everything else is integer.
//
//  a. raster.  A + B views, 0 .. A-1 the estimates a, A .. A+B-1 the ground truths b, each rastered into ITS OWN window (box[n] of
//     sam6d_pose_windows clamped to the image, words offset[n] ..) by verify_faces_kernel unchanged (verify.hip RECIPE b).
//  b. view pass, per view n and window word at pixel (x, y) with the key's depth r, or absent:
//   has      the word holds a key.
//   reading  o = depth_obs[y][x] is one when o > 0 (false also for a NaN).
//   distance c = sqrtf((ax ax + ay ay) + 1) with ax = ((float)x - cx) / fx, ay = ((float)y - cy) / fy; D = r * c, D_o = o * c.
//   own      = has && (!reading || D - D_o <= delta).
//   image    the 32-bit word of the pixel: 0 without a key, else the bits of D with `own` in the sign bit.  (D > 0 or a NaN whenever
//            near > 0: r >= near and c >= 1.  The D the pair pass compares is the word without its sign bit: the fp32 above, and a
//            NaN stays a NaN.)
//   counts   view_counts[n] = n_render (#has), n_visible (#own).
//  c. pair pass, per (i, j) with e = view i, g = view A + j, E_i = n_visible of e, G_j = n_visible of g, and X the intersection
//     rectangle of the two windows:
//   n_visib_gt  = G_j
//   n_inter     = #X{has_e && own_g}
//   n_visib_est = E_i + #X{has_e && !own_e && own_g}
//   n_union     = n_visib_est + G_j - n_inter
//   cost_k      = #X{has_e && own_g && fabsf(D_g - D_e) * inv_norm >= taus[k]}
//   counts (A, B, 4 + T) i32 = n_union, n_inter, n_visib_est, n_visib_gt, cost_0 .. cost_{T-1}.  total == 0: all 0, no pass runs.
//
// WHY THE SPLIT IS AN IDENTITY.  A z-buffer key depends on the view and the pixel only, not on the window: verify_raster.h's sink
// only clamps a face's pixel box to the window, and a view's own window holds every pixel the view can cover.  So in the pair's union
// window (poseerr.hip's) each view has, at every pixel, the key it has here, and none outside its own window.  With that recipe's
// terms, visib_gt = has_g && (!reading || D_g - D_o <= delta) = own_g.  visib_est = has_e && (!reading || D_e - D_o <= delta ||
// visib_gt) = own_e || (has_e && own_g).  inter = visib_est && visib_gt = has_e && own_g, because own_e implies has_e.  Counting:
// #visib_gt = G_j; #visib_est = #own_e + #{has_e && !own_e && own_g}, two disjoint sets; the second set and inter need has_e and
// has_g at once, which only pixels of X have.  The union is counted by inclusion and exclusion.  All of these are integers.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  Raster and view_counts: where workgroups meet it is an integer atomic at agent
// scope, 64-bit minima (the z-buffer) and 32-bit adds (the counters), commutative and associative, into buffers set by memsets that
// precede the kernels in stream order.  Every image word below `total` has one writer, its thread of the view pass.  A pair has one
// owner, one workgroup, which sums integers and writes the pair's row of counts with plain stores: no atomics and no memset of counts.
// Nothing reads a buffer in the launch that writes it.
//
// WORK.  A + B renders where the pair entry has 2 A B, and one square root and two divisions per view pixel, not per pair pixel.  View
// pass: one thread per window word of all views, sixteen waves to a workgroup, the two counters reduced as vsd_compare_kernel reduces
// its own.  Pair pass: one workgroup of four waves per pair, i fastest over neighbouring workgroups, so that the A readers of ground
// truth j's window meet in L2.  The workgroup walks X 256 pixels at a time and reads 4 bytes per view and pixel (the 32-bit image,
// half the traffic of the 8-byte keys); the 2 + T counters are ballots and popcounts, kept in scalar registers.  A pair whose windows
// do not meet reads no pixel and writes [E_i + G_j, 0, E_i, G_j, 0, ...].  One owner per pair was chosen over a split of X with
// atomics because the matrix is the case with many pairs; a call of a few pairs with image-sized windows is served by four waves a
// pair, which is slow and still exact.
//
// WHAT THE HOST CANNOT SEE.  box and offset are on the device: a window is the box clamped to the image, X is the intersection of two
// such windows, no word at or beyond `total` (or below 0) is addressed whatever they hold, in the z-buffer or in the image, and counts
// and view_counts are addressed by (i, j) and a view index in range alone.  Inconsistent boxes and offsets give meaningless counts,
// never an access outside the buffers.
#include "verify_raster.h"
#include "poseerr_point.h"  // PeCam, PeTaus and the refusals the two VSD entries share
#include "../../include/sam6d_hip.h"

#define VP_MAX_POSES 1024           // A and B, each
#define VP_VIEW_WG 1024             // sixteen waves, as vsd_compare_kernel: one offer per workgroup at a view's counters
#define VP_PAIR_WG 256              // four waves own a pair
#define VP_PAIR_WAVES (VP_PAIR_WG / 64)
#define VP_OWN 0x80000000u

// ---------------------------------------------------------------------------------------------------------- b. view pass
// One thread per window word of all NV = A + B views (the grid is sized by `total`, the host's figure).  Every image word below
// total is written, 0 where vf_word finds no pixel.  The counts of the view of the workgroup's first word are gathered in LDS and
// leave as one atomic per counter and workgroup, a wave's counts for another view as one atomic per counter and wave.
__global__ __launch_bounds__(VP_VIEW_WG) void vsd_view_kernel(const unsigned long long* __restrict__ zbuf, long long total,
                                                              const int* __restrict__ box, const long long* __restrict__ offset, int NV,
                                                              int H, int W, const float* __restrict__ depth_obs, PeCam cam, float delta,
                                                              unsigned* __restrict__ image, int* __restrict__ view_counts) {
  __shared__ int wg[2];
  const long long base = (long long)blockIdx.x * VP_VIEW_WG, i = base + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 2) wg[threadIdx.x] = 0;
  const int nb = vf_first_pose(offset, NV, base);
  VfPixel px;
  const bool has = vf_word(zbuf, total, box, offset, NV, H, W, i, nb, px);
  bool own = false;
  unsigned word = 0;
  if (has) {
    const float o = depth_obs[px.p];
    const bool reading = o > 0.f;
    const float ax = ((float)px.x - cam.cx) / cam.fx, ay = ((float)px.y - cam.cy) / cam.fy;
    const float c = sqrtf((ax * ax + ay * ay) + 1.f);
    const float D = px.r() * c, Do = o * c;
    own = !reading || D - Do <= delta;
    word = (__float_as_uint(D) & ~VP_OWN) | (own ? VP_OWN : 0u);
  }
  if (i < total) image[i] = word;
  __syncthreads();  // wg is zero
  int* const wg_of_nb = wg;
  vf_each_pose(has, px.n, [=](int lead, int pn, bool mine, unsigned long long m) {
    const int c[2] = {(int)__popcll(m), (int)__popcll(__ballot(mine && own))};
    if (lane != lead) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!c[k]) continue;
      if (pn == nb) atomicAdd(&wg_of_nb[k], c[k]);
      else vf_add(view_counts + (size_t)pn * 2 + k, c[k]);
    }
  });
  __syncthreads();
  if (threadIdx.x < 2 && wg[threadIdx.x]) vf_add(view_counts + (size_t)nb * 2 + threadIdx.x, wg[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------- c. pair pass
// the image word of pixel (x, y) of window w, 0 where the word would lie at or beyond total (unsigned: whatever the offset holds, no
// overflow).  (x, y) is inside w, so the index within the window is below 2^22.
__device__ __forceinline__ unsigned vp_word(const unsigned* __restrict__ image, long long total, const VfWin& w, int x, int y) {
  const unsigned long long at = (unsigned long long)w.off + (unsigned long long)((long long)(y - w.y0) * w.bw + (x - w.x0));
  return at < (unsigned long long)total ? image[at] : 0u;
}

// grid A B, workgroup p owns pair (i, j) = (p % A, p / A).  X is walked in row-major order, pixel q = threadIdx.x + 256 s at step s;
// from one step to the next a thread moves by 256 = dq xw + dr pixels, so (x, y) advance without a division.  The loop count is
// uniform over the workgroup, so every ballot has all lanes of its wave.
__global__ __launch_bounds__(VP_PAIR_WG) void vsd_pair_kernel(const unsigned* __restrict__ image, long long total, const int* __restrict__ box,
                                                              const long long* __restrict__ offset, int A, int B, int H, int W, PeTaus taus,
                                                              int T, float inv_norm, const int* __restrict__ view_counts,
                                                              int* __restrict__ counts) {
  __shared__ int red[VP_PAIR_WAVES][2 + PE_MAX_T];
  const int i = blockIdx.x % A, j = blockIdx.x / A;  // j < B: the grid is A B
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const VfWin we = vf_window(box, offset, i, H, W), wg = vf_window(box, offset, A + j, H, W);
  const int xs = max(we.x0, wg.x0), ys = max(we.y0, wg.y0);
  const int xw = max(min(we.x0 + we.bw, wg.x0 + wg.bw) - xs, 0), xh = max(min(we.y0 + we.bh, wg.y0 + wg.bh) - ys, 0);  // an empty window: 0
  const int area = xw * xh;  // at most 2^22
  int n_inter = 0, n_extra = 0, cost[PE_MAX_T];
#pragma unroll
  for (int k = 0; k < PE_MAX_T; ++k) cost[k] = 0;
  if (area > 0) {
    const int dq = VP_PAIR_WG / xw, dr = VP_PAIR_WG % xw;
    int x = (int)threadIdx.x % xw, y = (int)threadIdx.x / xw;
    for (int q = threadIdx.x; q - (int)threadIdx.x < area; q += VP_PAIR_WG) {
      bool inter = false, extra = false;
      float err = 0.f;
      if (q < area) {
        const unsigned e = vp_word(image, total, we, xs + x, ys + y), g = vp_word(image, total, wg, xs + x, ys + y);
        const bool has_e = (e & ~VP_OWN) != 0, own_e = has_e && (e & VP_OWN), own_g = (g & ~VP_OWN) != 0 && (g & VP_OWN);
        inter = has_e && own_g;
        extra = inter && !own_e;
        err = fabsf(__uint_as_float(g & ~VP_OWN) - __uint_as_float(e & ~VP_OWN)) * inv_norm;
      }
      n_inter += (int)__popcll(__ballot(inter));
      n_extra += (int)__popcll(__ballot(extra));
#pragma unroll
      for (int k = 0; k < PE_MAX_T; ++k)
        if (k < T) cost[k] += (int)__popcll(__ballot(inter && err >= taus.v[k]));
      x += dr;
      y += dq;
      if (x >= xw) {
        x -= xw;
        ++y;
      }
    }
  }
  if (lane == 0) {
    red[wave][0] = n_inter;
    red[wave][1] = n_extra;
#pragma unroll
    for (int k = 0; k < PE_MAX_T; ++k) red[wave][2 + k] = cost[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= 4 + T) return;
  const int E = view_counts[(size_t)i * 2 + 1], G = view_counts[(size_t)(A + j) * 2 + 1];
  const auto sum = [&](int c) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < VP_PAIR_WAVES; ++w) s += red[w][c];
    return s;
  };
  const int inter = sum(0), visib_est = E + sum(1);
  counts[((size_t)i * B + j) * (4 + T) + k] = k == 0 ? visib_est + G - inter : k == 1 ? inter : k == 2 ? visib_est : k == 3 ? G : sum(k - 2);
}

// ---------------------------------------------------------------------------------------------------------- the entry
// workspace: total z-buffer words | total image words, rounded up to a whole 8 bytes | (A+B, 8) i32, the raster pass's counter words
extern "C" size_t sam6d_pose_pair_vsd_workspace_bytes(long total, int A, int B) {
  if (A < 1 || A > VP_MAX_POSES || B < 1 || B > VP_MAX_POSES || total < 0 || total > (long)(A + B) * RS_MAX_HW * RS_MAX_HW) return 0;
  return (size_t)total * 8 + (((size_t)total + 1) / 2) * 8 + (size_t)(A + B) * 8 * sizeof(int);
}

// the refusals are sam6d_pose_vsd's, by name: those of the tolerances are one copy, poseerr_point.h's
extern "C" int sam6d_pose_pair_vsd(const float* vertices, int V, const int* faces, int F, const float* view, int A, int B, float fx, float fy,
                                   float cx, float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset,
                                   long total, const float* depth_obs, float delta, const float* taus, int T, float inv_norm, int* counts,
                                   int* view_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const int bad = rs_limits("pose_pair_vsd", V, F, "A", A, VP_MAX_POSES, H, W, near);
  if (bad) return bad;
  SAM6D_REQUIRE(B >= 1 && B <= VP_MAX_POSES, "pose_pair_vsd: B = %d is not in 1 .. %d", B, VP_MAX_POSES);
  if (const int bad_tol = pe_check_vsd("pose_pair_vsd", wave_area, delta, inv_norm, fx, fy, T)) return bad_tol;
  const int NV = A + B;
  SAM6D_REQUIRE(total >= 0 && total <= (long)NV * H * W, "pose_pair_vsd: total = %ld is not in 0 .. (A + B) H W = %ld", total, (long)NV * H * W);
  SAM6D_POINTER("pose_pair_vsd", vertices);
  SAM6D_POINTER("pose_pair_vsd", faces);
  SAM6D_POINTER("pose_pair_vsd", view);
  SAM6D_POINTER("pose_pair_vsd", box);
  SAM6D_POINTER("pose_pair_vsd", offset);
  SAM6D_POINTER("pose_pair_vsd", depth_obs);
  SAM6D_POINTER("pose_pair_vsd", taus);
  SAM6D_POINTER("pose_pair_vsd", counts);
  SAM6D_POINTER("pose_pair_vsd", view_counts);
  SAM6D_POINTER("pose_pair_vsd", workspace);
  PeTaus tv;
  if (const int bad_tau = pe_check_taus("pose_pair_vsd", taus, T, tv)) return bad_tau;
  const size_t need = sam6d_pose_pair_vsd_workspace_bytes(total, A, B);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_pair_vsd: workspace of %zu bytes is below sam6d_pose_pair_vsd_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "pose_pair_vsd: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  unsigned long long* zbuf = (unsigned long long*)workspace;
  unsigned* image = (unsigned*)(zbuf + total);
  int* dropped = (int*)(zbuf + total + (total + 1) / 2);  // the raster pass's dropped-face counter lives in column 7 of (A+B,8); nothing reads it
  hipError_t e = hipMemsetAsync(view_counts, 0, (size_t)NV * 2 * sizeof(int), s);
  if (e == hipSuccess && total == 0) e = hipMemsetAsync(counts, 0, (size_t)A * B * (4 + T) * sizeof(int), s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(zbuf, 0xff, (size_t)total * 8, s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(dropped, 0, (size_t)NV * 8 * sizeof(int), s);
  SAM6D_MEMSET_CHECK("pose_pair_vsd", e);
  if (total == 0) return 0;
  hipLaunchKernelGGL(verify_faces_kernel, dim3((F + 63) / 64, NV), dim3(64), 0, s, vertices, V, faces, F, view, cam,
                     wave_area ? wave_area : RS_WAVE_AREA, box, offset, (long long)total, zbuf, dropped);
  SAM6D_LAUNCH_CHECK_CONT("pose_pair_vsd (faces)");
  // total <= 2^33: at most 2^23 blocks
  hipLaunchKernelGGL(vsd_view_kernel, dim3((unsigned)((total + VP_VIEW_WG - 1) / VP_VIEW_WG)), dim3(VP_VIEW_WG), 0, s, zbuf, (long long)total, box, offset,
                     NV, H, W, depth_obs, PeCam{fx, fy, cx, cy}, delta, image, view_counts);
  SAM6D_LAUNCH_CHECK_CONT("pose_pair_vsd (views)");
  hipLaunchKernelGGL(vsd_pair_kernel, dim3((unsigned)(A * B)), dim3(VP_PAIR_WG), 0, s, image, (long long)total, box, offset, A, B, H, W, tv, T, inv_norm,
                     view_counts, counts);
  SAM6D_LAUNCH_CHECK("pose_pair_vsd (pairs)");
}
