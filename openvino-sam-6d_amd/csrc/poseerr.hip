// Scoring poses against ground truth: the BOP pose errors MSSD, MSPD and VSD (Hodan et al., "BOP Challenge 2020 on 6D Object
// Localization", section 2.2) and ADD (Hinterstoisser et al. 2012), batched over N pose pairs.  The reference has no evaluation code:
// it writes its poses (PEM/run_inference_custom_pytorch.py:460-471) and leaves the scoring to bop_toolkit.  The definitions are the
// published ones, restated here and pinned against the numpy restatement tests/poseerr_ref.py -- NOT against bop_toolkit, which the
// suite does not have.  VSD renders with the package's own rasteriser (verify.hip's raster pass: verify_raster.h), so it is BOP's in
// kind and not pixel for pixel.  Every comparison with the restatement is bit for bit.
//
// RECIPE.  All float arithmetic is IEEE fp32 in the order written unless float64 is named (the library is built with
// -ffp-contract=off and this file has no fused multiply-add), everything else is integer.
//
//  a. point errors (sam6d_pose_point_errors), per pose n, symmetry s and model point x:
//   G        = gt[n] o syms[s] in float64 from the fp32 factors: G_rc = (gt_r0 S_0c + gt_r1 S_1c) + gt_r2 S_2c, and for c = 3
//            ... + gt_r3 (the products are exact, the sums run left to right), rounded once to fp32.
//   points   e = E x and g = G x with E = est[n]: ((M_r0 x0 + M_r1 x1) + M_r2 x2) + M_r3 (raster.h's rs_to_camera).
//   d2       = (dx dx + dy dy) + dz dz with d = e - g.
//   pixels   u_e = fx * (e0 / e2) + cx, v_e = fy * (e1 / e2) + cy, the same for g; p2 = du du + dv dv with du = u_e - u_g.
//   skipped  a point with e2 > 0 false or g2 > 0 false takes no part in the pair's p2 maximum (it does in the d2 maximum);
//            n_skipped[n] counts such points for s = 0 only.  The package's own rule, as draw_detections' behind-camera rule; BOP
//            divides regardless.  A pair all of whose points are skipped has the p2 maximum 0.
//   maxima   over the points, of the bit patterns: a value > 0 orders as its bits, 0 is 0, and anything else (a NaN) counts as
//            0x7fc00000, above every number.
//   MSSD     mssd[n] = sqrtf(min_s max_x d2), mssd_sym[n] = the lowest s that attains the minimum.  MSPD: the same with p2.
//   ADD      add_sum[n] = sum_x rint(w) with w = ((double)sqrtf(d2 at s = 0) * (double)inv_unit) * 2^30, and w = 2^42 where
//            w <= 2^42 is false (4096 units; also a NaN): a 64-bit integer sum, at most 2^20 * 2^42 = 2^62.
//
//  b. VSD (sam6d_pose_vsd).  2N views: 0 .. N-1 the estimates, N .. 2N-1 the ground truths, rastered into their windows by
//     verify_faces_kernel unchanged (verify.hip RECIPE b).  Both views of a pair have the same window (the caller's: the union of their
//     boxes), so the halves have the same layout and the ground-truth word of word i < offset[N] is i + offset[N].  Per word i of pair
//     n at pixel (x, y), with r_e and r_g the depths in the two keys or absent (has_e, has_g):
//   reading  o = depth_obs[y][x] is one when o > 0 (false also for a NaN, as in verify.hip).
//   distance c = sqrtf((ax ax + ay ay) + 1) with ax = ((float)x - cx) / fx, ay = ((float)y - cy) / fy; D = z * c for r_e, r_g and o.
//   visible  visib_gt = has_g && (!reading || D_g - D_o <= delta);
//            visib_est = has_e && (!reading || D_e - D_o <= delta || visib_gt)           (BOP's visibility mode `bop19`)
//   sets     inter = visib_est && visib_gt, union = visib_est || visib_gt.
//   cost     cost_k = the inter pixels with fabsf(D_g - D_e) * inv_norm >= taus[k]          (BOP's cost type `step`)
//   counts   (N, 4 + T) i32 = n_union, n_inter, n_visib_est, n_visib_gt, cost_0 .. cost_{T-1}.  total == 0: all 0, no pass runs.
//     The caller forms vsd[n][k] = (cost_k + n_union - n_inter) / n_union, and 1 where n_union is 0, as BOP does.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  a: posematch.hip's paragraph of that name, part a; the kernels are its.  b: where
// workgroups meet it is an integer atomic at agent scope: 32-bit adds (the counters) and 64-bit minima (the z-buffer), commutative and
// associative.  The buffers are set by memsets that precede the kernels in stream order, and nothing reads a buffer in the launch
// that reduces into it.
//
// WORK.  point errors: N S V point transforms, by posematch.hip's pair kernels on the diagonal (its WORK a, with A = N, B = 1 and b's
// row taken from i).  VSD: verify_faces_kernel, then one thread per window word of the estimates' half, sixteen waves to a workgroup,
// the counters reduced per pose inside the wave and then in LDS as verify_classify_kernel does.
//
// WHAT THE HOST CANNOT SEE.  box and offset are on the device: the window is the box clamped to the image, no word at or beyond
// `total` (or below 0) is addressed whatever they hold, and counts is addressed by a pose index in [0, N) alone.  Inconsistent boxes
// and offsets give meaningless counts, never an access outside the buffers.
#include "verify_raster.h"
#include "poseerr_point.h"
#include "../../include/sam6d_hip.h"

#define PE_MAX_V (1 << 20)
#define PE_MAX_N 1024
#define PE_MAX_S 1024
#define PE_MAX_PAIRS 512
#define PE_VSD_WG 1024              // sixteen waves, as verify.hip's classify: one offer per workgroup at a pose's counters

// ---------------------------------------------------------------------------------------------------------- a. point errors
// The kernels are posematch.hip's: est[n] against gt[n] o syms[s] is the diagonal of its all-pairs walk (poseerr_point.h's pe_errors).
extern "C" size_t sam6d_pose_point_errors_workspace_bytes(int N, int S) {
  if (N < 1 || N > PE_MAX_N || S < 1 || S > PE_MAX_S) return 0;
  return (size_t)N * S * 2 * sizeof(unsigned);
}

extern "C" int sam6d_pose_point_errors(const float* points, int V, const float* est, const float* gt, int N, const float* syms, int S,
                                       float fx, float fy, float cx, float cy, float inv_unit, float* mssd, float* mspd, int* mssd_sym,
                                       int* mspd_sym, int* n_skipped, long long* add_sum, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  SAM6D_REQUIRE(V >= 1 && V <= PE_MAX_V, "pose_point_errors: V = %d is not in 1 .. %d", V, PE_MAX_V);
  SAM6D_REQUIRE(N >= 1 && N <= PE_MAX_N, "pose_point_errors: N = %d is not in 1 .. %d", N, PE_MAX_N);
  SAM6D_REQUIRE(S >= 1 && S <= PE_MAX_S, "pose_point_errors: S = %d is not in 1 .. %d", S, PE_MAX_S);
  if (const int bad = pe_check_inv_unit("pose_point_errors", inv_unit)) return bad;
  SAM6D_POINTER("pose_point_errors", points);
  SAM6D_POINTER("pose_point_errors", est);
  SAM6D_POINTER("pose_point_errors", gt);
  SAM6D_POINTER("pose_point_errors", syms);
  SAM6D_POINTER("pose_point_errors", mssd);
  SAM6D_POINTER("pose_point_errors", mspd);
  SAM6D_POINTER("pose_point_errors", mssd_sym);
  SAM6D_POINTER("pose_point_errors", mspd_sym);
  SAM6D_POINTER("pose_point_errors", n_skipped);
  SAM6D_POINTER("pose_point_errors", add_sum);
  SAM6D_POINTER("pose_point_errors", workspace);
  const size_t need = sam6d_pose_point_errors_workspace_bytes(N, S);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_point_errors: workspace of %zu bytes is below sam6d_pose_point_errors_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)add_sum & 7) == 0, "pose_point_errors: workspace or add_sum is not 8-byte aligned");
  return pe_errors("pose_point_errors", points, V, est, N, gt, 1, true, syms, S, PeCam{fx, fy, cx, cy}, inv_unit, true, mssd, mspd, mssd_sym, mspd_sym,
                   n_skipped, add_sum, workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------- b. VSD
// One thread per window word of the estimates' half (the grid is sized by `total`, the host's figure; a workgroup beyond the half
// leaves at once), sixteen waves in a workgroup.  The walk from word i to its pair and pixel is vf_word's, without its test of the
// key: a pixel counts when either key of the pair is there.  The counts of the pair of the workgroup's first word are gathered in
// LDS and leave as one atomic per counter and workgroup, a wave's counts for another pair as one atomic per counter and wave.
__global__ __launch_bounds__(PE_VSD_WG) void vsd_compare_kernel(const unsigned long long* __restrict__ zbuf, long long total,
                                                            const int* __restrict__ box, const long long* __restrict__ offset, int N, int H,
                                                            int W, const float* __restrict__ depth_obs, PeCam cam, float delta, PeTaus taus,
                                                            int T, float inv_norm, int* __restrict__ counts) {
  __shared__ int wg[4 + PE_MAX_T];
  const long long half = offset[N];
  const long long lim = half < total ? half : total;  // words of the estimates' half that exist
  const long long base = (long long)blockIdx.x * PE_VSD_WG, i = base + threadIdx.x;
  if (base >= lim) return;  // (uniform over the workgroup; also a negative half)
  const int lane = threadIdx.x & 63, C = 4 + T;
  if (threadIdx.x < C) wg[threadIdx.x] = 0;
  const int nb = vf_first_pose(offset, N, base);
  int n = nb;
  bool uni = false, inter = false, v_e = false, v_g = false;
  float err = 0.f;
  if (i < lim) {
    while (n + 1 < N && offset[n + 1] <= i) ++n;
    const VfWin w = vf_window(box, offset, n, H, W);
    const long long local = i - w.off;
    const unsigned long long j = (unsigned long long)i + (unsigned long long)half;  // (unsigned: whatever offset[N] holds, no overflow)
    if (local >= 0 && local < (long long)w.bw * w.bh) {
      const unsigned long long ke = zbuf[i];
      const unsigned long long kg = j < (unsigned long long)total ? zbuf[j] : VF_EMPTY;
      const bool has_e = ke != VF_EMPTY, has_g = kg != VF_EMPTY;
      if (has_e || has_g) {
        const int y = w.y0 + (int)(local / w.bw), x = w.x0 + (int)(local % w.bw);
        const float o = depth_obs[(size_t)y * W + x];
        const bool reading = o > 0.f;
        const float ax = ((float)x - cam.cx) / cam.fx, ay = ((float)y - cam.cy) / cam.fy;
        const float c = sqrtf((ax * ax + ay * ay) + 1.f);
        const float De = __uint_as_float((unsigned)(ke >> 32)) * c, Dg = __uint_as_float((unsigned)(kg >> 32)) * c, Do = o * c;
        v_g = has_g && (!reading || Dg - Do <= delta);
        v_e = has_e && (!reading || De - Do <= delta || v_g);
        inter = v_e && v_g;
        uni = v_e || v_g;
        err = fabsf(Dg - De) * inv_norm;
      }
    }
  }
  __syncthreads();  // wg is zero
  int* const wg_of_nb = wg;
  vf_each_pose(uni, n, [=](int lead, int pn, bool mine, unsigned long long m) {
    int c[4 + PE_MAX_T];
    c[0] = (int)__popcll(m);
    c[1] = (int)__popcll(__ballot(mine && inter));
    c[2] = (int)__popcll(__ballot(mine && v_e));
    c[3] = (int)__popcll(__ballot(mine && v_g));
#pragma unroll
    for (int k = 0; k < PE_MAX_T; ++k) c[4 + k] = k < T ? (int)__popcll(__ballot(mine && inter && err >= taus.v[k])) : 0;
    if (lane != lead) return;
#pragma unroll
    for (int k = 0; k < 4 + PE_MAX_T; ++k) {
      if (k >= C || !c[k]) continue;
      if (pn == nb) atomicAdd(&wg_of_nb[k], c[k]);
      else vf_add(counts + (size_t)pn * C + k, c[k]);
    }
  });
  __syncthreads();
  if (threadIdx.x < C && wg[threadIdx.x]) vf_add(counts + (size_t)nb * C + threadIdx.x, wg[threadIdx.x]);
}

extern "C" size_t sam6d_pose_vsd_workspace_bytes(long total, int N) {
  if (N < 1 || N > PE_MAX_PAIRS || total < 0 || total > 2L * N * RS_MAX_HW * RS_MAX_HW) return 0;
  return (size_t)total * sizeof(unsigned long long) + (size_t)N * 2 * 8 * sizeof(int);
}

extern "C" int sam6d_pose_vsd(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy, float cx,
                              float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset, long total,
                              const float* depth_obs, float delta, const float* taus, int T, float inv_norm, int* counts, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int bad = rs_limits("pose_vsd", V, F, "N", N, PE_MAX_PAIRS, H, W, near);
  if (bad) return bad;
  if (const int bad_tol = pe_check_vsd("pose_vsd", wave_area, delta, inv_norm, fx, fy, T)) return bad_tol;
  SAM6D_REQUIRE(total >= 0 && total <= 2L * N * H * W, "pose_vsd: total = %ld is not in 0 .. 2 N H W = %ld", total, 2L * N * H * W);
  SAM6D_POINTER("pose_vsd", vertices);
  SAM6D_POINTER("pose_vsd", faces);
  SAM6D_POINTER("pose_vsd", view);
  SAM6D_POINTER("pose_vsd", box);
  SAM6D_POINTER("pose_vsd", offset);
  SAM6D_POINTER("pose_vsd", depth_obs);
  SAM6D_POINTER("pose_vsd", taus);
  SAM6D_POINTER("pose_vsd", counts);
  SAM6D_POINTER("pose_vsd", workspace);
  PeTaus tv;
  if (const int bad_tau = pe_check_taus("pose_vsd", taus, T, tv)) return bad_tau;
  const size_t need = sam6d_pose_vsd_workspace_bytes(total, N);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_vsd: workspace of %zu bytes is below sam6d_pose_vsd_workspace_bytes = %zu", workspace_bytes,
                need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "pose_vsd: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  unsigned long long* zbuf = (unsigned long long*)workspace;
  int* dropped = (int*)(zbuf + total);  // the raster pass's dropped-face counter lives in column 7 of (2N,8); nothing reads it
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * (4 + T) * sizeof(int), s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(zbuf, 0xff, (size_t)total * 8, s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(dropped, 0, (size_t)N * 2 * 8 * sizeof(int), s);
  SAM6D_MEMSET_CHECK("pose_vsd", e);
  if (total == 0) return 0;
  hipLaunchKernelGGL(verify_faces_kernel, dim3((F + 63) / 64, 2 * N), dim3(64), 0, s, vertices, V, faces, F, view, cam,
                     wave_area ? wave_area : RS_WAVE_AREA, box, offset, (long long)total, zbuf, dropped);
  SAM6D_LAUNCH_CHECK_CONT("pose_vsd (faces)");
  // total <= 2^32: at most 2^22 blocks
  const PeCam pc = {fx, fy, cx, cy};
  hipLaunchKernelGGL(vsd_compare_kernel, dim3((unsigned)((total + PE_VSD_WG - 1) / PE_VSD_WG)), dim3(PE_VSD_WG), 0, s, zbuf, (long long)total, box, offset, N, H,
                     W, depth_obs, pc, delta, tv, T, inv_norm, counts);
  SAM6D_LAUNCH_CHECK("pose_vsd (compare)");
}
