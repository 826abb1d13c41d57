// Refining poses against the depth image the scene was measured with: projective point-to-plane Gauss-Newton steps, batched over N
// poses.  Each pose is rendered into a window of its own (verify.hip's raster pass: verify_raster.h), every rendered pixel
// with an observed depth near the rendered one is a pair, the pairs' normal equations are summed as integers, and one thread per pose
// solves them and moves the pose.  The reference has no refinement: its poses leave the weighted SVD of 2048 sampled points as they are
// (PEM/run_inference_custom_pytorch.py:460-471).  The method, its gates and its status codes are the package's own, as the check of
// verify.hip is.  Restated in numpy in tests/refine_ref.py; every comparison is bit for bit.
//
// RECIPE.  One call of sam6d_pose_refine_step is one iteration.  The state of pose n is twelve float64: R row-major, then t.  Per-pixel
// arithmetic is IEEE fp32 in the order written (the library is built with -ffp-contract=off and this file has no fused multiply-add),
// the sums are integers, the solve is float64 with + - * / and sqrt only, in the order written.
//
//  a. window  box[n] and offset[n] are the caller's and stay what they are for every iteration (sam6d_hip.refine grows
//             sam6d_pose_windows' box of the initial pose by a margin); the window is verify.hip's: the box clamped to the image.
//             What moves out of the window is not seen.
//  b. raster  view[n] = [fl32(R * scale) | fl32(t)] (the float64 product, rounded once; with R and scale float32 values that is the
//             float32 product of verify.pose_views).  verify_faces_kernel rasters it into the window's words: sam6d_pose_verify's keys.
//  c. pairs   per window word that is not empty: r = the float of the key's upper half, f = its lower half, o = depth[y][x].  A pair
//             when o > 0, |o - r| <= gate and, with masks, masks[n][y][x] != 0, and when none of the tests below drops it.
//     ray     rx = (((float)x + 0.5) - cx) / fx, ry = (((float)y + 0.5) - cy) / fy, 1: raster.hip's pixel centre.
//     points  q = (rx o, ry o, o) observed, p = (rx r, ry r, r) rendered.
//     normal  P0 P1 P2 = the face's stored vertices through view[n] (rs_to_camera); a = P1 - P0, b = P2 - P0; m = a x b with
//             m0 = a1 b2 - a2 b1, m1 = a2 b0 - a0 b2, m2 = a0 b1 - a1 b0 (rs_face_normal: the resolve kernels' flat normal);
//             l = sqrt((m0 m0 + m1 m1) + m2 m2), dropped unless l > 0;
//             nrm = m / l, negated when (nrm0 p0 + nrm1 p1) + nrm2 p2 > 0: towards the camera.
//     e       ((nrm0 d0 + nrm1 d1) + nrm2 d2) * inv_unit with d = q - p.
//     c       (q - t) * inv_unit per component, t the view's fourth column; dropped unless (c0 c0 + c1 c1) + c2 c2 <= 16^2 and
//             |e| <= 16 (NaN drops).
//     J       (c x nrm, nrm) with the cross product in the order of m.
//  d. sums    u = (J0 .. J5, e).  For i <= j, row-major over the upper triangle of the 7 x 7 matrix (28 products, word k): the product
//             (double)u_i * (double)u_j is exact, times 2^30 exact, rint() to the nearest even integer, added to acc[n][k] as a 64-bit
//             integer.  So words 0 .. 27 hold J_i J_j, J_i e (column 6) and e e (word 27); word 28 the number of pairs; 29 .. 31 stay 0.
//  e. solve   A_ij = (double)acc * 2^-30, g_i = (double)acc(i,6) * 2^-30; A_ii = A_ii + damping * A_ii.  Cholesky A = L L^T, column by
//             column: s = A_jj - L_j0 L_j0 - ... (subtracted one by one, ascending k); singular unless s > 0; L_jj = sqrt(s);
//             L_ij = (A_ij - L_i0 L_j0 - ...) / L_jj.  y_i = (g_i - L_i0 y_0 - ...) / L_ii; x_i = (y_i - L_{i+1,i} x_{i+1} - ...) / L_ii
//             from i = 5 down, k ascending.  omega = x_0..2, v = x_3..5; refused unless
//             ((((x0 x0 + x1 x1) + x2 x2) + x3 x3) + x4 x4) + x5 x5 <= max_step^2.
//     update  w = omega * 0.5; s = (w0 w0 + w1 w1) + w2 w2; k = 2 / (1 + s); C_ij = delta_ij + k * ([w]x_ij + (w_i w_j - delta_ij s))
//             (the Cayley map I + 2 / (1 + |w|^2) ([w]x + [w]x^2): a rotation by 2 atan|w| about w, no sin or cos);
//             R_ij <- (C_i0 R_0j + C_i1 R_1j) + C_i2 R_2j; t_i <- t_i + v_i * unit, unit = 1 / (double)inv_unit.
//     status  0 stepped; 4 the window is empty; 1 fewer than min_pairs pairs; 2 a pivot is not positive; 3 the step is refused (also a
//             NaN).  The first that holds, in the order 4 1 2 3; with any but 0 the state is not written.
//     stats   (N,4) i32: pairs, status, the low and the high 32 bits of acc[n][27] (sum e e, in units of 2^-30 inv_unit^-2).
//
// WHERE J COMES FROM.  A point p of the model's surface with normal nrm sees the observed point q at signed distance e = nrm . (q - p).
// Moving the model by xi = (omega, v) about the centre t takes p to p' = p + omega x (p - t) + v (first order), so the distance
// becomes nrm . (q - p') = e - nrm . (omega x (p - t)) - nrm . v = e - omega . ((p - t) x nrm) - nrm . v.  With q - t in place of
// p - t the difference is omega . ((q - p) x nrm): the product of the step and the residual's tangential part, second order, and zero
// at the solution; the turning of nrm itself, (omega x nrm) . (q - p), is second order in the same way.  So the residual is e - J xi
// with J = [(q - t) x nrm, nrm], Gauss-Newton minimises sum (e - J xi)^2: (sum J^T J) xi = sum J^T e, and the model moves by
// R <- C(omega) R, t <- t + v.  Lengths are divided by `unit` first (the caller passes the model's radius in the unit of t), so J and e
// are O(1) and omega, in radians, and v, in radii, weigh alike in the step bound and the damping.
//
// WHY THE SUMS CANNOT OVERFLOW.  |c| <= 16 and |nrm| <= 1 up to fp32 rounding, so |J_i| <= 16 (1 + 2^-20), |e| <= 16, and every
// product is below 257 < 2^9.  A window has at most 2048 * 2048 = 2^22 pixels.  |sum| < 2^22 * 2^9 * 2^30 = 2^61 < 2^63.  Each term
// is rounded by at most 2^-31, so a sum over P pairs differs from the exact one by at most P * 2^-31.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  As verify.hip: the z-buffer words meet in 64-bit atomic minima, the sums in
// 64-bit integer atomic adds at agent scope, both commutative and associative; memsets precede the kernels in stream order, nothing
// reads a buffer in the launch that reduces into it, and state and stats have one writer, refine_solve_kernel's thread of the pose.
//
// WORK.  refine_view: one thread per matrix element.  raster: verify_faces_kernel, its thread path and wave path.  accumulate: one
// thread per window word of all poses, sixteen waves to a workgroup, the grid sized by the sum of the windows, the pose and pixel
// found by the code classify finds them with (verify_raster.h: vf_first_pose, vf_word, and vf_each_pose for the poses present in a
// wave).  The 29 sums are reduced inside the wave (shuffles), then in LDS for the pose of the workgroup's first word, and
// leave as one atomic per sum and workgroup -- verify.hip's WORK paragraph has what one atomic per wave cost there.  A wave without a
// pair reduces nothing.  solve: one thread per pose.
//
// WHAT THE HOST CANNOT SEE.  box and offset are on the device: the kernels guard themselves as verify.hip's do, a face index at or
// beyond F or a vertex index outside [0, V) drops the pixel, and acc, state and stats are addressed by the pose index alone.
#include "verify_raster.h"
#include "../../include/sam6d_hip.h"

#define RF_WG 1024
#define RF_SUMS 29          // 28 products and the pair count
#define RF_WORDS 32         // words of a pose's accumulator
#define RF_SCALE 1073741824.0        // 2^30
#define RF_INV_SCALE (1.0 / 1073741824.0)
#define RF_BOUND 16.0f

// ---------------------------------------------------------------------------------------------------------- b. view
__global__ __launch_bounds__(256) void refine_view_kernel(const double* __restrict__ state, int N, float scale, float* __restrict__ view) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * 12) return;
  const int n = i / 12, r = (i % 12) / 4, c = i % 4;
  const double* s = state + (size_t)n * 12;
  view[i] = c < 3 ? (float)(s[r * 3 + c] * (double)scale) : (float)s[9 + r];
}

// ---------------------------------------------------------------------------------------------------------- c. pairs
// u = (J0 .. J5, e) of the window pixel (y, x); false when the pixel is dropped
__device__ __forceinline__ bool rf_pair(const float* __restrict__ vert, int V, const int* __restrict__ faces, int F, unsigned face,
                                        const float* __restrict__ M, const RsCam& cam, int x, int y, float r, float o, float inv_unit,
                                        float (&u)[7]) {
  if (face >= (unsigned)F) return false;
  float P[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int id = faces[(size_t)face * 3 + k];
    if ((unsigned)id >= (unsigned)V) return false;
    rs_to_camera(M, vert + (size_t)id * 3, P[k]);
  }
  const float rx = (((float)x + 0.5f) - cam.cx) / cam.fx, ry = (((float)y + 0.5f) - cam.cy) / cam.fy;
  const float q0 = rx * o, q1 = ry * o, q2 = o;
  const float p0 = rx * r, p1 = ry * r, p2 = r;
  float m[3];
  rs_face_normal(P, m);
  const float l = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  if (!(l > 0.f)) return false;
  float n0 = m[0] / l, n1 = m[1] / l, n2 = m[2] / l;
  if ((n0 * p0 + n1 * p1) + n2 * p2 > 0.f) {
    n0 = -n0;
    n1 = -n1;
    n2 = -n2;
  }
  const float d0 = q0 - p0, d1 = q1 - p1, d2 = q2 - p2;
  const float e = ((n0 * d0 + n1 * d1) + n2 * d2) * inv_unit;
  const float c0 = (q0 - M[3]) * inv_unit, c1 = (q1 - M[7]) * inv_unit, c2 = (q2 - M[11]) * inv_unit;
  if (!((c0 * c0 + c1 * c1) + c2 * c2 <= RF_BOUND * RF_BOUND) || !(fabsf(e) <= RF_BOUND)) return false;
  u[0] = c1 * n2 - c2 * n1;
  u[1] = c2 * n0 - c0 * n2;
  u[2] = c0 * n1 - c1 * n0;
  u[3] = n0;
  u[4] = n1;
  u[5] = n2;
  u[6] = e;
  return true;
}

// ---------------------------------------------------------------------------------------------------------- d. sums
__device__ __forceinline__ void rf_put(long long v, int k, bool local, unsigned long long* wg, unsigned long long* __restrict__ acc) {
  if (v == 0) return;
  if (local) atomicAdd(wg + k, (unsigned long long)v);
  else __hip_atomic_fetch_add(acc + k, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per window word of all poses, sixteen waves in a workgroup: the sums of the pose of the workgroup's first word are
// gathered in LDS and leave as one atomic per sum and workgroup; a wave's sums for another pose (a window that begins inside the
// workgroup) leave as one atomic per sum and wave
__global__ __launch_bounds__(RF_WG) void refine_accumulate_kernel(const unsigned long long* __restrict__ zbuf, long long total,
                                                                  const int* __restrict__ box, const long long* __restrict__ offset, int N,
                                                                  const float* __restrict__ vert, int V, const int* __restrict__ faces, int F,
                                                                  const float* __restrict__ view, RsCam cam,
                                                                  const float* __restrict__ depth_obs, const unsigned char* __restrict__ masks,
                                                                  float gate, float inv_unit, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long wg[RF_SUMS];
  const int H = cam.H, W = cam.W;
  const long long base = (long long)blockIdx.x * RF_WG, i = base + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < RF_SUMS) wg[threadIdx.x] = 0;
  const int nb = vf_first_pose(offset, N, base);
  bool pair = false;
  float u[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  VfPixel px;
  if (vf_word(zbuf, total, box, offset, N, H, W, i, nb, px)) {
    const float r = px.r(), o = depth_obs[px.p];
    pair = o > 0.f && fabsf(o - r) <= gate;
    if (pair && masks) pair = masks[(size_t)px.n * H * W + px.p] != 0;
    if (pair) pair = rf_pair(vert, V, faces, F, px.face(), view + (size_t)px.n * 12, cam, px.x, px.y, r, o, inv_unit, u);
  }
  __syncthreads();  // wg is zero
  unsigned long long* const wg_of_nb = wg;
  vf_each_pose(pair, px.n, [=](int lead, int pn, bool mine, unsigned long long m) {
    const bool local = pn == nb;
    unsigned long long* dst = acc + (size_t)pn * RF_WORDS;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = a; b < 7; ++b) {
        const long long term = mine ? (long long)rint((double)u[a] * (double)u[b] * RF_SCALE) : 0ll;
        const long long sum = wave_sum(term);
        if (lane == lead) rf_put(sum, k, local, wg_of_nb, dst);
        ++k;
      }
    if (lane == lead) rf_put((long long)__popcll(m), 28, local, wg_of_nb, dst);
  });
  __syncthreads();
  if (threadIdx.x < RF_SUMS && wg[threadIdx.x])
    __hip_atomic_fetch_add(acc + (size_t)nb * RF_WORDS + threadIdx.x, wg[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------- e. solve
// word k of the product (i, j), i <= j, row-major over the upper triangle of the 7 x 7 matrix
__device__ __forceinline__ constexpr int rf_word(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }

// one thread per pose: the only writer of state[n] and stats[n]
__global__ __launch_bounds__(64) void refine_solve_kernel(const long long* __restrict__ acc, const int* __restrict__ box,
                                                          const long long* __restrict__ offset, int N, int H, int W, double damping,
                                                          int min_pairs, double max_step, float inv_unit, double* __restrict__ state,
                                                          int* __restrict__ stats) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const long long* a = acc + (size_t)n * RF_WORDS;
  const long long pairs = a[28], see = a[27];
  int* st = stats + (size_t)n * 4;
  st[0] = (int)pairs;
  st[2] = (int)(unsigned)((unsigned long long)see & 0xffffffffull);
  st[3] = (int)(unsigned)((unsigned long long)see >> 32);
  const VfWin w = vf_window(box, offset, n, H, W);
  if (w.bw == 0) {
    st[1] = 4;
    return;
  }
  if (pairs < (long long)min_pairs) {
    st[1] = 1;
    return;
  }
  double L[6][6], g[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) L[i][j] = (double)a[rf_word(j, i)] * RF_INV_SCALE;  // A, lower triangle
    g[i] = (double)a[rf_word(i, 6)] * RF_INV_SCALE;
    L[i][i] = L[i][i] + damping * L[i][i];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) ok = false;
    const double d = sqrt(s);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  if (!ok) {
    st[1] = 2;
    return;
  }
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t = t - L[i][k] * x[k];
    x[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t = t - L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
  const double step2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
  if (!(step2 <= max_step * max_step)) {
    st[1] = 3;
    return;
  }
  const double w0 = x[0] * 0.5, w1 = x[1] * 0.5, w2 = x[2] * 0.5;
  const double s = (w0 * w0 + w1 * w1) + w2 * w2;
  const double k = 2.0 / (1.0 + s);
  const double wv[3] = {w0, w1, w2};
  const double X[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  double C[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double sq = i == j ? wv[i] * wv[j] - s : wv[i] * wv[j];
      C[i][j] = (i == j ? 1.0 : 0.0) + k * (X[i][j] + sq);
    }
  double* sp = state + (size_t)n * 12;
  double R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = sp[i];
  const double unit = 1.0 / (double)inv_unit;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) sp[i * 3 + j] = (C[i][0] * R[j] + C[i][1] * R[3 + j]) + C[i][2] * R[6 + j];
    sp[9 + i] = sp[9 + i] + x[3 + i] * unit;
  }
  st[1] = 0;
}

// ---------------------------------------------------------------------------------------------------------- the entries
extern "C" size_t sam6d_pose_refine_workspace_bytes(long total, int N) {
  if (N < 1 || N > VF_MAX_N || total < 0 || total > (long)N * RS_MAX_HW * RS_MAX_HW) return 0;
  return (size_t)total * sizeof(unsigned long long) + (size_t)N * (12 * sizeof(float) + 8 * sizeof(int));
}

extern "C" int sam6d_pose_refine_step(const float* vertices, int V, const int* faces, int F, float scale, int N, float fx, float fy,
                                      float cx, float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset,
                                      long total, const float* depth_obs, const unsigned char* masks, float gate, float inv_unit,
                                      double damping, int min_pairs, double max_step, double* state, long long* acc, int* stats,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const int bad = vf_check("pose_refine_step", V, F, N, H, W, near);
  if (bad) return bad;
  SAM6D_REQUIRE(wave_area >= 0, "pose_refine_step: wave_area = %d is negative", wave_area);
  SAM6D_REQUIRE(gate >= 0.f && gate <= 3.4028234e38f, "pose_refine_step: gate = %g is not a finite number >= 0", (double)gate);
  SAM6D_REQUIRE(inv_unit > 0.f && inv_unit <= 3.4028234e38f, "pose_refine_step: inv_unit = %g is not a finite number > 0", (double)inv_unit);
  SAM6D_REQUIRE(fabsf(scale) > 0.f && fabsf(scale) <= 3.4028234e38f, "pose_refine_step: scale = %g is not a finite number != 0", (double)scale);
  SAM6D_REQUIRE(damping >= 0.0 && damping <= 1.7976931348623157e308, "pose_refine_step: damping = %g is not a finite number >= 0", damping);
  SAM6D_REQUIRE(min_pairs >= 1, "pose_refine_step: min_pairs = %d is not positive", min_pairs);
  SAM6D_REQUIRE(max_step > 0.0, "pose_refine_step: max_step = %g is not a number > 0", max_step);
  SAM6D_REQUIRE(fx != 0.f && fy != 0.f && fx == fx && fy == fy, "pose_refine_step: fx, fy = %g, %g: zero or not a number", (double)fx, (double)fy);
  SAM6D_REQUIRE(total >= 0 && total <= (long)N * H * W, "pose_refine_step: total = %ld is not in 0 .. N H W = %ld", total, (long)N * H * W);
  SAM6D_REQUIRE(vertices && faces && box && offset && depth_obs && state && acc && stats && workspace, "pose_refine_step: null pointer");
  const size_t need = sam6d_pose_refine_workspace_bytes(total, N);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_refine_step: workspace of %zu bytes is below sam6d_pose_refine_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)acc & 7) == 0,
                "pose_refine_step: workspace, state or acc is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RsCam cam = {fx, fy, cx, cy, near, H, W};
  unsigned long long* zbuf = (unsigned long long*)workspace;
  float* view = (float*)(zbuf + total);
  int* counts = (int*)(view + (size_t)N * 12);  // the raster pass's dropped-face counter lives in column 7; nothing reads it
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)N * RF_WORDS * sizeof(long long), s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(zbuf, 0xff, (size_t)total * 8, s);
  if (e == hipSuccess && total > 0) e = hipMemsetAsync(counts, 0, (size_t)N * 8 * sizeof(int), s);
  if (e != hipSuccess) {
    sam6d_set_error("pose_refine_step: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (total > 0) {
    hipLaunchKernelGGL(refine_view_kernel, dim3((N * 12 + 255) / 256), dim3(256), 0, s, state, N, scale, view);
    SAM6D_LAUNCH_CHECK_CONT("pose_refine_step (view)");
    hipLaunchKernelGGL(verify_faces_kernel, dim3((F + 63) / 64, N), dim3(64), 0, s, vertices, V, faces, F, view, cam,
                       wave_area ? wave_area : RS_WAVE_AREA, box, offset, (long long)total, zbuf, counts);
    SAM6D_LAUNCH_CHECK_CONT("pose_refine_step (faces)");
    // total <= 2^32: at most 2^22 blocks
    hipLaunchKernelGGL(refine_accumulate_kernel, dim3((unsigned)((total + RF_WG - 1) / RF_WG)), dim3(RF_WG), 0, s, zbuf, (long long)total, box,
                       offset, N, vertices, V, faces, F, view, cam, depth_obs, masks, gate, inv_unit, (unsigned long long*)acc);
    SAM6D_LAUNCH_CHECK_CONT("pose_refine_step (accumulate)");
  }
  hipLaunchKernelGGL(refine_solve_kernel, dim3((N + 63) / 64), dim3(64), 0, s, acc, box, offset, N, H, W, damping, min_pairs, max_step, inv_unit,
                     state, stats);
  SAM6D_LAUNCH_CHECK("pose_refine_step (solve)");
}
