// The two pose-scoring quantities that need a search over all pairs of model vertices: ADD-S / ADI (Hinterstoisser et al. 2012;
// Hodan et al. 2016), batched over N pose pairs, and the model diameter as bop_toolkit defines it, the largest distance between two
// vertices.  The reference has no evaluation code: it writes its poses (PEM/run_inference_custom_pytorch.py:460-471) and leaves the
// scoring to bop_toolkit.  The definitions are the published ones, restated here and pinned against the numpy restatement
// tests/nearest_ref.py -- NOT against bop_toolkit, which the suite does not have.  Both are an exact extremum over V x V of the
// distance recipe of poseerr.hip, made affordable by skipping whole tiles of 256 points whose bound cannot change the extremum.
// Every comparison with the restatement is bit for bit, with and without the skipping.
//
// RECIPE.  All float arithmetic is IEEE fp32 in the order written unless float64 is named (the library is built with
// -ffp-contract=off and this file has no fused multiply-add), everything else is integer.
//
//  a. ADI (sam6d_pose_adi), per pose pair n with E = est[n], G = gt[n] (no symmetries), per model point x_i:
//   points   e_i = E x_i and g_j = G x_j: ((M_r0 x0 + M_r1 x1) + M_r2 x2) + M_r3 (raster.h's rs_to_camera).
//   d2_ij    = (dx dx + dy dy) + dz dz with d = e_i - g_j.
//   m_i      starts at +inf and is replaced by d2_ij where d2_ij < m_i: a NaN never wins, and the order of the j does not matter.
//   term     w_i = ((double)sqrtf(m_i) * (double)inv_unit) * 2^30, and w_i = 2^42 where w_i <= 2^42 is false (4096 units; also a
//            NaN, also a point none of whose d2 is a number: m_i = +inf).  ADD's term and cap.
//   ADI      adi_sum[n] = sum_i rint(w_i): a 64-bit integer sum, at most 2^20 * 2^42 = 2^62.  The caller forms
//            adi = adi_sum / 2^30 / inv_unit / V.
//
//  b. diameter (sam6d_points_diameter), over the raw fp32 vertices:
//   d2_ij    = (dx dx + dy dy) + dz dz with d = x_i - x_j.  -d is exact, so d2_ji has the bits of d2_ij.
//   maximum  over all pairs, of the words poseerr.hip's maxima use: a value > 0 offers its bits, 0 offers 0, anything else (a NaN)
//            offers 0x7fc00000, above every number.  d2 is a sum of squares, never negative and never -0, so the kernels take the
//            unsigned maximum of the raw bits and fold every word above +inf's into 0x7fc00000 before it leaves the wave (nn_word):
//            the same word.
//   diameter = sqrtf(the maximum as a float).  V = 1 gives 0; a vertex with a coordinate that is not finite gives NaN (x_i - x_i).
//
// THE SKIPPING, AND WHY IT IS EXACT.  Points are taken in tiles of 256 consecutive indices.  A pre-pass (nn_boxes_kernel) writes per
// (pose, tile) the axis-aligned box lo, hi of the tile's ACTUAL fp32 g_j (for the diameter: of its x_j); minima and maxima ignore a
// NaN as fminf and fmaxf do, a tile without a number has lo = +inf, hi = -inf.
//   ADI.  For a point e the gap per axis is gap_k = e_k > hi_k ? e_k - hi_k : (e_k < lo_k ? lo_k - e_k : 0), and the lower bound
//   lb = (gap_x gap_x + gap_y gap_y) + gap_z gap_z, in d2's order.  IEEE round-to-nearest subtraction, multiplication and addition are
//   monotone in each operand, and lo_k <= g_jk <= hi_k for every j of the tile whose g_jk is a number; so |fl(e_k - g_jk)| >= gap_k
//   and hence d2_ij >= lb IN FP32, with no rounding margin.  A tile is skipped for a point when lb > m_i: every d2_ij of the tile is
//   then above m_i or a NaN, and neither replaces m_i.  A comparison with a NaN is false, so nothing is skipped on one.  (The kernel
//   forms gap_k as fmaxf(fmaxf(e_k - hi_k, lo_k - e_k), 0): with lo_k <= hi_k at most one difference is above 0 and it is the one the
//   comparisons select, a NaN difference is dropped as a false comparison is, and the empty box gives +inf either way.)
//   Diameter.  The mirrored upper bound: u_k = max(|x_k - lo_k|, |x_k - hi_k|) (fmaxf) and ub = (u_x u_x + u_y u_y) + u_z u_z.
//   fl(x_k - x_jk) lies between fl(x_k - hi_k) and fl(x_k - lo_k) by the same monotonicity, so d2_ij <= ub.  A tile is skipped for a
//   point when ub <= L, where L is a lower bound of the answer.  Such a pair cannot raise a maximum that is at least L.  A d2 that is
//   a NaN needs a vertex p with a coordinate that is not finite, and then d2_pp is a NaN too: a point with such a coordinate never
//   skips a tile (the tile pair of its own tile is always walked), so the NaN is found whatever the boxes say.
//   L is the word written by an EARLIER launch (the seed launch: the distances from up to 8 seed vertices to all vertices), never the
//   word the same launch reduces into.
//   The decision is taken per workgroup and tile: a tile is walked when any live point of the workgroup cannot skip it.  Walking a
//   tile a point could have skipped does not change that point's extremum either.  flags bit 0 walks every tile.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  Where workgroups meet it is an integer atomic at agent scope: 64-bit adds
// (adi_sum), 32-bit maxima (the d2 words), commutative and associative.  m_i is a minimum and lives in one thread.  The buffers are
// set by memsets that precede the kernels in stream order, and nothing reads a buffer in the launch that reduces into it: the boxes
// are written by nn_boxes_kernel and read by the launch after it, the seed word is reduced into by nn_seed_kernel and read by
// nn_diameter_kernel, which reduces into a second word, and nn_diameter_finish_kernel, the only writer of `diameter`, reads both.
//
// WORK.  ADI: a workgroup of four waves takes 1024 points of one pose, four per thread, and keeps their e and m in registers, as
// pair_errors_kernel (posematch.hip) is laid out.  It walks the tiles beginning with the tiles of its own indices: with a small pose
// error the nearest vertex is the point itself or a neighbour, so m is tight after the first tile and the bounds of the others decide.
// The walk is nn_walk, the one copy of it: per tile one barrier with an OR takes the decision (and closes the reads of the tile
// before); the tile's g_j are formed once per workgroup into LDS and read from there as broadcasts, nine vector instructions per
// pair.  At the end one wave_sum and one atomic per wave.  Diameter: nn_walk over the tile pairs (a, b) with b >= a, the column
// tiles of a row chunk dealt to gridDim.y workgroups so that a small model still fills the chip; one atomic per wave.
// nn_walk, the lower bound and ADI's walk of one chunk live in nearest_walk.h, because pairadi.hip (ADI of every pose against every
// pose, sam6d_pose_pair_adi) runs the same walk per pair of the matrix and the same bound to leave far pairs out.
//
// WHAT THE HOST CANNOT SEE.  The seed indices are on the device: one outside [0, V) is ignored, never dereferenced.
#include "nearest_walk.h"
#include "../../include/sam6d_hip.h"

#define NN_MAX_N 1024
#define NN_MAX_SEEDS 8
#define NN_INF 0x7f800000u
#define NN_DIAM_WGS 2048            // the diameter's main launch aims at this many workgroups

// The constants, the guarded point load (pe_load_point), d2 (pe_d2) and the ADD term (pe_add_term) are poseerr_point.h's; the sizes,
// nn_point, the lower bound, nn_walk and ADI's walk of one chunk (nn_adi_chunk) are nearest_walk.h's, which pairadi.hip shares.
// RECIPE maximum: the word the unsigned maximum of raw d2 bits stands for
__device__ __forceinline__ unsigned nn_word(unsigned raw) { return raw > NN_INF ? PE_NAN : raw; }

// ---------------------------------------------------------------------------------------------------------- the boxes
// grid (T, N), four waves: point blockIdx.x * 256 + tid under gt[blockIdx.y], or the raw point where gt is null (N = 1).
// box (N,T,6) f32 = lo_x lo_y lo_z hi_x hi_y hi_z, every word written
__global__ __launch_bounds__(NN_TILE) void nn_boxes_kernel(const float* __restrict__ points, int V, const float* __restrict__ gt, int T,
                                                           float* __restrict__ box) {
  __shared__ float red[NN_TILE / 64][6];
  const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, idx = t * NN_TILE + tid;
  float g[3], b[6];
  nn_point(points, V, idx, gt ? gt + (size_t)n * 12 : nullptr, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b[k] = idx < V ? fminf(INFINITY, g[k]) : INFINITY;       // a NaN leaves +inf
    b[3 + k] = idx < V ? fmaxf(-INFINITY, g[k]) : -INFINITY;
    b[k] = wave_min(b[k]);
    b[3 + k] = wave_max(b[3 + k]);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[tid >> 6][k] = b[k];
  }
  __syncthreads();
  if (tid < 6) {
    float v = red[0][tid];
#pragma unroll
    for (int w = 1; w < NN_TILE / 64; ++w) v = tid < 3 ? fminf(v, red[w][tid]) : fmaxf(v, red[w][tid]);
    box[((size_t)n * T + t) * 6 + tid] = v;
  }
}

int nn_boxes(const char* who, const float* points, int V, const float* gt, int N, float* box, hipStream_t st) {
  const int T = (V + NN_TILE - 1) / NN_TILE;
  hipLaunchKernelGGL(nn_boxes_kernel, dim3(T, N), dim3(NN_TILE), 0, st, points, V, gt, T, box);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) sam6d_set_error("%s (boxes): launch failed: %s", who, hipGetErrorString(e));
  return (int)e;
}

// ---------------------------------------------------------------------------------------------------------- a. ADI
// grid (ceil(V / 1024), N), four waves: chunk blockIdx.x of pose pair blockIdx.y (nn_adi_chunk).  adi_sum (N) arrives zeroed
__global__ __launch_bounds__(NN_WG) void nn_adi_kernel(const float* __restrict__ points, int V, const float* __restrict__ est,
                                                       const float* __restrict__ gt, int T, const float* __restrict__ box, float inv_unit,
                                                       int flags, unsigned long long* __restrict__ adi_sum) {
  const int n = blockIdx.y;
  nn_adi_chunk(points, V, blockIdx.x, est + (size_t)n * 12, gt + (size_t)n * 12, T, box + (size_t)n * T * 6, inv_unit, flags, adi_sum + n);
}

extern "C" size_t sam6d_pose_adi_workspace_bytes(int V, int N) {
  if (V < 1 || V > NN_MAX_V || N < 1 || N > NN_MAX_N) return 0;
  return (size_t)N * ((V + NN_TILE - 1) / NN_TILE) * 6 * sizeof(float);
}

extern "C" int sam6d_pose_adi(const float* points, int V, const float* est, const float* gt, int N, float inv_unit, int flags,
                              long long* adi_sum, void* workspace, size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(V >= 1 && V <= NN_MAX_V, "pose_adi: V = %d is not in 1 .. %d", V, NN_MAX_V);
  SAM6D_REQUIRE(N >= 1 && N <= NN_MAX_N, "pose_adi: N = %d is not in 1 .. %d", N, NN_MAX_N);
  if (const int bad = pe_check_inv_unit("pose_adi", inv_unit)) return bad;
  SAM6D_REQUIRE((flags & ~NN_NO_PRUNE) == 0, "pose_adi: flags = %d has bits beyond bit 0", flags);
  SAM6D_POINTER("pose_adi", points);
  SAM6D_POINTER("pose_adi", est);
  SAM6D_POINTER("pose_adi", gt);
  SAM6D_POINTER("pose_adi", adi_sum);
  SAM6D_POINTER("pose_adi", workspace);
  const size_t need = sam6d_pose_adi_workspace_bytes(V, N);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_adi: workspace of %zu bytes is below sam6d_pose_adi_workspace_bytes = %zu", workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)adi_sum & 7) == 0, "pose_adi: workspace or adi_sum is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(adi_sum, 0, (size_t)N * sizeof(long long), s);
  SAM6D_MEMSET_CHECK("pose_adi", e);
  const int T = (V + NN_TILE - 1) / NN_TILE;
  float* box = (float*)workspace;
  if (const int bad = nn_boxes("pose_adi", points, V, gt, N, box, s)) return bad;
  hipLaunchKernelGGL(nn_adi_kernel, dim3((V + NN_CHUNK - 1) / NN_CHUNK, N), dim3(NN_WG), 0, s, points, V, est, gt, T, (const float*)box, inv_unit,
                     flags, (unsigned long long*)adi_sum);
  SAM6D_LAUNCH_CHECK("pose_adi (points)");
}

// ---------------------------------------------------------------------------------------------------------- b. diameter
__device__ __forceinline__ void nn_offer(unsigned* word, unsigned raw) {
  const unsigned v = (unsigned)wave_max((int)nn_word(raw));  // at most 0x7fc00000: orders as an int
  if ((threadIdx.x & 63) == 0 && v) __hip_atomic_fetch_max(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(V / 256)), four waves, one point per thread against every seed.  seed_word arrives zeroed
__global__ __launch_bounds__(NN_WG) void nn_seed_kernel(const float* __restrict__ points, int V, const int* __restrict__ seeds, int n_seeds,
                                                        unsigned* __restrict__ seed_word) {
  const int idx = blockIdx.x * NN_WG + threadIdx.x;
  float x[3];
  pe_load_point(points, V, idx, x);
  unsigned raw = 0u;
  for (int k = 0; k < n_seeds; ++k) {
    const int sd = seeds[k];
    if ((unsigned)sd >= (unsigned)V) continue;  // (uniform) ignored, never dereferenced
    const float d2 = pe_d2(x, points[(size_t)sd * 3], points[(size_t)sd * 3 + 1], points[(size_t)sd * 3 + 2]);
    if (idx < V) raw = max(raw, __float_as_uint(d2));
  }
  nn_offer(seed_word, raw);
}

// grid (ceil(V / 1024), Y), four waves: the points of row chunk blockIdx.x against the column tiles 4 blockIdx.x + blockIdx.y,
// + Y, + 2 Y ... below T.  seed_word is the earlier launch's, read only; best arrives zeroed
__global__ __launch_bounds__(NN_WG) void nn_diameter_kernel(const float* __restrict__ points, int V, int T, const float* __restrict__ box,
                                                            const unsigned* __restrict__ seed_word, int flags, unsigned* __restrict__ best) {
  const int tid = threadIdx.x;
  float x[NN_PTS][3];
  bool fin[NN_PTS];
#pragma unroll
  for (int j = 0; j < NN_PTS; ++j) {
    const int idx = blockIdx.x * NN_CHUNK + j * NN_WG + tid;
    pe_load_point(points, V, min(idx, V - 1), x[j]);  // a thread beyond V holds a copy of the last point: a maximum does not count copies
    fin[j] = fabsf(x[j][0]) < INFINITY && fabsf(x[j][1]) < INFINITY && fabsf(x[j][2]) < INFINITY;
  }
  const float L = __uint_as_float(*seed_word);  // a NaN (0x7fc00000) skips nothing
  unsigned raw = 0u;
  const int first = blockIdx.x * NN_PTS + blockIdx.y, Y = gridDim.y;
  nn_walk(
      V, box, flags, [&](int s) { return first + s * Y < T ? first + s * Y : -1; },
      [&](const float(&lo)[3], const float(&hi)[3]) {
        bool all = true;
#pragma unroll
        for (int j = 0; j < NN_PTS; ++j) {
          float u[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) u[k] = fmaxf(fabsf(x[j][k] - lo[k]), fabsf(x[j][k] - hi[k]));
          const float ub = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
          all = all && ub <= L && fin[j];
        }
        return all;
      },
      [&](int idx, float(&c)[3]) { nn_point(points, V, idx, nullptr, c); },
      [&](const float4 c) {
#pragma unroll
        for (int j = 0; j < NN_PTS; ++j) raw = max(raw, __float_as_uint(pe_d2(x[j], c.x, c.y, c.z)));
      });
  nn_offer(best, raw);
}

// one thread: the only writer of `diameter`
__global__ __launch_bounds__(64) void nn_diameter_finish_kernel(const unsigned* __restrict__ words, float* __restrict__ diameter) {
  if (threadIdx.x == 0) *diameter = sqrtf(__uint_as_float(max(words[0], words[1])));
}

extern "C" size_t sam6d_points_diameter_workspace_bytes(int V) {
  if (V < 1 || V > NN_MAX_V) return 0;
  return 8 + (size_t)((V + NN_TILE - 1) / NN_TILE) * 6 * sizeof(float);  // the seed word, the main launch's word, the boxes
}

extern "C" int sam6d_points_diameter(const float* points, int V, const int* seeds, int n_seeds, int flags, float* diameter, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(V >= 1 && V <= NN_MAX_V, "points_diameter: V = %d is not in 1 .. %d", V, NN_MAX_V);
  SAM6D_REQUIRE(n_seeds >= 1 && n_seeds <= NN_MAX_SEEDS, "points_diameter: n_seeds = %d is not in 1 .. %d", n_seeds, NN_MAX_SEEDS);
  SAM6D_REQUIRE((flags & ~NN_NO_PRUNE) == 0, "points_diameter: flags = %d has bits beyond bit 0", flags);
  SAM6D_POINTER("points_diameter", points);
  SAM6D_POINTER("points_diameter", seeds);
  SAM6D_POINTER("points_diameter", diameter);
  SAM6D_POINTER("points_diameter", workspace);
  const size_t need = sam6d_points_diameter_workspace_bytes(V);
  SAM6D_REQUIRE(workspace_bytes >= need, "points_diameter: workspace of %zu bytes is below sam6d_points_diameter_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "points_diameter: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned* words = (unsigned*)workspace;
  float* box = (float*)(words + 2);
  const hipError_t e = hipMemsetAsync(words, 0, 2 * sizeof(unsigned), s);
  SAM6D_MEMSET_CHECK("points_diameter", e);
  const int T = (V + NN_TILE - 1) / NN_TILE, chunks = (V + NN_CHUNK - 1) / NN_CHUNK;
  if (const int bad = nn_boxes("points_diameter", points, V, nullptr, 1, box, s)) return bad;
  hipLaunchKernelGGL(nn_seed_kernel, dim3(T), dim3(NN_WG), 0, s, points, V, seeds, n_seeds, words);
  SAM6D_LAUNCH_CHECK_CONT("points_diameter (seeds)");
  const int want = NN_DIAM_WGS / chunks, Y = want < 1 ? 1 : (want > T ? T : want);
  hipLaunchKernelGGL(nn_diameter_kernel, dim3(chunks, Y), dim3(NN_WG), 0, s, points, V, T, (const float*)box, (const unsigned*)words, flags,
                     words + 1);
  SAM6D_LAUNCH_CHECK_CONT("points_diameter (pairs)");
  hipLaunchKernelGGL(nn_diameter_finish_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)words, diameter);
  SAM6D_LAUNCH_CHECK("points_diameter (finish)");
}
