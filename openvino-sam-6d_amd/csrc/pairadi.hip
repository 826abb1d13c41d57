// ADD-S / ADI of every pose a[i] against every pose b[j] of one object (sam6d_pose_pair_adi), the matrix that matching and pose NMS
// consume (posematch.hip RECIPE b, c), with the pairs that are certainly above a cap left out before their V x V search starts.  The
// reference has no evaluation code: it writes its poses (PEM/run_inference_custom_pytorch.py:460-471) and leaves the scoring to
// bop_toolkit.  The definition is nearest.hip's RECIPE a, and the code that computes it is nearest.hip's: the point transform, d2,
// the term, the boxes, the skip rule and the walk are the one copy in nearest_walk.h and poseerr_point.h.  Restated in
// tests/pair_adi_ref.py over tests/nearest_ref.py; every comparison with the restatement is bit for bit.  Nothing is pinned against
// bop_toolkit, which the suite does not have.  ADI is evaluated over the vertices.
//
// RECIPE.  Arithmetic as in nearest.hip: IEEE fp32 in the order written, float64 where named, integers elsewhere.
//   computed   adi_sum[i][j] = nearest.hip's RECIPE a with E = a[i], G = b[j]: bit for bit what sam6d_pose_adi gives for that pair.
//   boxes      of the tiles of 256 consecutive points under b[j], as nearest.hip's THE SKIPPING builds them (nn_boxes_kernel).
//   lb_i       for the point e_i = a[i] x_i: the minimum over ALL tiles t of b[j] of the lower bound of THE SKIPPING
//              (nn_lower_bound: gap_k, then (gx gx + gy gy) + gz gz).  The minimum starts at +inf and is taken with fminf.
//   lower_sum  lower_sum[i][j] = sum_i rint(w(lb_i)), w RECIPE a's term with its cap at 2^42 (pe_add_term): a 64-bit integer sum.
//   skipped    iff cap_sum >= 0 and lower_sum[i][j] > cap_sum.  Then adi_sum[i][j] = -1 and the V x V walk of the pair is never
//              started.  cap_sum < 0: no cap, nothing is skipped, lower_sum is not formed.
//
// WHY THE SKIP IS EXACT.  For a tile t of b[j] and every j of it whose d2_ij is a number, lb_t <= d2_ij holds IN FP32 without a
// margin: that is THE SKIPPING of nearest.hip (rounding to nearest is monotone in each operand and lo_k <= g_jk <= hi_k).  A d2 that
// is not a number never becomes m_i.  So lb_i = min_t lb_t <= m_i wherever m_i is some d2_ij, and where no d2 of the point is a
// number m_i = +inf >= lb_i anyway.  lb is never a NaN: the gap of a NaN coordinate is 0 (fmaxf drops the NaN differences), the gap
// against an empty box is +inf, squares and sums of values in [0, +inf] stay there, and fminf of such values does too.  sqrtf, the
// widening to float64, the product with inv_unit > 0, the product with 2^30, the cap at 2^42 and rint are all monotone (non-decreasing)
// on [0, +inf], so rint(w(lb_i)) <= rint(w(m_i)) term by term and lower_sum <= adi_sum as integers (both below 2^63: at most 2^20
// terms of at most 2^42).  A skipped pair therefore has adi_sum >= lower_sum > cap_sum: its ADI is above the cap, which is all a
// consumer that compares with a threshold at or below the cap needs to know.  The decision depends on lower_sum and cap_sum alone,
// both functions of the inputs, so which pairs are computed does not depend on timing, on flags or on the order of the workgroups.
// A coarser bound (the union box of a pose) would decide a subset of these pairs; it is not used, lower_sum is an output.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  As in nearest.hip: workgroups meet in 64-bit integer atomic adds at agent
// scope (lower_sum, adi_sum), the buffers are set by memsets that precede the kernels in stream order, and nothing reads a buffer
// in the launch that reduces into it: the boxes are written by nn_boxes_kernel, lower_sum is reduced into by pair_adi_bound_kernel
// and read by pair_adi_walk_kernel, which reduces into adi_sum, and pair_adi_finish_kernel, one thread per pair, reads lower_sum and
// is the only writer of `skipped` and of the -1 of a skipped pair (whose adi_sum no walk touched).
//
// WORK.  The boxes once per pose b[j] (T x B workgroups), where the pair-by-pair entry builds them once per pair.  Bound launch over
// (pair, chunk): a workgroup holds 1024 points of a[i] in registers as nn_adi_chunk does and streams the (T,6) boxes of b[j]
// through LDS 256 at a time, read as broadcasts: V T box tests per pair, 1/256 of the full walk's distance count.  Walk launch over
// (pair, chunk): returns at once for a skipped pair (the first thing it reads), else nn_adi_chunk.  The pair is blockIdx.x, so
// the launch shape allows A B up to 2^20 and V / 1024 chunks up to 1024 in blockIdx.y; A B ceil(V / 1024) is capped at 2^22
// workgroups a launch (PA_MAX_WGS) and refused by name above it.
#include "nearest_walk.h"
#include "../../include/sam6d_hip.h"

#define PA_MAX_POSES 1024
#define PA_MAX_WGS (1 << 22)  // A B ceil(V / 1024)

// grid (A B, ceil(V / 1024)), four waves: chunk blockIdx.y of the pair blockIdx.x = i B + j.  lower_sum (A,B) arrives zeroed
__global__ __launch_bounds__(NN_WG) void pair_adi_bound_kernel(const float* __restrict__ points, int V, const float* __restrict__ a,
                                                               const float* __restrict__ b, int B, int T, const float* __restrict__ box,
                                                               float inv_unit, unsigned long long* __restrict__ lower_sum) {
  __shared__ float bx[NN_WG * 6];
  const int p = blockIdx.x, i = p / B, j = p - i * B, tid = threadIdx.x;
  float e[NN_PTS][3], lb[NN_PTS];
  bool live[NN_PTS];
#pragma unroll
  for (int q = 0; q < NN_PTS; ++q) {
    const int idx = blockIdx.y * NN_CHUNK + q * NN_WG + tid;  // below 2^20 + 1024
    live[q] = idx < V;
    nn_point(points, V, idx, a + (size_t)i * 12, e[q]);
    lb[q] = INFINITY;
  }
  const float* __restrict__ bj = box + (size_t)j * T * 6;
  for (int base = 0; base < T; base += NN_WG) {
    const int cnt = min(NN_WG, T - base);
    __syncthreads();  // closes the reads of the boxes before
    for (int w = tid; w < cnt * 6; w += NN_WG) bx[w] = bj[(size_t)base * 6 + w];
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
      float lo[3], hi[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        lo[k] = bx[t * 6 + k];
        hi[k] = bx[t * 6 + 3 + k];
      }
#pragma unroll
      for (int q = 0; q < NN_PTS; ++q) lb[q] = fminf(lb[q], nn_lower_bound(e[q], lo, hi));
    }
  }
  long long term = 0;
#pragma unroll
  for (int q = 0; q < NN_PTS; ++q)
    if (live[q]) term += pe_add_term(lb[q], inv_unit);
  term = wave_sum(term);
  if ((tid & 63) == 0 && term) __hip_atomic_fetch_add(lower_sum + p, (unsigned long long)term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (A B, ceil(V / 1024)), four waves.  lower_sum is the earlier launch's, read only (null: no cap); adi_sum (A,B) arrives zeroed
__global__ __launch_bounds__(NN_WG) void pair_adi_walk_kernel(const float* __restrict__ points, int V, const float* __restrict__ a,
                                                              const float* __restrict__ b, int B, int T, const float* __restrict__ box,
                                                              float inv_unit, int flags, const long long* __restrict__ lower_sum,
                                                              long long cap_sum, unsigned long long* __restrict__ adi_sum) {
  const int p = blockIdx.x, i = p / B, j = p - i * B;
  if (lower_sum && lower_sum[p] > cap_sum) return;  // (uniform) RECIPE skipped: before the first barrier
  nn_adi_chunk(points, V, blockIdx.y, a + (size_t)i * 12, b + (size_t)j * 12, T, box + (size_t)j * T * 6, inv_unit, flags, adi_sum + p);
}

// grid (ceil(A B / 256)): one thread per pair, the only writer of `skipped` and of a skipped pair's adi_sum
__global__ __launch_bounds__(NN_WG) void pair_adi_finish_kernel(int P, const long long* __restrict__ lower_sum, long long cap_sum,
                                                                long long* __restrict__ adi_sum, unsigned char* __restrict__ skipped) {
  const int p = blockIdx.x * NN_WG + threadIdx.x;
  if (p >= P) return;
  const bool skip = lower_sum && lower_sum[p] > cap_sum;
  skipped[p] = skip ? 1 : 0;
  if (skip) adi_sum[p] = -1;
}

extern "C" size_t sam6d_pose_pair_adi_workspace_bytes(int V, int A, int B) {
  if (V < 1 || V > NN_MAX_V || A < 1 || A > PA_MAX_POSES || B < 1 || B > PA_MAX_POSES) return 0;
  if ((long long)A * B * ((V + NN_CHUNK - 1) / NN_CHUNK) > PA_MAX_WGS) return 0;
  return (size_t)B * ((V + NN_TILE - 1) / NN_TILE) * 6 * sizeof(float);
}

extern "C" int sam6d_pose_pair_adi(const float* points, int V, const float* a, int A, const float* b, int B, float inv_unit, int flags,
                                   long cap_sum, long long* adi_sum, long long* lower_sum, unsigned char* skipped, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(V >= 1 && V <= NN_MAX_V, "pose_pair_adi: V = %d is not in 1 .. %d", V, NN_MAX_V);
  SAM6D_REQUIRE(A >= 1 && A <= PA_MAX_POSES, "pose_pair_adi: A = %d is not in 1 .. %d", A, PA_MAX_POSES);
  SAM6D_REQUIRE(B >= 1 && B <= PA_MAX_POSES, "pose_pair_adi: B = %d is not in 1 .. %d", B, PA_MAX_POSES);
  const int chunks = (V + NN_CHUNK - 1) / NN_CHUNK, P = A * B;
  SAM6D_REQUIRE((long long)P * chunks <= PA_MAX_WGS, "pose_pair_adi: A B ceil(V / 1024) = %d x %d x %d is above the cap of %d workgroups a launch", A,
                B, chunks, PA_MAX_WGS);
  if (const int bad = pe_check_inv_unit("pose_pair_adi", inv_unit)) return bad;
  SAM6D_REQUIRE((flags & ~NN_NO_PRUNE) == 0, "pose_pair_adi: flags = %d has bits beyond bit 0", flags);
  SAM6D_POINTER("pose_pair_adi", points);
  SAM6D_POINTER("pose_pair_adi", a);
  SAM6D_POINTER("pose_pair_adi", b);
  SAM6D_POINTER("pose_pair_adi", adi_sum);
  SAM6D_POINTER("pose_pair_adi", skipped);
  SAM6D_POINTER("pose_pair_adi", workspace);
  const bool cap = cap_sum >= 0;
  SAM6D_REQUIRE(!cap || lower_sum != nullptr, "pose_pair_adi: lower_sum is a null pointer and cap_sum = %ld asks for it", cap_sum);
  const size_t need = sam6d_pose_pair_adi_workspace_bytes(V, A, B);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_pair_adi: workspace of %zu bytes is below sam6d_pose_pair_adi_workspace_bytes = %zu", workspace_bytes,
                need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)adi_sum & 7) == 0 && (!cap || ((uintptr_t)lower_sum & 7) == 0),
                "pose_pair_adi: workspace, adi_sum or lower_sum is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(adi_sum, 0, (size_t)P * sizeof(long long), s);
  if (cap && e == hipSuccess) e = hipMemsetAsync(lower_sum, 0, (size_t)P * sizeof(long long), s);
  SAM6D_MEMSET_CHECK("pose_pair_adi", e);
  const int T = (V + NN_TILE - 1) / NN_TILE;
  float* box = (float*)workspace;
  if (const int bad = nn_boxes("pose_pair_adi", points, V, b, B, box, s)) return bad;
  const long long* lower = cap ? lower_sum : nullptr;
  if (cap) {
    hipLaunchKernelGGL(pair_adi_bound_kernel, dim3(P, chunks), dim3(NN_WG), 0, s, points, V, a, b, B, T, (const float*)box, inv_unit,
                       (unsigned long long*)lower_sum);
    SAM6D_LAUNCH_CHECK_CONT("pose_pair_adi (bound)");
  }
  hipLaunchKernelGGL(pair_adi_walk_kernel, dim3(P, chunks), dim3(NN_WG), 0, s, points, V, a, b, B, T, (const float*)box, inv_unit, flags, lower, (long long)cap_sum,
                     (unsigned long long*)adi_sum);
  SAM6D_LAUNCH_CHECK_CONT("pose_pair_adi (walk)");
  hipLaunchKernelGGL(pair_adi_finish_kernel, dim3((P + NN_WG - 1) / NN_WG), dim3(NN_WG), 0, s, P, lower, (long long)cap_sum, adi_sum, skipped);
  SAM6D_LAUNCH_CHECK("pose_pair_adi (finish)");
}
