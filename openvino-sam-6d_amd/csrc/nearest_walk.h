// The pieces of nearest.hip's pruned searches in one copy, for nearest.hip itself (ADI pair by pair, the diameter) and for
// pairadi.hip (ADI of every pose against every pose): the sizes, the point under a pose, the lower bound of THE SKIPPING, the walk
// over the tiles (nn_walk) and ADI's walk of one chunk of points (nn_adi_chunk).  The recipe and the proof that the skipping is
// exact are written out at the top of nearest.hip and nowhere else; every function here names the line of it that it is.
#pragma once
#include "poseerr_point.h"

#define NN_MAX_V (1 << 20)
#define NN_WG 256
#define NN_PTS 4                    // points per thread
#define NN_CHUNK (NN_WG * NN_PTS)   // points per workgroup
#define NN_TILE 256                 // points per box and LDS tile
#define NN_NO_PRUNE 1               // flags bit 0

// the point idx under the (3,4) matrix M, or the raw point where M is null; zeros go in beyond V
__device__ __forceinline__ void nn_point(const float* __restrict__ points, int V, int idx, const float* __restrict__ M, float (&g)[3]) {
  float x[3];
  pe_load_point(points, V, idx, x);
  if (M) {  // (uniform)
    rs_to_camera(M, x, g);
  } else {
    g[0] = x[0];
    g[1] = x[1];
    g[2] = x[2];
  }
}

// THE SKIPPING, ADI: lb of the point e against the box lo, hi; the gap of the header without a branch.  Never a NaN: a NaN
// difference is dropped by fmaxf, so the gap of a NaN coordinate is 0, and the empty box gives +inf
__device__ __forceinline__ float nn_lower_bound(const float (&e)[3], const float (&lo)[3], const float (&hi)[3]) {
  float gap[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gap[k] = fmaxf(fmaxf(e[k] - hi[k], lo[k] - e[k]), 0.f);
  return (gap[0] * gap[0] + gap[1] * gap[1]) + gap[2] * gap[2];
}

// THE SKIPPING's protocol for a workgroup of four waves, in one copy.  tiles(s) is the s-th tile of the workgroup's sequence, below 0
// after the last.  A tile is walked when flags has NN_NO_PRUNE or skips(lo, hi) is false in any thread: whether all of the thread's
// points can do without a tile whose box is lo, hi (box (T,6), read only then).  point(idx, g) is the tile's point idx as it is
// staged, and fold(c) takes one staged point into the thread's points.  Every thread of the workgroup calls it, with the same tiles
template <class Tiles, class Skips, class Point, class Fold>
__device__ __forceinline__ void nn_walk(int V, const float* __restrict__ box, int flags, Tiles tiles, Skips skips, Point point, Fold fold) {
  __shared__ float4 tile[NN_TILE];
  const int tid = threadIdx.x;
  for (int s = 0, t; (t = tiles(s)) >= 0; ++s) {
    bool walk = (flags & NN_NO_PRUNE) != 0;
    if (!walk) {  // (uniform)
      float lo[3], hi[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        lo[k] = box[(size_t)t * 6 + k];
        hi[k] = box[(size_t)t * 6 + 3 + k];
      }
      walk = !skips(lo, hi);
    }
    if (!__syncthreads_or(walk)) continue;  // (uniform; the barrier also closes the reads of the tile before)
    float g[3];
    point(t * NN_TILE + tid, g);
    tile[tid] = make_float4(g[0], g[1], g[2], 0.f);
    __syncthreads();
    const int cnt = min(NN_TILE, V - t * NN_TILE);
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) fold(tile[jj]);
  }
}

// RECIPE a for one workgroup of four waves: the points chunk * 1024 + j * 256 + tid (j = 0 .. 3) under E against every point under
// G, whose boxes are box (T,6); the terms of the live points are added to *sum, one atomic per wave.  The walk begins at the tiles
// of the workgroup's own indices.  Every thread of the workgroup calls it
__device__ __forceinline__ void nn_adi_chunk(const float* __restrict__ points, int V, int chunk, const float* __restrict__ E,
                                             const float* __restrict__ G, int T, const float* __restrict__ box, float inv_unit, int flags,
                                             unsigned long long* __restrict__ sum) {
  const int tid = threadIdx.x;
  float e[NN_PTS][3], m[NN_PTS];
  bool live[NN_PTS];
#pragma unroll
  for (int j = 0; j < NN_PTS; ++j) {
    const int idx = chunk * NN_CHUNK + j * NN_WG + tid;  // below 2^20 + 1024
    live[j] = idx < V;
    nn_point(points, V, idx, E, e[j]);
    m[j] = INFINITY;
  }
  const int first = chunk * NN_PTS;  // the tile of the workgroup's first point: below T
  nn_walk(
      V, box, flags, [&](int s) { return s < T ? (first + s < T ? first + s : first + s - T) : -1; },
      [&](const float(&lo)[3], const float(&hi)[3]) {
        bool all = true;
#pragma unroll
        for (int j = 0; j < NN_PTS; ++j) all = all && (!live[j] || nn_lower_bound(e[j], lo, hi) > m[j]);
        return all;
      },
      [&](int idx, float(&g)[3]) { nn_point(points, V, idx, G, g); },
      [&](const float4 g) {
#pragma unroll
        for (int j = 0; j < NN_PTS; ++j) m[j] = fminf(m[j], pe_d2(e[j], g.x, g.y, g.z));  // m is never a NaN: d2 < m ? d2 : m
      });
  long long term = 0;
#pragma unroll
  for (int j = 0; j < NN_PTS; ++j)
    if (live[j]) term += pe_add_term(m[j], inv_unit);
  term = wave_sum(term);
  if ((tid & 63) == 0 && term) __hip_atomic_fetch_add(sum, (unsigned long long)term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// The boxes' launch, one copy for both ADI entries (defined in nearest.hip): nn_boxes_kernel over (T, N), box (N,T,6) f32, every
// word written.  `who` names the entry in an error text.  -> 0, or the hipError_t with sam6d_set_error() called.
int nn_boxes(const char* who, const float* points, int V, const float* gt, int N, float* box, hipStream_t st);
