// Area-weighted samples of a mesh surface (trimesh.sample.sample_surface as the reference calls it: Render/render_custom_templates.py:35,
// ISM/run_inference_custom.py:232-234, PEM/run_inference_custom_pytorch.py:298-300) drawn on the device.  It is neither numpy's nor
// trimesh's stream: like choice.hip it has an integer definition of its own, equal to the reference in distribution only, restated in
// tests/meshsample_ref.py.  All float arithmetic is fp32 in the order written.
//   1. area[f] = sqrt((cx*cx + cy*cy) + cz*cz) * 0.5, c = (v1 - v0) x (v2 - v0); a face with an index outside [0, V), or whose area
//      is not > 0 (a NaN), counts as area 0.
//   2. area_max = the maximum (exact in any order: an integer atomicMax over the bit patterns of non-negative floats).
//   3. weight[f] = 0 for area 0, else max(1, min(2^24, (unsigned)floor(area / area_max * 2^24))).
//   4. start[f] = the exclusive prefix sum of the weights in uint64, total = their sum (integers: any scan order gives this table).
//   5. a = fmix(seed ^ 0x9E3779B9), b = fmix(a + 0x4D455348), h(r) = fmix(fmix(r ^ b) + a) (hash_key of common.h, modulo 2^32).
//      Sample j of a call is sample g = row + j of the stream (modulo 2^32) and takes h(3g), h(3g+1), h(3g+2):
//        u = (h(3g) * total) >> 32 (exact: total < 2^49);  face = the last f with start[f] <= u (its weight is not 0);
//        r1 = (h(3g+1) >> 8) / 2^24, r2 = (h(3g+2) >> 8) / 2^24; where r1 + r2 > 1: r1 = 1 - r1, r2 = 1 - r2;
//        point = (v0 + r1 * (v1 - v0)) + r2 * (v2 - v0) per coordinate.
// Launches: areas and their maximum; the weights' sums per 1024 faces; one workgroup scans those sums (at most 2^14 of them); the
// per-face starts; the samples.  The entry reads area_max back once (a stream synchronisation) to refuse a mesh without area before
// anything is written to the outputs.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define MS_MAX (1 << 24)
#define MS_BLOCK 1024
typedef unsigned long long u64;

__device__ __forceinline__ unsigned ms_weight(float area, float amax) {
  if (!(area > 0.f)) return 0u;
  float r = area / amax * 16777216.0f;
  r = r >= 1.f ? r : 1.f;
  r = r <= 16777216.0f ? r : 16777216.0f;
  return (unsigned)floorf(r);
}

__global__ __launch_bounds__(256) void ms_area_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int F,
                                                      float* __restrict__ area, unsigned* __restrict__ amax_bits) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  float a = 0.f;
  if (f < F) {
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
      const float* p = vert + (size_t)i0 * 3;
      const float* q = vert + (size_t)i1 * 3;
      const float* r = vert + (size_t)i2 * 3;
      const float ax = q[0] - p[0], ay = q[1] - p[1], az = q[2] - p[2];
      const float bx = r[0] - p[0], by = r[1] - p[1], bz = r[2] - p[2];
      const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      a = sqrtf((cx * cx + cy * cy) + cz * cz) * 0.5f;
      a = a > 0.f ? a : 0.f;
    }
    area[f] = a;
  }
  const float m = wave_max(a);
  if (lane_id() == 0 && m > 0.f) atomicMax(amax_bits, __float_as_uint(m));
}

// inclusive scan of one value per thread over the workgroup of MS_BLOCK threads
__device__ __forceinline__ u64 ms_block_scan(u64 v, u64* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < MS_BLOCK; o <<= 1) {
    const u64 x = t >= o ? s[t - o] : 0ull;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  return s[t];
}

__global__ __launch_bounds__(MS_BLOCK) void ms_block_sum_kernel(const float* __restrict__ area, int F, const unsigned* __restrict__ amax_bits,
                                                                u64* __restrict__ block_sum) {
  __shared__ u64 s[MS_BLOCK];
  const int f = blockIdx.x * MS_BLOCK + threadIdx.x;
  const float amax = __uint_as_float(*amax_bits);
  const u64 incl = ms_block_scan(f < F ? (u64)ms_weight(area[f], amax) : 0ull, s);
  if (threadIdx.x == MS_BLOCK - 1) block_sum[blockIdx.x] = incl;
}

// one workgroup: block_sum (NB) -> its exclusive prefix in place, total
__global__ __launch_bounds__(MS_BLOCK) void ms_scan_blocks_kernel(u64* __restrict__ block_sum, int NB, u64* __restrict__ total) {
  __shared__ u64 s[MS_BLOCK];
  const int per = (NB + MS_BLOCK - 1) / MS_BLOCK, lo = threadIdx.x * per, hi = min(lo + per, NB);
  u64 sum = 0;
  for (int i = lo; i < hi; ++i) sum += block_sum[i];
  const u64 incl = ms_block_scan(sum, s);
  u64 run = incl - sum;
  for (int i = lo; i < hi; ++i) {
    const u64 v = block_sum[i];
    block_sum[i] = run;
    run += v;
  }
  if (threadIdx.x == MS_BLOCK - 1) *total = incl;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_start_kernel(const float* __restrict__ area, int F, const unsigned* __restrict__ amax_bits,
                                                            const u64* __restrict__ block_start, u64* __restrict__ start) {
  __shared__ u64 s[MS_BLOCK];
  const int f = blockIdx.x * MS_BLOCK + threadIdx.x;
  const float amax = __uint_as_float(*amax_bits);
  const u64 w = f < F ? (u64)ms_weight(area[f], amax) : 0ull;
  const u64 incl = ms_block_scan(w, s);
  if (f < F) start[f] = block_start[blockIdx.x] + (incl - w);
}

__global__ __launch_bounds__(256) void ms_sample_kernel(const float* __restrict__ vert, const int* __restrict__ faces, int F,
                                                        const u64* __restrict__ start, const u64* __restrict__ total_p, int n, unsigned seed,
                                                        unsigned row, float* __restrict__ points, int* __restrict__ face_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned a = hash_fmix(seed ^ 0x9E3779B9u), b = hash_fmix(a + 0x4D455348u);
  const unsigned g = (row + (unsigned)j) * 3u;
  const unsigned h0 = hash_key(g, a, b), h1 = hash_key(g + 1u, a, b), h2 = hash_key(g + 2u, a, b);
  const u64 total = *total_p;
  const u64 u = (u64)h0 * (total >> 32) + (((u64)h0 * (total & 0xffffffffull)) >> 32);
  int lo = 0, hi = F - 1;  // the last f in [0, F) with start[f] <= u; start[0] = 0 <= u
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= u) lo = mid;
    else hi = mid - 1;
  }
  float r1 = (float)(h1 >> 8) / 16777216.0f, r2 = (float)(h2 >> 8) / 16777216.0f;
  if (r1 + r2 > 1.0f) {
    r1 = 1.0f - r1;
    r2 = 1.0f - r2;
  }
  // weight[lo] > 0, so its indices passed the check of ms_area_kernel
  const float* p = vert + (size_t)faces[(size_t)lo * 3] * 3;
  const float* q = vert + (size_t)faces[(size_t)lo * 3 + 1] * 3;
  const float* r = vert + (size_t)faces[(size_t)lo * 3 + 2] * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[(size_t)j * 3 + k] = (p[k] + r1 * (q[k] - p[k])) + r2 * (r[k] - p[k]);
  face_out[j] = lo;
}

static size_t ms_blocks(int F) { return (size_t)(F + MS_BLOCK - 1) / MS_BLOCK; }

// layout: [0] area_max bits (u32), [8] total (u64), [16] block sums (NB u64), then start (F u64), then area (F f32)
extern "C" size_t sam6d_mesh_sample_workspace_bytes(int F) {
  if (F < 1 || F > MS_MAX) return 0;
  return 16 + ms_blocks(F) * 8 + (size_t)F * 8 + (size_t)F * 4;
}

extern "C" int sam6d_mesh_sample(const float* vertices, int V, const int* faces, int F, int n, unsigned seed, unsigned row, float* points,
                                 int* face, void* workspace, size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(n >= 1 && n <= MS_MAX, "mesh_sample: n = %d is not in 1 .. %d", n, MS_MAX);
  SAM6D_REQUIRE(F >= 1 && F <= MS_MAX, "mesh_sample: F = %d is not in 1 .. %d", F, MS_MAX);
  SAM6D_REQUIRE(V >= 1, "mesh_sample: V = %d is not positive", V);
  SAM6D_REQUIRE(vertices && faces && points && face && workspace, "mesh_sample: null pointer");
  const size_t need = sam6d_mesh_sample_workspace_bytes(F);
  SAM6D_REQUIRE(workspace_bytes >= need, "mesh_sample: workspace of %zu bytes is below sam6d_mesh_sample_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0, "mesh_sample: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int NB = (int)ms_blocks(F);
  unsigned char* ws = (unsigned char*)workspace;
  unsigned* amax_bits = (unsigned*)ws;
  u64* total = (u64*)(ws + 8);
  u64* block_sum = (u64*)(ws + 16);
  u64* start = block_sum + NB;
  float* area = (float*)(start + F);
  hipError_t e = hipMemsetAsync(ws, 0, 16, s);
  if (e != hipSuccess) {
    sam6d_set_error("mesh_sample: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(ms_area_kernel, dim3((F + 255) / 256), dim3(256), 0, s, vertices, V, faces, F, area, amax_bits);
  SAM6D_LAUNCH_CHECK_CONT("mesh_sample (areas)");
  unsigned bits = 0;
  e = hipMemcpyAsync(&bits, amax_bits, sizeof(bits), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    sam6d_set_error("mesh_sample: reading area_max back failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  SAM6D_REQUIRE(bits != 0u && bits < 0x7f800000u, "mesh_sample: every face has zero area (or an area is not finite)");
  hipLaunchKernelGGL(ms_block_sum_kernel, dim3(NB), dim3(MS_BLOCK), 0, s, area, F, amax_bits, block_sum);
  SAM6D_LAUNCH_CHECK_CONT("mesh_sample (block sums)");
  hipLaunchKernelGGL(ms_scan_blocks_kernel, dim3(1), dim3(MS_BLOCK), 0, s, block_sum, NB, total);
  SAM6D_LAUNCH_CHECK_CONT("mesh_sample (scan)");
  hipLaunchKernelGGL(ms_start_kernel, dim3(NB), dim3(MS_BLOCK), 0, s, area, F, amax_bits, block_sum, start);
  SAM6D_LAUNCH_CHECK_CONT("mesh_sample (starts)");
  hipLaunchKernelGGL(ms_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, s, vertices, faces, F, start, total, n, seed, row, points, face);
  SAM6D_LAUNCH_CHECK("mesh_sample (samples)");
}
