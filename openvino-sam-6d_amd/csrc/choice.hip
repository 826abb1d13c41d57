// The random choice of points of get_test_data and _get_template (PEM/run_inference_custom_pytorch.py:337-340 and :215-218:
// np.random.choice(np.arange(n), ns, replace = n > ns)) drawn on the device.  numpy's Mersenne stream cannot be replayed per row on a
// GPU, so the draw has an integer definition of its own, counter based: every candidate r of a row gets the sort key
//   fmix(x):  x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16        (mod 2^32; a bijection)
//   a = fmix(seed ^ 0x9E3779B9),  b = fmix(a + row),  h(r) = fmix(fmix(r ^ b) + a)                  (a bijection of r: no ties)
// and a row of n candidates that wants ns indices gets
//   n > ns        the ns values r in [0, n) with the smallest h(r), in ascending order of h (random sort keys: a uniform subset in a
//                 uniform order -- the order matters, FPS starts from point 0)
//   1 <= n <= ns  sel[j] = (h(j) * n) >> 32 (64-bit product), the reference's draw with replacement
//   n <= 0        zeros.
// It matches the reference in distribution, not in its values.  tests/choice_ref.py restates it in numpy.
//
// One workgroup of 1024 threads per row; the kernel reads nothing but n[row], every key is recomputed from r wherever it is needed.
// n > ns: an 8-bit radix select finds the ns-th smallest key T -- four passes over r = 0 .. n - 1, most significant byte first, each a
// 256-bin LDS histogram of the keys that agree with the bytes fixed so far; a collect pass puts the (h, r) pairs with h <= T into LDS
// (exactly ns of them: the keys are distinct; LDS atomics hand out the slots in any order), the slots up to the next power of two are
// filled with the largest 64-bit value, and a bitonic sort of h << 32 | r makes the output a function of (seed, row, n, ns) alone.
// 8192 pairs are 64 KB of LDS: hence ns <= 8192.  Integer VALU and LDS work, no MFMA; five hashes per candidate.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define CH_THREADS 1024
#define CH_MAX_NS 8192
#define CH_MAX_N (1 << 24)

// (fmix and the key h(r) are hash_fmix / hash_key of common.h: meshsample.hip draws from the same keys)

// P = the power of two >= ns (the sort's size); dynamic LDS = P pairs of 8 bytes
__global__ __launch_bounds__(CH_THREADS) void draw_choice_kernel(const int* __restrict__ n_in, int ns, int P, unsigned seed, unsigned row0,
                                                                 int* __restrict__ sel) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long ch_pairs[];
  __shared__ int s_hist[256];
  __shared__ int s_wave[4];
  __shared__ int s_bin, s_need, s_cnt;
  const int i = blockIdx.x, t = threadIdx.x;
  const unsigned a = hash_fmix(seed ^ 0x9E3779B9u);
  const unsigned b = hash_fmix(a + (row0 + (unsigned)i));
  const int n = min(n_in[i], CH_MAX_N);
  int* out = sel + (size_t)i * ns;
  if (n <= ns) {  // with replacement (n >= 1), or an empty row: a plain map
    for (int j = t; j < ns; j += CH_THREADS)
      out[j] = n > 0 ? (int)(((unsigned long long)hash_key((unsigned)j, a, b) * (unsigned long long)(unsigned)n) >> 32) : 0;
    return;
  }
  // ---- radix select: after the pass at `shift` the bytes of T from `shift` up are known (prefix under mask)
  unsigned prefix = 0, mask = 0;
  int need = ns;  // T is the need-th smallest of the keys that agree with prefix under mask
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (t < 256) s_hist[t] = 0;
    __syncthreads();
    for (int r = t; r < n; r += CH_THREADS) {
      const unsigned k = hash_key((unsigned)r, a, b);
      if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    // the bin that holds the need-th key: exclusive count below it < need <= inclusive count (one bin, and it is not empty)
    int incl = 0, cnt = 0;
    if (t < 256) {
      cnt = s_hist[t];
      incl = wave_incl_scan_i32_dpp(cnt);
      if ((t & 63) == 63) s_wave[t >> 6] = incl;
    }
    __syncthreads();
    if (t < 256) {
      for (int w = 0; w < (t >> 6); ++w) incl += s_wave[w];
      if (incl - cnt < need && need <= incl) {
        s_bin = t;
        s_need = need - (incl - cnt);
      }
    }
    __syncthreads();
    prefix |= (unsigned)s_bin << shift;
    mask |= 255u << shift;
    need = s_need;
  }
  // ---- collect the ns pairs with h <= T, pad to P, sort
  if (t == 0) s_cnt = 0;
  for (int j = ns + t; j < P; j += CH_THREADS) ch_pairs[j] = ~0ull;  // above every real pair (r < 2^24)
  __syncthreads();
  for (int r = t; r < n; r += CH_THREADS) {
    const unsigned k = hash_key((unsigned)r, a, b);
    if (k <= prefix) {
      const int slot = atomicAdd(&s_cnt, 1);
      if (slot < ns) ch_pairs[slot] = ((unsigned long long)k << 32) | (unsigned)r;  // (always: exactly ns keys are <= T)
    }
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = t; e < P; e += CH_THREADS) {
        const int p = e ^ j;
        if (p > e) {
          const unsigned long long x = ch_pairs[e], y = ch_pairs[p];
          if ((x > y) == ((e & k) == 0)) {
            ch_pairs[e] = y;
            ch_pairs[p] = x;
          }
        }
      }
      __syncthreads();
    }
  for (int j = t; j < ns; j += CH_THREADS) out[j] = (int)(unsigned)(ch_pairs[j] & 0xffffffffull);
}

extern "C" int sam6d_draw_choice(const int* n, int N, int ns, unsigned seed, unsigned row0, int* sel, void* stream) {
  SAM6D_REQUIRE(ns >= 1 && ns <= CH_MAX_NS, "draw_choice: ns = %d is not in 1 .. %d", ns, CH_MAX_NS);
  SAM6D_REQUIRE(N >= 0, "draw_choice: N = %d is negative", N);
  if (N == 0) return 0;
  SAM6D_REQUIRE(n && sel, "draw_choice: null pointer");
  int P = 1;
  while (P < ns) P <<= 1;
  const int lds = P * (int)sizeof(unsigned long long);
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "draw_choice", {{(const void*)draw_choice_kernel, CH_MAX_NS * (int)sizeof(unsigned long long)}})) return rc;
  hipLaunchKernelGGL(draw_choice_kernel, dim3(N), dim3(CH_THREADS), lds, (hipStream_t)stream, n, ns, P, seed, row0, sel);
  SAM6D_LAUNCH_CHECK("draw_choice");
}
