// All-pairs pose errors, and what is built on an error matrix: the greedy matching of estimates to ground-truth instances (BOP's
// match_poses in kind: Hodan et al., "BOP Challenge 2020 on 6D Object Localization", section 2.4) and the greedy removal of duplicate
// poses.  The reference has neither: it writes all its poses with their scores (PEM/run_inference_custom_pytorch.py:460-471) and
// leaves matching and scoring to bop_toolkit.  The error of a pair is poseerr.hip's, bit for bit; the matching and the suppression
// are the package's own recipes, restated in tests/posematch_ref.py and pinned against that restatement -- NOT against bop_toolkit,
// which the suite does not have.  Every comparison with the restatement is bit for bit.
//
// RECIPE.  Float comparisons are IEEE fp32 comparisons; everything else is integer.
//
//  a. pair errors (sam6d_pose_pair_errors), per (i, j) in A x B: exactly what sam6d_pose_point_errors gives for est = a[i],
//     gt = b[j] -- poseerr.hip RECIPE a, through the one copy of its per-point step in poseerr_point.h.  Nothing of it is restated
//     here.  With the flag PM_NO_MSPD the pixel half of that recipe (the projections, their divisions, the skipped points) is not
//     computed and mspd, mspd_sym, n_skipped are not written.
//
//  the order (b and c): estimates by descending score, equal scores the lower index first, a NaN score after every number.
//     key(v) = 0 for a NaN, else the bits of v (a zero of either sign as +0) with all bits flipped when the sign is set and the sign
//     bit set when it is not: key(u) < key(v) exactly when u < v.  position(i) = the number of j with key_j > key_i, or key_j == key_i
//     and j < i.
//
//  b. matching (sam6d_pose_match), for each threshold k on its own, walking the first n = (max_ests > 0 ? min(max_ests, A) : A)
//     estimates of the order: estimate i takes, among the targets j with valid[j], not taken before and err[i][j] < thr[k] (strict,
//     false for a NaN), the one with the smallest err[i][j], the lowest j among equal errors (-0 equals +0): the minimum of the 64-bit
//     keys key(err[i][j]) << 32 | j.  est_match[k][i] = j, gt_match[k][j] = i, -1 where there is none; n_matched[k] counts them.
//
//  c. suppression (sam6d_pose_nms), walking the order: pose i is kept unless a pose r kept before it has err[r][i] < thresh (the row
//     is the kept, higher-ranked pose; the matrix need not be symmetric; the diagonal is never read).  keep_idx = the kept poses in
//     order, then -1; suppressed_by[i] = the first kept pose in order that suppresses i, i itself when it is kept.  A pose that a
//     suppressed pose would suppress is not suppressed by it: greedy.
//
// WHY THE RESULT IS A FUNCTION OF THE INPUTS ALONE.  a: where workgroups meet it is an integer atomic at agent scope -- 32-bit maxima
// (the d2 and p2 bit patterns), 32-bit adds (n_skipped), 64-bit adds (add_sum) -- commutative and associative, so neither the order
// of the workgroups nor the split of the B S matrices over blockIdx.z (a launch heuristic) changes a bit.  The buffers are set by
// memsets that precede the kernel in stream order, nothing reads a buffer in the launch that reduces into it, and mssd, mspd and
// their indices have one writer, pair_errors_finish_kernel's wave of the pair.  b and c have no atomics at all: the order is a rank
// (every position written once), a threshold's matching is one wave's walk, the mask words have one writer each and the scan is one
// wave's walk.
//
// WORK.  a: A B S V point transforms.  A workgroup of four waves takes 1024 points under one a[i], four per thread, and keeps their
// x, e and (u_e, v_e) in registers across its share of the B S matrices b[j] o syms[s] (m = j S + s); 128 of them at a time are formed
// once per workgroup into LDS and read from there as broadcasts; per matrix the wave's two maxima are reduced on the DPP path, meet
// the other waves' in LDS, and leave as one atomic per word, workgroup and tile; the ADD terms of a matrix with s = 0 meet in LDS in
// the same way.  blockIdx.z splits the matrices into runs of 8 .. 256: a small A x V still fills the chip, and a large B S does not
// make workgroups so long that the last round of them leaves most of the chip idle (measured: DESIGN section 8, f21).  finish: one
// wave per pair takes the minima over s as 64-bit keys (bits << 32 | s: the lowest s wins a tie).  sam6d_pose_point_errors
// (poseerr.hip) is the same launch on the diagonal: B = 1 and b's row taken from i, so A = N poses against their own ground truths
// under the same split.  b: one wave per threshold; lane l holds the taken flags of the targets l, l + 64,
// ..., sixteen per lane, in one register, and the next estimate's row is loaded while the present one is decided.  c: the bit mask
// over the ordered poses (one thread per row and word, the upper triangle), then one wave whose lane w owns removed-word w.
//
// WHAT THE HOST CANNOT SEE.  Nothing that addresses memory: no index is read from a caller's buffer.  The order lies in the
// workspace, written by pm_order_kernel of the same call as a permutation of 0 .. N-1 whatever the scores hold.  The values of err,
// scores, thr and valid only decide comparisons.
#include "poseerr_point.h"
#include "../../include/sam6d_hip.h"

#define PM_MAX_V (1 << 20)
#define PM_MAX_N 1024               // A, B, S, and c's N
#define PM_MAX_TRIPLES (1 << 22)    // A B S
#define PM_MAX_T 64
#define PM_NO_MSPD 1                // flags bit 0
#define PM_WGS 2048                 // the pair kernel aims at this many workgroups
#define PM_MIN_RUN 8                // and gives one at least this many matrices,
#define PM_MAX_RUN 256              // at most this many: short workgroups, so that the last round of them wastes little of the chip
#define PM_Q (PM_MAX_N / 64)        // targets per lane

// ---------------------------------------------------------------------------------------------------------- a. pair errors
// grid (ceil(V / 1024), A, Z), four waves; the workgroup's matrices are m = blockIdx.z * run .. + run - 1 (below B S).
// ws (A, B S, 2) u32 arrives zeroed: word 0 the d2 maximum of the triple, word 1 the p2 maximum.  DIAG (then B = 1): the pose
// b[i] stands for b[0], the diagonal of A x A without the rest of it
template <bool PIX, bool DIAG>
__global__ __launch_bounds__(PE_WG) void pair_errors_kernel(const float* __restrict__ points, int V, const float* __restrict__ a,
                                                            const float* __restrict__ b, int B, const float* __restrict__ syms, int S, int run,
                                                            PeCam cam, float inv_unit, unsigned* __restrict__ ws, int* __restrict__ n_skipped,
                                                            unsigned long long* __restrict__ add_sum) {
  __shared__ float G[PE_ST][12];
  __shared__ unsigned mx[PE_ST * 2];
  __shared__ unsigned long long addl[PE_ST];
  __shared__ int skl[PE_ST];
  const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, BS = B * S;  // B S <= 2^20
  const int m_lo = blockIdx.z * run, m_hi = min(BS, m_lo + run);
  if (DIAG) b += (size_t)i * 12;
  PePoints<PIX> P;
  P.load(points, V, blockIdx.x, tid, a + (size_t)i * 12, cam);
  for (int m0 = m_lo; m0 < m_hi; m0 += PE_ST) {
    const int cnt = min(PE_ST, m_hi - m0);
    __syncthreads();  // the tile before is flushed
    for (int t = tid; t < cnt * 12; t += PE_WG) {
      const int m = m0 + t / 12, j = m / S;
      G[t / 12][t % 12] = pe_compose(b + (size_t)j * 12, syms + (size_t)(m - j * S) * 12, t % 12);
    }
    for (int t = tid; t < cnt; t += PE_WG) {
      mx[t * 2] = mx[t * 2 + 1] = 0u;
      addl[t] = 0ull;
      skl[t] = 0;
    }
    __syncthreads();
    int s = m0 % S;
    for (int sl = 0; sl < cnt; ++sl) {
      float M[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) M[k] = G[sl][k];
      unsigned m2, mp;
      float d2s[PE_PTS];
      bool skip[PE_PTS];
      P.step(M, cam, m2, mp, d2s, skip);
      if (s == 0) {  // (uniform) ADD and the skipped points, of the first symmetry alone
        long long term;
        int skipped;
        P.add_terms(d2s, skip, inv_unit, term, skipped);
        term = wave_sum(term);
        if (PIX) skipped = wave_sum(skipped);
        if (lane == 0) {
          if (term) __hip_atomic_fetch_add(&addl[sl], (unsigned long long)term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (PIX && skipped) atomicAdd(&skl[sl], skipped);
        }
      }
      s = s + 1 == S ? 0 : s + 1;
      m2 = pe_wave_max(m2);
      if (PIX) mp = pe_wave_max(mp);
      if (lane == 0) {
        if (m2) atomicMax(&mx[sl * 2], m2);
        if (PIX && mp) atomicMax(&mx[sl * 2 + 1], mp);
      }
    }
    __syncthreads();
    for (int t = tid; t < cnt * 2; t += PE_WG) {
      const unsigned v = mx[t];
      if (v) __hip_atomic_fetch_max(ws + ((size_t)i * BS + m0) * 2 + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int t = tid; t < cnt; t += PE_WG) {
      const int m = m0 + t, j = m / S;
      if (m != j * S) continue;
      const size_t pair = (size_t)i * B + j;
      if (addl[t]) __hip_atomic_fetch_add(add_sum + pair, addl[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (PIX && skl[t]) __hip_atomic_fetch_add(n_skipped + pair, skl[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// one wave per pair, four to a workgroup: the only writer of mssd, mspd and their indices.  mspd == nullptr: MSSD alone
__global__ __launch_bounds__(256) void pair_errors_finish_kernel(const unsigned* __restrict__ ws, int pairs, int S, float* __restrict__ mssd,
                                                                 float* __restrict__ mspd, int* __restrict__ mssd_sym,
                                                                 int* __restrict__ mspd_sym) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= pairs) return;  // (uniform over the wave)
  unsigned long long k2 = ~0ull, kp = ~0ull;
  for (int s = lane; s < S; s += 64) {
    const unsigned* w = ws + ((size_t)n * S + s) * 2;
    const unsigned long long c = ((unsigned long long)w[0] << 32) | (unsigned)s, d = ((unsigned long long)w[1] << 32) | (unsigned)s;
    k2 = c < k2 ? c : k2;
    kp = d < kp ? d : kp;
  }
  k2 = pe_wave_min_u64(k2);
  kp = pe_wave_min_u64(kp);
  if (lane != 0) return;
  mssd[n] = sqrtf(__uint_as_float((unsigned)(k2 >> 32)));
  mssd_sym[n] = (int)(unsigned)(k2 & 0xffffffffull);
  if (mspd == nullptr) return;
  mspd[n] = sqrtf(__uint_as_float((unsigned)(kp >> 32)));
  mspd_sym[n] = (int)(unsigned)(kp & 0xffffffffull);
}

// poseerr_point.h's pe_errors: the host side of both entries.  ws holds A B S pairs of words
int pe_errors(const char* who, const float* points, int V, const float* a, int A, const float* b, int B, bool diag, const float* syms, int S,
              const PeCam& cam, float inv_unit, bool pix, float* mssd, float* mspd, int* mssd_sym, int* mspd_sym, int* n_skipped,
              long long* add_sum, void* ws, hipStream_t st) {
  const size_t pairs = (size_t)A * B;
  hipError_t e = hipMemsetAsync(ws, 0, pairs * S * 2 * sizeof(unsigned), st);
  if (e == hipSuccess && pix) e = hipMemsetAsync(n_skipped, 0, pairs * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(add_sum, 0, pairs * sizeof(long long), st);
  SAM6D_MEMSET_CHECK(who, e);
  // the split of the B S matrices over blockIdx.z: enough workgroups for the chip, runs of PM_MIN_RUN .. PM_MAX_RUN matrices
  const int chunks = (V + PE_CHUNK - 1) / PE_CHUNK, BS = B * S;
  const long long wgs = (long long)chunks * A;
  const int zwant = (int)((PM_WGS + wgs - 1) / wgs);
  const int per = (BS + zwant - 1) / zwant, run = per < PM_MIN_RUN ? PM_MIN_RUN : (per > PM_MAX_RUN ? PM_MAX_RUN : per);
  const dim3 grid(chunks, A, (BS + run - 1) / run);  // z <= max(PM_WGS, 2^20 / PM_MAX_RUN) = 4096
  const auto kernel = diag ? pair_errors_kernel<true, true> : (pix ? pair_errors_kernel<true, false> : pair_errors_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(PE_WG), 0, st, points, V, a, b, B, syms, S, run, cam, inv_unit, (unsigned*)ws,
                     pix ? n_skipped : (int*)nullptr, (unsigned long long*)add_sum);
  char step[64];
  snprintf(step, sizeof step, "%s (points)", who);
  SAM6D_LAUNCH_CHECK_CONT(step);
  hipLaunchKernelGGL(pair_errors_finish_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, (const unsigned*)ws, (int)pairs, S, mssd,
                     pix ? mspd : (float*)nullptr, mssd_sym, mspd_sym);
  snprintf(step, sizeof step, "%s (finish)", who);
  SAM6D_LAUNCH_CHECK(step);
}

static bool pm_sizes_ok(int A, int B, int S) {
  return A >= 1 && A <= PM_MAX_N && B >= 1 && B <= PM_MAX_N && S >= 1 && S <= PM_MAX_N && (long long)A * B * S <= PM_MAX_TRIPLES;
}

extern "C" size_t sam6d_pose_pair_errors_workspace_bytes(int A, int B, int S) {
  if (!pm_sizes_ok(A, B, S)) return 0;
  return (size_t)A * B * S * 2 * sizeof(unsigned);
}

extern "C" int sam6d_pose_pair_errors(const float* points, int V, const float* a, int A, const float* b, int B, const float* syms, int S,
                                      float fx, float fy, float cx, float cy, float inv_unit, int flags, float* mssd, float* mspd,
                                      int* mssd_sym, int* mspd_sym, int* n_skipped, long long* add_sum, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(V >= 1 && V <= PM_MAX_V, "pose_pair_errors: V = %d is not in 1 .. %d", V, PM_MAX_V);
  SAM6D_REQUIRE(A >= 1 && A <= PM_MAX_N, "pose_pair_errors: A = %d is not in 1 .. %d", A, PM_MAX_N);
  SAM6D_REQUIRE(B >= 1 && B <= PM_MAX_N, "pose_pair_errors: B = %d is not in 1 .. %d", B, PM_MAX_N);
  SAM6D_REQUIRE(S >= 1 && S <= PM_MAX_N, "pose_pair_errors: S = %d is not in 1 .. %d", S, PM_MAX_N);
  SAM6D_REQUIRE(pm_sizes_ok(A, B, S), "pose_pair_errors: A B S = %lld is above the cap of %d", (long long)A * B * S, PM_MAX_TRIPLES);
  if (const int bad = pe_check_inv_unit("pose_pair_errors", inv_unit)) return bad;
  SAM6D_REQUIRE((flags & ~PM_NO_MSPD) == 0, "pose_pair_errors: flags = %d has bits beyond bit 0", flags);
  const bool pix = !(flags & PM_NO_MSPD);
  SAM6D_POINTER("pose_pair_errors", points);
  SAM6D_POINTER("pose_pair_errors", a);
  SAM6D_POINTER("pose_pair_errors", b);
  SAM6D_POINTER("pose_pair_errors", syms);
  SAM6D_POINTER("pose_pair_errors", mssd);
  SAM6D_POINTER("pose_pair_errors", mssd_sym);
  if (pix) {
    SAM6D_POINTER("pose_pair_errors", mspd);
    SAM6D_POINTER("pose_pair_errors", mspd_sym);
    SAM6D_POINTER("pose_pair_errors", n_skipped);
  }
  SAM6D_POINTER("pose_pair_errors", add_sum);
  SAM6D_POINTER("pose_pair_errors", workspace);
  const size_t need = sam6d_pose_pair_errors_workspace_bytes(A, B, S);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_pair_errors: workspace of %zu bytes is below sam6d_pose_pair_errors_workspace_bytes = %zu",
                workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)add_sum & 7) == 0, "pose_pair_errors: workspace or add_sum is not 8-byte aligned");
  return pe_errors("pose_pair_errors", points, V, a, A, b, B, false, syms, S, PeCam{fx, fy, cx, cy}, inv_unit, pix, mssd, mspd, mssd_sym, mspd_sym,
                   n_skipped, add_sum, workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------- the order
// RECIPE the order: key(u) < key(v) exactly when u < v, for numbers
__device__ __forceinline__ unsigned pm_key(float v) {
  const unsigned w = v == 0.f ? 0u : __float_as_uint(v);
  return (w & 0x80000000u) ? ~w : (w | 0x80000000u);
}
__device__ __forceinline__ unsigned pm_score_key(float v) { return v != v ? 0u : pm_key(v); }

// rank counting over L2-resident scores, as detections.hip's nms_order_kernel: every position is written once
__global__ __launch_bounds__(256) void pm_order_kernel(const float* __restrict__ scores, int N, int* __restrict__ order) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const unsigned ki = pm_score_key(scores[i]);
  int pos = 0;
  for (int j = 0; j < N; ++j) {
    const unsigned kj = pm_score_key(scores[j]);
    pos += (kj > ki) || (kj == ki && j < i);
  }
  order[pos] = i;
}

static size_t pm_order_bytes(int N) { return ((size_t)N * sizeof(int) + 15) & ~(size_t)15; }

// ---------------------------------------------------------------------------------------------------------- b. matching
// grid (T), one wave: lane l owns the targets l + 64 q, bit q of `open` = valid and not taken.  est_match and gt_match arrive as -1
__global__ __launch_bounds__(64) void pm_match_kernel(const float* __restrict__ err, const int* __restrict__ order, int A, int B,
                                                      const float* __restrict__ thr, const unsigned char* __restrict__ valid, int n_take,
                                                      int* __restrict__ est_match, int* __restrict__ gt_match, int* __restrict__ n_matched) {
  const int k = blockIdx.x, lane = threadIdx.x, nq = (B + 63) >> 6;
  const float limit = thr[k];
  unsigned open = 0u;
#pragma unroll
  for (int q = 0; q < PM_Q; ++q) {
    const int j = q * 64 + lane;
    if (q < nq && j < B && (valid == nullptr || valid[j])) open |= 1u << q;
  }
  // the next estimate's row is on its way while this one is decided.  (Measured at 1024 x 1024: the walk is bound by the instructions
  // of the wave's scan and minimum, not by the loads; the order in LDS and rows two ahead were slower, 1.91 ms against 1.72 ms.)
  float cur[PM_Q], nxt[PM_Q];
  auto load_row = [&](int p, float (&row)[PM_Q]) {
    const float* r = err + (size_t)order[p] * B;
#pragma unroll
    for (int q = 0; q < PM_Q; ++q) {
      const int j = q * 64 + lane;
      row[q] = (q < nq && j < B) ? r[j] : 0.f;
    }
  };
  load_row(0, cur);
  int cnt = 0;
  for (int p = 0; p < n_take; ++p) {
    const int i = order[p];
    if (p + 1 < n_take) load_row(p + 1, nxt);
    unsigned long long best = ~0ull;
#pragma unroll
    for (int q = 0; q < PM_Q; ++q) {
      if (((open >> q) & 1u) && cur[q] < limit) {
        const unsigned long long key = ((unsigned long long)pm_key(cur[q]) << 32) | (unsigned)(q * 64 + lane);
        best = key < best ? key : best;
      }
    }
    best = pe_wave_min_u64(best);
    if (best != ~0ull) {  // (uniform)
      const int j = (int)(unsigned)(best & 0xffffffffull);
      if ((j & 63) == lane) open &= ~(1u << (j >> 6));
      if (lane == 0) {
        est_match[(size_t)k * A + i] = j;
        gt_match[(size_t)k * B + j] = i;
      }
      ++cnt;
    }
#pragma unroll
    for (int q = 0; q < PM_Q; ++q) cur[q] = nxt[q];
  }
  if (lane == 0) n_matched[k] = cnt;
}

extern "C" size_t sam6d_pose_match_workspace_bytes(int A) {
  if (A < 1 || A > PM_MAX_N) return 0;
  return pm_order_bytes(A);
}

extern "C" int sam6d_pose_match(const float* err, int A, int B, const float* scores, const float* thr, int T, const unsigned char* valid,
                                int max_ests, int* est_match, int* gt_match, int* n_matched, void* workspace, size_t workspace_bytes,
                                void* stream) {
  SAM6D_REQUIRE(A >= 1 && A <= PM_MAX_N, "pose_match: A = %d is not in 1 .. %d", A, PM_MAX_N);
  SAM6D_REQUIRE(B >= 1 && B <= PM_MAX_N, "pose_match: B = %d is not in 1 .. %d", B, PM_MAX_N);
  SAM6D_REQUIRE(T >= 1 && T <= PM_MAX_T, "pose_match: T = %d is not in 1 .. %d", T, PM_MAX_T);
  SAM6D_REQUIRE(max_ests >= 0, "pose_match: max_ests = %d is negative", max_ests);
  SAM6D_POINTER("pose_match", err);
  SAM6D_POINTER("pose_match", scores);
  SAM6D_POINTER("pose_match", thr);
  SAM6D_POINTER("pose_match", est_match);
  SAM6D_POINTER("pose_match", gt_match);
  SAM6D_POINTER("pose_match", n_matched);
  SAM6D_POINTER("pose_match", workspace);
  const size_t need = sam6d_pose_match_workspace_bytes(A);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_match: workspace of %zu bytes is below sam6d_pose_match_workspace_bytes = %zu", workspace_bytes,
                need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 3) == 0, "pose_match: workspace is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(est_match, 0xff, (size_t)T * A * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(gt_match, 0xff, (size_t)T * B * sizeof(int), st);
  SAM6D_MEMSET_CHECK("pose_match", e);
  int* order = (int*)workspace;
  hipLaunchKernelGGL(pm_order_kernel, dim3((A + 255) / 256), dim3(256), 0, st, scores, A, order);
  SAM6D_LAUNCH_CHECK_CONT("pose_match (order)");
  const int n_take = max_ests > 0 && max_ests < A ? max_ests : A;
  hipLaunchKernelGGL(pm_match_kernel, dim3(T), dim3(64), 0, st, err, (const int*)order, A, B, thr, valid, n_take, est_match, gt_match, n_matched);
  SAM6D_LAUNCH_CHECK("pose_match (match)");
}

// ---------------------------------------------------------------------------------------------------------- c. suppression
// the bit matrix over the ordered poses, as detections.hip's nms_mask_kernel: bit c of word (r, cw) = the pose at position
// cw * 64 + c comes after position r and err[order[r]][order[cw * 64 + c]] < thresh.  grid (nw, nw), one wave: thread t is row
// rb * 64 + t
__global__ __launch_bounds__(64) void pm_nms_mask_kernel(const float* __restrict__ err, const int* __restrict__ order, int N, int nw, float thresh,
                                                         unsigned long long* __restrict__ mask) {
  __shared__ int co[64];
  const int rb = blockIdx.y, cw = blockIdx.x, t = threadIdx.x;
  const int r = rb * 64 + t;
  if (cw < rb) {
    if (r < N) mask[(size_t)r * nw + cw] = 0ull;
    return;
  }
  if (cw * 64 + t < N) co[t] = order[cw * 64 + t];
  __syncthreads();
  if (r >= N) return;
  const float* row = err + (size_t)order[r] * N;
  unsigned long long bits = 0ull;
  const int cn = min(64, N - cw * 64);
  for (int c = (cw == rb ? t + 1 : 0); c < cn; ++c)
    if (row[co[c]] < thresh) bits |= 1ull << c;
  mask[(size_t)r * nw + cw] = bits;
}

// the greedy walk, one wave: lane w owns removed-word w (nw <= 16).  keep_idx arrives as -1
__global__ __launch_bounds__(64) void pm_nms_scan_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ order, int N, int nw,
                                                         long long* __restrict__ keep_idx, int* __restrict__ count,
                                                         int* __restrict__ suppressed_by) {
  const int lane = threadIdx.x;
  unsigned long long removed = 0ull;
  int cnt = 0;
  unsigned long long next = lane < nw ? mask[lane] : 0ull;
  for (int q = 0; q < nw; ++q) {
    const int oq = q * 64 + lane < N ? order[q * 64 + lane] : 0;
    const int cn = min(64, N - q * 64);
    for (int c = 0; c < cn; ++c) {
      const int p = q * 64 + c;
      const unsigned long long row = next;
      if (p + 1 < N) next = lane < nw ? mask[(size_t)(p + 1) * nw + lane] : 0ull;
      const unsigned long long word = __shfl(removed, q, 64);  // bit p is final: rows only ever set bits of later positions
      if ((word >> c) & 1ull) continue;                        // (uniform)
      const int o = __shfl(oq, c, 64);
      unsigned long long fresh = row & ~removed;
      removed |= row;
      while (fresh) {
        const int bit = __ffsll((long long)fresh) - 1;
        fresh &= fresh - 1;
        suppressed_by[order[lane * 64 + bit]] = o;  // lane < nw and the bit below N: the mask has no others
      }
      if (lane == 0) {
        keep_idx[cnt] = o;
        suppressed_by[o] = o;
      }
      ++cnt;
    }
  }
  if (lane == 0) count[0] = cnt;
}

extern "C" size_t sam6d_pose_nms_workspace_bytes(int N) {
  if (N < 1 || N > PM_MAX_N) return 0;
  return pm_order_bytes(N) + (size_t)N * ((N + 63) / 64) * sizeof(unsigned long long);
}

extern "C" int sam6d_pose_nms(const float* err, const float* scores, int N, float thresh, long long* keep_idx, int* count, int* suppressed_by,
                              void* workspace, size_t workspace_bytes, void* stream) {
  SAM6D_REQUIRE(N >= 1 && N <= PM_MAX_N, "pose_nms: N = %d is not in 1 .. %d", N, PM_MAX_N);
  SAM6D_POINTER("pose_nms", err);
  SAM6D_POINTER("pose_nms", scores);
  SAM6D_POINTER("pose_nms", keep_idx);
  SAM6D_POINTER("pose_nms", count);
  SAM6D_POINTER("pose_nms", suppressed_by);
  SAM6D_POINTER("pose_nms", workspace);
  const size_t need = sam6d_pose_nms_workspace_bytes(N);
  SAM6D_REQUIRE(workspace_bytes >= need, "pose_nms: workspace of %zu bytes is below sam6d_pose_nms_workspace_bytes = %zu", workspace_bytes, need);
  SAM6D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)keep_idx & 7) == 0, "pose_nms: workspace or keep_idx is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(keep_idx, 0xff, (size_t)N * sizeof(long long), st);
  SAM6D_MEMSET_CHECK("pose_nms", e);
  const int nw = (N + 63) / 64;
  int* order = (int*)workspace;
  unsigned long long* mask = (unsigned long long*)((char*)workspace + pm_order_bytes(N));
  hipLaunchKernelGGL(pm_order_kernel, dim3((N + 255) / 256), dim3(256), 0, st, scores, N, order);
  SAM6D_LAUNCH_CHECK_CONT("pose_nms (order)");
  hipLaunchKernelGGL(pm_nms_mask_kernel, dim3(nw, nw), dim3(64), 0, st, err, (const int*)order, N, nw, thresh, mask);
  SAM6D_LAUNCH_CHECK_CONT("pose_nms (mask)");
  hipLaunchKernelGGL(pm_nms_scan_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)mask, (const int*)order, N, nw, keep_idx, count,
                     suppressed_by);
  SAM6D_LAUNCH_CHECK("pose_nms (scan)");
}
