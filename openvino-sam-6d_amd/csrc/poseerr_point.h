// The pieces of the distance recipe (poseerr.hip RECIPE a) in one copy for the scoring family: the constants, the guarded point
// load, d2, the ADD term and the per-point step under a composed matrix, for pair_errors_kernel (posematch.hip: the one kernel that
// walks model points under composed matrices, for sam6d_pose_pair_errors and, on the diagonal, sam6d_pose_point_errors) and for
// nearest.hip's searches; the bit-pattern helpers around them; and the host pieces the entries share.  The recipe is written out at
// the top of poseerr.hip and nowhere else; every function here names the line of it that it is.
#pragma once
#include "raster.h"
#include "common.h"

#define PE_WG 256
#define PE_PTS 4                    // points per thread
#define PE_CHUNK (PE_WG * PE_PTS)   // points per workgroup
#define PE_ST 128                   // composed matrices per LDS tile
#define PE_NAN 0x7fc00000u
#define PE_SCALE 1073741824.0       // 2^30
#define PE_TERM_MAX 4398046511104.0 // 2^42

struct PeCam {
  float fx, fy, cx, cy;
};

// the point idx of (V,3), zeros beyond V
__device__ __forceinline__ void pe_load_point(const float* __restrict__ points, int V, int idx, float (&x)[3]) {
  x[0] = x[1] = x[2] = 0.f;
  if (idx < V) {
    x[0] = points[(size_t)idx * 3];
    x[1] = points[(size_t)idx * 3 + 1];
    x[2] = points[(size_t)idx * 3 + 2];
  }
}

// RECIPE d2
__device__ __forceinline__ float pe_d2(const float (&a)[3], float bx, float by, float bz) {
  const float dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// RECIPE ADD: one point's term
__device__ __forceinline__ long long pe_add_term(float d2, float inv_unit) {
  double w = ((double)sqrtf(d2) * (double)inv_unit) * PE_SCALE;
  if (!(w <= PE_TERM_MAX)) w = PE_TERM_MAX;
  return (long long)rint(w);
}

// RECIPE maxima: the word a value offers
__device__ __forceinline__ unsigned pe_bits(float v) { return v > 0.f ? __float_as_uint(v) : (v == 0.f ? 0u : PE_NAN); }

template <int CTRL>
__device__ __forceinline__ unsigned pe_dpp(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
// the maximum over the wave in every lane, on the DPP path as common.h's wave_max_dpp: rotations inside each row of 16, then the
// exchanges with the lanes 16 and 32 away
__device__ __forceinline__ unsigned pe_wave_max(unsigned v) {
  typedef unsigned u2_ __attribute__((ext_vector_type(2)));
  v = max(v, pe_dpp<0x128>(v));  // row_ror:8
  v = max(v, pe_dpp<0x124>(v));  // row_ror:4
  v = max(v, pe_dpp<0x122>(v));  // row_ror:2
  v = max(v, pe_dpp<0x121>(v));  // row_ror:1
  const u2_ a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = max(v, (threadIdx.x & 16) ? a[0] : a[1]);
  const u2_ b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max(v, (threadIdx.x & 32) ? b[0] : b[1]);
}

__device__ __forceinline__ unsigned long long pe_wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// RECIPE G: element k = 4 r + c of fl32(Gt o Sm), both (3,4) row-major
__device__ __forceinline__ float pe_compose(const float* __restrict__ Gt, const float* __restrict__ Sm, int k) {
  const int r = k >> 2, c = k & 3;
  double a = (double)Gt[r * 4] * (double)Sm[c];
  a = a + (double)Gt[r * 4 + 1] * (double)Sm[4 + c];
  a = a + (double)Gt[r * 4 + 2] * (double)Sm[8 + c];
  if (c == 3) a = a + (double)Gt[r * 4 + 3];
  return (float)a;
}

// the points of one thread and what does not change over the matrices: x, e = E x, e's pixel (PIX), whether e lies in front
template <bool PIX>
struct PePoints {
  float x[PE_PTS][3], e[PE_PTS][3], ue[PE_PTS], ve[PE_PTS];
  bool live[PE_PTS], front[PE_PTS];

  // points chunk * 1024 + j * 256 + tid for j = 0 .. 3 (below 2^20 + 1024); RECIPE points, pixels for E
  __device__ __forceinline__ void load(const float* __restrict__ points, int V, int chunk, int tid, const float* __restrict__ E, const PeCam& cam) {
#pragma unroll
    for (int j = 0; j < PE_PTS; ++j) {
      const int idx = chunk * PE_CHUNK + j * PE_WG + tid;
      live[j] = idx < V;
      pe_load_point(points, V, idx, x[j]);
      rs_to_camera(E, x[j], e[j]);
      front[j] = e[j][2] > 0.f;
      if (PIX) {
        ue[j] = cam.fx * (e[j][0] / e[j][2]) + cam.cx;
        ve[j] = cam.fy * (e[j][1] / e[j][2]) + cam.cy;
      }
    }
  }

  // RECIPE d2, pixels, skipped, maxima for the matrix M (12 floats in registers): the thread's words m2, mp over its live points;
  // d2s and skip per point for the caller's ADD
  __device__ __forceinline__ void step(const float (&M)[12], const PeCam& cam, unsigned& m2, unsigned& mp, float (&d2s)[PE_PTS], bool (&skip)[PE_PTS]) const {
    m2 = 0u;
    mp = 0u;
#pragma unroll
    for (int j = 0; j < PE_PTS; ++j) {
      float g[3];
      rs_to_camera(M, x[j], g);
      const float d2 = pe_d2(e[j], g[0], g[1], g[2]);
      d2s[j] = d2;
      skip[j] = !(front[j] && g[2] > 0.f);
      if (live[j]) m2 = max(m2, pe_bits(d2));
      if (PIX) {
        const float ug = cam.fx * (g[0] / g[2]) + cam.cx, vg = cam.fy * (g[1] / g[2]) + cam.cy;
        const float du = ue[j] - ug, dv = ve[j] - vg;
        const float p2 = du * du + dv * dv;
        if (live[j] && !skip[j]) mp = max(mp, pe_bits(p2));
      }
    }
  }

  // RECIPE ADD, skipped: the thread's sum of terms and count of skipped points, of its live points
  __device__ __forceinline__ void add_terms(const float (&d2s)[PE_PTS], const bool (&skip)[PE_PTS], float inv_unit, long long& term, int& skipped) const {
    term = 0;
    skipped = 0;
#pragma unroll
    for (int j = 0; j < PE_PTS; ++j) {
      if (!live[j]) continue;
      term += pe_add_term(d2s[j], inv_unit);
      skipped += skip[j] ? 1 : 0;
    }
  }
};

// ---- host side ----------------------------------------------------------------------------------------------------------
// the refusal of an inv_unit that is not a finite number > 0 -> 0 or SAM6D_EINVAL with the error text set
static inline int pe_check_inv_unit(const char* who, float inv_unit) {
  SAM6D_REQUIRE(inv_unit > 0.f && inv_unit <= 3.4028234e38f, "%s: inv_unit = %g is not a finite number > 0", who, (double)inv_unit);
  return 0;
}

// what the two VSD entries share (sam6d_pose_vsd in poseerr.hip, sam6d_pose_pair_vsd in vsdpairs.hip): the tolerances as a kernel
// argument and their refusals, by name
#define PE_MAX_T 16

struct PeTaus {
  float v[PE_MAX_T];
};

static inline int pe_check_vsd(const char* who, int wave_area, float delta, float inv_norm, float fx, float fy, int T) {
  SAM6D_REQUIRE(wave_area >= 0, "%s: wave_area = %d is negative", who, wave_area);
  SAM6D_REQUIRE(delta >= 0.f && delta <= 3.4028234e38f, "%s: delta = %g is not a finite number >= 0", who, (double)delta);
  SAM6D_REQUIRE(inv_norm > 0.f && inv_norm <= 3.4028234e38f, "%s: inv_norm = %g is not a finite number > 0", who, (double)inv_norm);
  SAM6D_REQUIRE(fx != 0.f && fy != 0.f && fx == fx && fy == fy, "%s: fx, fy = %g, %g: zero or not a number", who, (double)fx, (double)fy);
  SAM6D_REQUIRE(T >= 1 && T <= PE_MAX_T, "%s: T = %d is not in 1 .. %d", who, T, PE_MAX_T);
  return 0;
}

// taus (T floats on the host, not null) -> tv, zeros beyond T
static inline int pe_check_taus(const char* who, const float* taus, int T, PeTaus& tv) {
  for (int k = 0; k < PE_MAX_T; ++k) {
    tv.v[k] = k < T ? taus[k] : 0.f;
    SAM6D_REQUIRE(tv.v[k] >= 0.f && tv.v[k] <= 3.4028234e38f, "%s: taus[%d] = %g is not a finite number >= 0", who, k, (double)tv.v[k]);
  }
  return 0;
}

// Host side of the point errors, one copy for both entries (defined in posematch.hip): zeroes ws (A B S pairs of words), n_skipped
// (pix) and add_sum in stream order, picks the run of matrices per workgroup, launches pair_errors_kernel<pix, diag> and
// pair_errors_finish_kernel.  diag (with pix and B = 1 alone): a[i] is scored against b[i].  !pix: mspd, mspd_sym and n_skipped are
// not touched.  `who` names the entry in an error text.  -> 0, or the hipError_t with sam6d_set_error() called.
int pe_errors(const char* who, const float* points, int V, const float* a, int A, const float* b, int B, bool diag, const float* syms, int S,
              const PeCam& cam, float inv_unit, bool pix, float* mssd, float* mspd, int* mssd_sym, int* mspd_sym, int* n_skipped,
              long long* add_sum, void* ws, hipStream_t st);
