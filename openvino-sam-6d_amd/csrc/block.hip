// Fused transformer-block kernels for 256-channel token rows: a tile of tokens stays on chip from the block's input to its second
// LayerNorm.
//
//   the layer tail -- what every attention layer of PEM/model/transformer.py ends with (AttentionLayer.forward :152-160 /
//             RPEAttentionLayer.forward :436-444 after the attention itself, then AttentionOutput :184-199):
//                 y   = LayerNorm(hidden . Wlin^T + b + x)
//                 out = LayerNorm(relu(y . Wexp^T + b) . Wsq^T + b + y)
//             on its own for the 197-token layers: token_tail_kernel (sam6d_token_block), which has a data flow of its own.
//   the dense layer -- the whole LinearTransformerLayer of the sparse-to-dense lift (:532-622) on the 2048 dense tokens of a cloud:
//                 q = D . Wq^T + b;  phi(q) (focused ReLU kernel);  z_h = 1 / (phi(q)_h . ksum_h + 1e-6);
//                 hidden_h = (phi(q)_h . kv_h) z_h;  then the layer tail with x = D: token_block_kernel (sam6d_linattn_layer).
//             (k / v side: the 196 sparse tokens, reduced to kv^T and key sums by tb_kv_fused_kernel)
//
// Before: 8 GEMM launches + 2 LayerNorm + focus passes per dense layer = twelve passes over 134 MB tensors (~3.2 GB of HBM traffic
// per layer); now D is read once and D' written once (268 MB).
//
// What follows describes token_block_kernel and the kernels that share its panel machinery (rpe_front, out_split, rows_linear).
// Layout: one workgroup = 4 waves, one wave = 16 tokens, and every product is computed TRANSPOSED:
//     Y^T (out-channel x token) = W (out-channel x k) . X^T (k x token)          v_mfma_f32_16x16x32_f16
// so the weights are the A operand (streamed through LDS by LDS-DMA, shared by the waves of a workgroup) and a wave's activations are the B
// operand, held in registers for the whole K extent (8 k-steps x {hi, lo} x 4 VGPRs = 64 VGPRs).  In the 16x16 accumulator a lane
// (token = lane & 15, g = lane >> 4) holds out-channels 4g .. 4g+3 of ITS OWN token; two such tiles give the 8 values the B operand of
// the next product wants from that lane, up to a fixed permutation inside every 32-channel block (slot 8g + e <-> channel
// 16 (e >> 2) + 4g + (e & 3)), which is applied to the weights once, when they are packed.  Between two products there is only the
// row-wise epilogue (bias, focus / LayerNorm statistics: a lane's 64 values + the three lanes 16 / 32 / 48 away) and the fp16 hi/lo
// split -- no LDS slab, no transposition.  <= 256 VGPRs, so the epilogue of one wave runs beside the MFMAs of its SIMD partner.
//
// Arithmetic: fp16 x3 split precision like gemm_nt_h3_kernel (a_lo.b_hi + a_hi.b_lo + a_hi.b_hi, fp32 accumulate), made range-safe:
// every weight matrix carries a power-of-two scale chosen at pack time (max |w| -> [2^13, 2^14)), every activation row a power-of-two
// scale chosen from its own max (the FFN hidden row: from a bound computed at pack time, because its chunks accumulate into one
// accumulator); the scales are undone exactly in the epilogues.  No operand can overflow fp16, no lo half falls into subnormals.
#include "common.h"
#include "../../include/sam6d_hip.h"
#include <stdlib.h>

// A panel = 32 weight rows x K (KS k-steps of 32): per row KS*32 hi halves | KS*32 lo halves, NO padding -- instead the 16-byte chunk
// c of row r is stored at chunk c ^ (r & 15), which makes the ds_read_b128 fragment reads (16 rows x 2 adjacent chunks per lane
// group) conflict-free.  The global image is stored swizzled, so a linear LDS-DMA copy reproduces it.
#define TB_ROWB(KS) ((KS) * 128)                // bytes of one weight row in a panel
#define TB_PBYTES(KS) (32 * TB_ROWB(KS))        // 32 768 (K=256), 16 384 (K=128), 8 192 (K=64): 32 / 16 / 8 DMA pieces of 1 KiB
#define TB_PANEL_BYTES TB_PBYTES(8)
#define TB_P256 TB_PBYTES(8)
#define TB_P128 TB_PBYTES(4)
#define TB_P64 TB_PBYTES(2)
#define TB_CHUNK_BYTES (4 * TB_P256 + 8 * TB_P128)  // one 128-wide FFN chunk: 4 expand panels + 8 squeeze panels
#define TB_Q_OFF (8 * TB_P256 + 4 * TB_CHUNK_BYTES) // proj_q panels follow the common part of the image
#define TB_IMAGE_BYTES(MODE) (TB_Q_OFF + ((MODE) ? 8 * TB_P256 : 0))
// constant vectors (floats)
#define TC_BQ 0
#define TC_ISP 256     // 1 / softplus(scale)
#define TC_BLIN 512
#define TC_G1 768
#define TC_BE1 1024
#define TC_BEXP 1280   // 512
#define TC_BSQ 1792
#define TC_G2 2048
#define TC_BE2 2304
#define TC_SC 2560     // inv_wq, inv_wlin, inv_wexp, inv_wsq_h (= 1 / (scale_wsq * scale_h)), scale_h
#define TC_N 2568

// slot p (0..31) of a 32-wide k-step <-> channel offset inside the step (see the header comment)
__host__ __device__ __forceinline__ int tb_slot_channel(int p) {
  const int g = p >> 3, e = p & 7;
  return 16 * (e >> 2) + 4 * g + (e & 3);
}

// ----------------------------------------------------------------------------------------------------- weight packing
// W (rows x ldw) fp32 -> panels of 32 rows x KS k-steps of 32 starting at column k0: per row [hi: KS*32 halves | lo: KS*32 halves |
// pad]; value = W * scale.
__global__ __launch_bounds__(256) void tb_pack_kernel(const float* __restrict__ W, long ldw, int k0, int KS, float scale,
                                                      unsigned char* __restrict__ dst) {
  const int panel = blockIdx.x;
  const int rowb = TB_ROWB(KS);
  unsigned char* out = dst + (size_t)panel * TB_PBYTES(KS);
  for (int i = threadIdx.x; i < 32 * KS * 32; i += 256) {
    const int m = i / (KS * 32), p = i % (KS * 32);
    const int col = k0 + 32 * (p >> 5) + tb_slot_channel(p & 31);
    const float v = W[(size_t)(panel * 32 + m) * ldw + col] * scale;
    _Float16 hi, lo;
    sam6d_split_f16(v, hi, lo);
    // logical half index -> 16-byte chunk (8 halves) -> swizzled chunk
    const int ch = p >> 3, cl = (KS * 32 + p) >> 3;
    _Float16* row = reinterpret_cast<_Float16*>(out + (size_t)m * rowb);
    row[((ch ^ (m & 15)) << 3) + (p & 7)] = hi;
    row[((cl ^ (m & 15)) << 3) + (p & 7)] = lo;
  }
}

extern "C" int sam6d_pack_panels(const float* W, long ldw, int rows, int k0, int ksteps, float scale, void* dst, void* stream) {
  SAM6D_REQUIRE(W && dst && rows > 0 && (rows % 32) == 0 && k0 >= 0 && (ksteps == 2 || ksteps == 4 || ksteps == 8) && scale > 0.f,
                "pack_panels: bad arguments (ksteps = K / 32 must be 2, 4 or 8)");
  hipLaunchKernelGGL(tb_pack_kernel, dim3(rows / 32), dim3(256), 0, (hipStream_t)stream, W, ldw, k0, ksteps, scale,
                     (unsigned char*)dst);
  SAM6D_LAUNCH_CHECK("pack_panels");
}

// per cloud: kv^T (4 heads x 64 d x 64 c) -> 8 panels of 32 d-rows x K = 64 (head h: panels 2h, 2h+1), every head scaled by its own
// power of two (from the head's max |kv|); inv[4 b + h] = 1 / scale.
__global__ __launch_bounds__(256) void tb_kv_pack_kernel(const float* __restrict__ kvT, unsigned char* __restrict__ dst,
                                                         float* __restrict__ inv) {
  __shared__ float red[4][4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* src = kvT + (size_t)b * 16384;
  float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int hd = 0; hd < 4; ++hd)
    for (int i = t; i < 4096; i += 256) m[hd] = fmaxf(m[hd], fabsf(src[hd * 4096 + i]));
#pragma unroll
  for (int hd = 0; hd < 4; ++hd) {
    m[hd] = wave_max_dpp(m[hd]);
    if ((t & 63) == 0) red[hd][t >> 6] = m[hd];
  }
  __syncthreads();
  float scale[4];
#pragma unroll
  for (int hd = 0; hd < 4; ++hd) scale[hd] = pow2_scale(fmaxf(fmaxf(red[hd][0], red[hd][1]), fmaxf(red[hd][2], red[hd][3])));
  if (t < 4) inv[(size_t)b * 4 + t] = 1.0f / (t == 0 ? scale[0] : t == 1 ? scale[1] : t == 2 ? scale[2] : scale[3]);
  unsigned char* out = dst + (size_t)b * (8 * TB_P64);
  for (int i = t; i < 16384; i += 256) {
    const int hd = i >> 12, d = (i >> 6) & 63, p = i & 63;  // p: slot inside the 64-wide K
    const int c = 32 * (p >> 5) + tb_slot_channel(p & 31);
    const float sc = hd == 0 ? scale[0] : hd == 1 ? scale[1] : hd == 2 ? scale[2] : scale[3];
    const float v = src[(hd * 64 + d) * 64 + c] * sc;
    _Float16 hi, lo;
    sam6d_split_f16(v, hi, lo);
    const int mrow = d & 31;
    _Float16* row = reinterpret_cast<_Float16*>(out + (size_t)(2 * hd + (d >> 5)) * TB_P64 + (size_t)mrow * TB_ROWB(2));
    row[(((p >> 3) ^ (mrow & 15)) << 3) + (p & 7)] = hi;
    row[((((64 + p) >> 3) ^ (mrow & 15)) << 3) + (p & 7)] = lo;
  }
}

// ----------------------------------------------------------------------------------------------------- kv side in one launch
// phi(k) (the focused-ReLU kernel function, linattn.hip focus_row: same operations in the same order), kv^T = sum_j phi(k)_j^T v_j and
// the key sums of the 4 heads of one cloud, then the packed fp16 image of kv^T with the cloud's power-of-two scale -- what
// focus_k_kernel + kv_reduce_kernel + tb_kv_pack_kernel did in three launches (15 + 38 + 28 us at 64 clouds x 196 tokens).  One
// workgroup of 1024 threads per cloud: wave w stages key rows w, w + 16 of every 32-key tile (a wave = one 256-channel row: the focus
// norms are wave reductions), thread (head h = t >> 8, d = (t >> 2) & 63, c0 = 16 (t & 3)) owns kv^T[h][d][c0 .. c0 + 15] and
// accumulates over the keys in ascending order, exactly as kv_reduce_kernel does.
__device__ __forceinline__ float tbk_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// Round 3: one workgroup per (cloud, HEAD) instead of per cloud (64 workgroups of 1024 threads on 64 of the 256 CUs, 68 us): 256
// threads own kv^T[h][d][c0 .. c0 + 15] of their head, the four waves stage the 16 key rows of a step (a wave = one 256-channel row:
// the focus norms need the whole row, only the head's 64 k and 64 v channels go to LDS), every head gets its own power-of-two scale.
// Same phi(k), same per-output accumulation order: kv^T and the key sums keep their bits.
// Round 4: THREADS per (cloud, head) workgroup is a template parameter.  With 256 threads (round 3) a CU held four waves, one per SIMD,
// and a step's chain -- four rows of phi(k) per wave with two wave reductions each, then 16 keys x (LDS reads + 16 fma) per thread --
// ran without anything to overlap with: 56 us, unchanged by deeper row prefetch (58.7 us with a four-step register ring: not a load-
// latency problem).  1024 threads: one row per wave and step, four outputs per thread, sixteen waves per CU.  The accumulation order
// of every output (keys ascending) does not depend on the thread that owns it: same bits.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void tb_kv_fused_kernel(const float* __restrict__ kv, const float* __restrict__ scale, int J, long ld,
                                                              long sb, unsigned char* __restrict__ image, float* __restrict__ inv,
                                                              float* __restrict__ ksum) {
  constexpr int NW = THREADS / 64, RPW = 16 / NW;   // waves, key rows per wave and step
  constexpr int OPT = 4096 / THREADS, TPR = 64 / OPT;  // outputs per thread, threads per kv^T row
  __shared__ __attribute__((aligned(16))) float ks[16][64];
  __shared__ __attribute__((aligned(16))) float vs[16][68];
  __shared__ float red[NW];
  const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* kb = kv + (size_t)b * sb;
  const float4 sc = *reinterpret_cast<const float4*>(scale + lane * 4);
  const float sp[4] = {tbk_softplus(sc.x), tbk_softplus(sc.y), tbk_softplus(sc.z), tbk_softplus(sc.w)};
  const int d = t / TPR, c0 = (t % TPR) * OPT;
  const bool mine = (lane >> 4) == h;  // this lane's 4 channels belong to head h
  float acc[OPT];
#pragma unroll
  for (int u = 0; u < OPT; ++u) acc[u] = 0.f;
  float ksacc = 0.f;  // threads t < 64 accumulate ksum[h][c = t]
  // this wave's key rows of a step (rows wave, wave + NW, ...) in a register ring of NS steps: the rows of step i + NS - 1 are requested
  // before step i is accumulated.  (NS = 4 measured: 58.7 against 56.4 us at 256 threads, 41.1 against 41.3 us at 1024 -- the loop is
  // bound by the instructions it issues, ~130 per key row for phi(k) with its eight IEEE divisions and ~130 per step and wave for the
  // accumulation, not by the loads.)
  constexpr int NS = 2;
  float4 xr[NS][RPW], vr[NS][RPW];
  auto fetch = [&](float4 (&xq)[RPW], float4 (&vq)[RPW], int j0) {
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int j = j0 + NW * rr + wave;
      xq[rr] = vq[rr] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < J) {
        xq[rr] = *reinterpret_cast<const float4*>(kb + (size_t)j * ld + lane * 4);
        vq[rr] = *reinterpret_cast<const float4*>(kb + (size_t)j * ld + 256 + lane * 4);
      }
    }
  };
#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (st * 16 < J) fetch(xr[st], vr[st], st * 16);
  for (int jb = 0; jb < J; jb += NS * 16) {
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      const int j0 = jb + st * 16;
      if (j0 < J) {  // (uniform)
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
          const int jr = NW * rr + wave, j = j0 + jr;
          float4 kx = make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 vx = vr[st][rr];
          if (j < J) {
            const float4 x = xr[st][rr];
            float a[4] = {x.x, x.y, x.z, x.w}, c[4];
            float n1 = 0.f, n3 = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              float v = (a[u] > 0.f ? a[u] : 0.f) + 1e-6f;
              v = v / sp[u];
              n1 += v * v;
              c[u] = (v * v) * v;
              n3 += c[u] * c[u];
            }
            n1 = sqrtf(wave_sum_dpp(n1));
            n3 = sqrtf(wave_sum_dpp(n3));
            kx = make_float4((c[0] / n3) * n1, (c[1] / n3) * n1, (c[2] / n3) * n1, (c[3] / n3) * n1);
          }
          if (mine) {
            *reinterpret_cast<float4*>(&ks[jr][(lane & 15) * 4]) = kx;
            *reinterpret_cast<float4*>(&vs[jr][(lane & 15) * 4]) = vx;
          }
        }
        __syncthreads();
        if (j0 + (NS - 1) * 16 < J) fetch(xr[(st + NS - 1) % NS], vr[(st + NS - 1) % NS], j0 + (NS - 1) * 16);
#pragma unroll 4
        for (int jj = 0; jj < 16; ++jj) {
          const float vv = vs[jj][d];
#pragma unroll
          for (int u = 0; u < OPT; ++u) acc[u] = fmaf(ks[jj][c0 + u], vv, acc[u]);
          if (t < 64) ksacc += ks[jj][t];
        }
      }
    }
  }
  if (t < 64) ksum[((size_t)b * 4 + h) * 64 + t] = ksacc;
  // the head's scale from max |kv^T_h|
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < OPT; ++u) m = fmaxf(m, fabsf(acc[u]));
  m = wave_max_dpp(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float mm = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red[w]);
  const float s2 = pow2_scale(mm);
  if (t == 0) inv[(size_t)b * 4 + h] = 1.0f / s2;
  // image: head h, row d -> panel 2 h + (d >> 5), row m = d & 31; channel c sits in slot p = 32 (c >> 5) + 8 g + e of the 64-wide K
  // (tb_slot_channel inverted: g = (c >> 2) & 3, e = 4 ((c >> 4) & 1) + (c & 3))
  const int mrow = d & 31;
  _Float16* row = reinterpret_cast<_Float16*>(image + (size_t)b * (8 * TB_P64) + (size_t)(2 * h + (d >> 5)) * TB_P64 +
                                              (size_t)mrow * TB_ROWB(2));
#pragma unroll
  for (int u = 0; u < OPT; u += 2) {
    unsigned hi, lo;
    sam6d_split2_f16(acc[u] * s2, acc[u + 1] * s2, hi, lo);
    const _Float16 __attribute__((ext_vector_type(2))) h2 = __builtin_bit_cast(_Float16 __attribute__((ext_vector_type(2))), hi);
    const _Float16 __attribute__((ext_vector_type(2))) l2 = __builtin_bit_cast(_Float16 __attribute__((ext_vector_type(2))), lo);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int c = c0 + u + w, cc = c & 31;
      const int pslot = 32 * (c >> 5) + 8 * ((cc >> 2) & 3) + 4 * (cc >> 4) + (cc & 3);
      row[(((pslot >> 3) ^ (mrow & 15)) << 3) + (pslot & 7)] = h2[w];
      row[((((64 + pslot) >> 3) ^ (mrow & 15)) << 3) + (pslot & 7)] = l2[w];
    }
  }
}

extern "C" int sam6d_linattn_kv_image(const float* kv, const float* scale, int B, int J, long ld, long stride, void* image, float* inv,
                                      float* ksum, void* stream) {
  SAM6D_REQUIRE(kv && scale && image && inv && ksum && B >= 0 && B <= 65535 && J > 0 && ld >= 512 && (ld & 3) == 0 &&
                    (((size_t)kv | (size_t)scale) & 15) == 0,
                "linattn_kv_image: bad arguments (kv rows = 256 k | 256 v channels, 16-byte aligned)");
  if (B == 0) return 0;
  hipLaunchKernelGGL(tb_kv_fused_kernel<1024>, dim3(4, B), dim3(1024), 0, (hipStream_t)stream, kv, scale, J, ld, stride,
                     (unsigned char*)image, inv, ksum);
  SAM6D_LAUNCH_CHECK("linattn_kv_image");
}

extern "C" int sam6d_linattn_kv_pack(const float* kvT, int B, void* image, float* inv, void* stream) {
  SAM6D_REQUIRE(kvT && image && inv && B >= 0, "linattn_kv_pack: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(tb_kv_pack_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, kvT, (unsigned char*)image, inv);
  SAM6D_LAUNCH_CHECK("linattn_kv_pack");
}

extern "C" long sam6d_token_block_image_bytes(int mode) { return mode ? TB_IMAGE_BYTES(1) : TB_IMAGE_BYTES(0); }
extern "C" long sam6d_linattn_kv_image_bytes(void) { return 8 * TB_P64; }

// ------------------------------------------------------------------------------------------------------- the kernel
// one 32-row panel = two 16-row out tiles; KS k-steps of 32.  The weight fragments of step s+1 are requested before the six MFMAs
// of step s are issued (the eight waves run in lock-step between the panel barriers, so nothing else hides the LDS latency).  The
// reads and their counted waits are inline assembly: left to the compiler, the machine scheduler sinks every read to just before its
// use and waits with lgkmcnt(0) (measured: 2.7x the MFMA time per panel).
template <int OFF>
__device__ __forceinline__ u32x4 tb_lds128(unsigned addr) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
// wait until at most N LDS operations are outstanding; the fragments are in/out operands so that their uses stay behind the wait
template <int N>
__device__ __forceinline__ void tb_wait(u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
// chunk (16 B) index of (plane P, step S, lane group g) in a row: P * KS * 4 + 4 S + g; its low four bits are XORed with the row:
// the lane-dependent part ((4 q + g) ^ row) << 4 for q = 0..3 sits in four address registers, the rest is an immediate offset
template <int KS, int P, int S>
struct TbChunk {
  static constexpr int c = P * KS * 4 + 4 * S;     // + g (g < 4 never carries out of the low two bits)
  static constexpr int q = (c & 15) >> 2;
  static constexpr int off = (c & ~15) * 16;
};
template <int KS, int S>
__device__ __forceinline__ void tb_load_step(const unsigned (&a)[4], u32x4* f) {
  constexpr int R1 = 16 * TB_ROWB(KS);
  typedef TbChunk<KS, 0, S> H;
  typedef TbChunk<KS, 1, S> L;
  f[0] = tb_lds128<H::off>(a[H::q]);
  f[1] = tb_lds128<L::off>(a[L::q]);
  f[2] = tb_lds128<R1 + H::off>(a[H::q]);
  f[3] = tb_lds128<R1 + L::off>(a[L::q]);
}
// Fragment ring of TB_FD + 1 steps: the reads of step S + TB_FD are issued before the six MFMAs of step S (one step of MFMAs, 96
// cycles, does not cover the LDS latency when all eight waves of the CU stream b128 reads).
// Deeper rings were measured on the 197-token layers (round 3): two steps ahead within the same register budget 48.1 us against 48.3 us,
// three steps with a 4-slot panel ring and one wave per SIMD 52.5 us -- s_memtime stamps (scratch/tb_stamps.py) put a K = 256 panel at
// ~1420 cycles against 768 of MFMA issue with the waits for DMA and barrier at ~100 + ~160: the four waves of a workgroup each re-read
// the whole panel from LDS (64 LDS cycles per 96-cycle k-step), which a longer look-ahead does not change.
#define TB_FD 1
template <int KS, int S, int FD_>
__device__ __forceinline__ void tb_mma_step(f32x4& acc0, f32x4& acc1, const unsigned (&a)[4], const half8* __restrict__ xh,
                                            const half8* __restrict__ xl, u32x4 (&f)[FD_ + 1][4], bool half) {
  constexpr int cur = S % (FD_ + 1);
#ifndef TB_ABL_NOREAD  // (scratch/abl_build.sh: timing-only builds without the fragment reads / the panel DMA / the panel barrier)
  if constexpr (S + FD_ < KS) tb_load_step<KS, S + FD_>(a, f[(S + FD_) % (FD_ + 1)]);
#endif
  constexpr int newer = (KS - 1 - S) < FD_ ? (KS - 1 - S) : FD_;  // steps requested after this one
  tb_wait<4 * newer>(f[cur][0], f[cur][1], f[cur][2], f[cur][3]);
  const half8 h0 = __builtin_bit_cast(half8, f[cur][0]), l0 = __builtin_bit_cast(half8, f[cur][1]);
  const half8 h1 = __builtin_bit_cast(half8, f[cur][2]), l1 = __builtin_bit_cast(half8, f[cur][3]);
  if (!half) {  // (launch-uniform) matmul mode 2 keeps the hi . hi product only
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(l0, xh[S], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(l1, xh[S], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, xl[S], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, xl[S], acc1, 0, 0, 0);
  }
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, xh[S], acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, xh[S], acc1, 0, 0, 0);
  if constexpr (S + 1 < KS) tb_mma_step<KS, S + 1, FD_>(acc0, acc1, a, xh, xl, f, half);
}
// `panel`: LDS byte address of the panel; rows fr (first out tile) and fr + 16 (second)
template <int KS, int FD = TB_FD>
__device__ __forceinline__ void tb_mma(f32x4& acc0, f32x4& acc1, unsigned panel, const half8* __restrict__ xh,
                                       const half8* __restrict__ xl, int fr, int fg, bool half) {
  const unsigned rowbase = panel + fr * TB_ROWB(KS);
  const unsigned a[4] = {rowbase + (((0 + fg) ^ fr) << 4), rowbase + (((4 + fg) ^ fr) << 4), rowbase + (((8 + fg) ^ fr) << 4),
                         rowbase + (((12 + fg) ^ fr) << 4)};
  u32x4 f[FD + 1][4];
  tb_load_step<KS, 0>(a, f[0]);
  if constexpr (FD >= 2 && KS >= 2) tb_load_step<KS, 1>(a, f[1]);
  if constexpr (FD >= 3 && KS >= 3) tb_load_step<KS, 2>(a, f[2]);
  tb_mma_step<KS, 0, FD>(acc0, acc1, a, xh, xl, f, half);
}

// makes a register value opaque to the optimiser (no instruction): without it the compiler keeps the fp32 images of y's hi / lo
// halves, computed while splitting, alive across the whole FFN for the second residual (128 VGPRs -> scratch spills)
__device__ __forceinline__ void tb_opaque(half8& x) {
  u32x4 t = __builtin_bit_cast(u32x4, x);
  asm volatile("" : "+v"(t));
  x = __builtin_bit_cast(half8, t);
}

// split NT accumulator tiles (true units) into k-steps x{h,l}[t >> 1] (slot 4 (t & 1) + r); returns the row scale used
template <int NT>
__device__ __forceinline__ float tb_split_rows(const f32x4* v, half8* xh, half8* xl) {
  float m = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(v[t][r]));
  const float sc = pow2_scale(tok_max(m));
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; r += 2) sam6d_split2_f16(v[t][r] * sc, v[t][r + 1] * sc, xh[t >> 1], xl[t >> 1], 4 * (t & 1) + r);
  return sc;
}

// LayerNorm over the token's 256 channels, in place on 16 accumulator tiles; gamma / beta from LDS
__device__ __forceinline__ void tb_layernorm(f32x4* v, const float* __restrict__ g, const float* __restrict__ be, int fg, float eps) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) s += (v[t][0] + v[t][1]) + (v[t][2] + v[t][3]);
  const float mean = tok_sum(s) * (1.0f / 256.0f);
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[t][r] -= mean;
      q += v[t][r] * v[t][r];
    }
  const float rstd = 1.0f / sqrtf(tok_sum(q) * (1.0f / 256.0f) + eps);
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float4 gg = *reinterpret_cast<const float4*>(g + 16 * t + 4 * fg);
    const float4 bb = *reinterpret_cast<const float4*>(be + 16 * t + 4 * fg);
    v[t][0] = v[t][0] * rstd * gg.x + bb.x;
    v[t][1] = v[t][1] * rstd * gg.y + bb.y;
    v[t][2] = v[t][2] * rstd * gg.z + bb.z;
    v[t][3] = v[t][3] * rstd * gg.w + bb.w;
  }
}

struct TbArgs {
  const float* in;        // tail: hidden (M,256);   dense layer: D (B, I, 256)
  const float* resid;     // tail: x (M,256);        dense layer: unused (the residual is D)
  float* out;             // tail: (M,256);          dense layer: D' (B, I, 256)
  const unsigned char* wimg;
  const float* consts;
  const unsigned char* kvimg;  // dense layer: (B, 8 panels)
  const float* kvinv;          // dense layer: (B, 4) one inverse image scale per head
  const float* ksum;           // dense layer: (B, 256)
  long M;                 // tail: rows
  int I, row0, tiles_per_b;  // dense layer: rows per cloud, first row handled, tiles per cloud
  float eps;
  int half;               // 1: fp16 single product (matmul mode 2)
};

// The dense layer's panel sequence: proj_q x8 (K = 256), kv x8 (K = 64, the cloud's own image), linear x8 (K = 256), then per 128-wide FFN
// chunk expand x4 (K = 256) and squeeze x8 (K = 128).
struct TbSched {
  static constexpr int NPAN = 16 + 8 + 4 * 12;
  static constexpr int P0 = 16;  // first panel of the layer tail
  static constexpr bool kv(int i) { return i >= 8 && i < 16; }
  static constexpr int pieces(int i) {  // 1 KiB DMA pieces of panel i
    return kv(i) ? 8 : (i >= P0 + 8 && ((i - P0 - 8) % 12) >= 4) ? 16 : 32;
  }
  static constexpr size_t offset(int i) {  // of panel i in the weight image (kv panels: in the cloud's kv image)
    if (i < 8) return TB_Q_OFF + (size_t)i * TB_P256;
    if (i < P0) return (size_t)(i - 8) * TB_P64;
    if (i < P0 + 8) return (size_t)(i - P0) * TB_P256;
    const int c = (i - P0 - 8) / 12, u = (i - P0 - 8) % 12;
    return 8 * (size_t)TB_P256 + c * (size_t)TB_CHUNK_BYTES + (u < 4 ? u * (size_t)TB_P256 : 4 * (size_t)TB_P256 + (u - 4) * (size_t)TB_P128);
  }
};

#ifdef TB_STAMP  // diagnostic build only (scratch/stamp): per-wave s_memtime stamps around every panel's wait / barrier
#define TB_NSTAMP 256
__device__ unsigned long long tb_stamps[512 * 8 * TB_NSTAMP];
extern "C" int sam6d_tb_debug_stamps(void* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(tb_stamps), sizeof(unsigned long long) * 512 * 8 * TB_NSTAMP);
}
// (stamps go to LDS and are flushed at the end: a global store before a panel's s_waitcnt vmcnt would itself be waited for)
#define TB_ST(i) do { if (lane == 0 && wave < TB_WAVES && (i) < TB_NSTAMP) st_lds[wave][(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TB_ST(i)
#endif

// The dense layer: a workgroup = TB_WAVES waves x 16 tokens, the weight panels pass through a ring of TB_NBUF LDS slots; every wave
// issues its share of each panel's DMA.  (77 KB of LDS: two workgroups per CU, which run out of step, so one's row epilogues overlap
// the other's MFMAs.)
#define TB_WAVES 4
#define TB_NBUF 2
#define TB_LDS_BYTES (TB_NBUF * TB_PANEL_BYTES + (TC_N + 256) * 4)
static_assert(8 % TB_WAVES == 0, "every panel (8, 16 or 32 pieces) is dealt evenly to the waves");
__global__ __launch_bounds__(TB_WAVES * 64, 2) void token_block_kernel(TbArgs a) {  // (2 waves per SIMD: <= 256 VGPR + AGPR)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* pan = lds;                                                   // TB_NBUF panel slots
  float* cst = reinterpret_cast<float*>(lds + TB_NBUF * TB_PANEL_BYTES);      // TC_N floats
  float* ksm = cst + TC_N;                                                    // 256 floats
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const bool half = a.half != 0;
#ifdef TB_STAMP
  __shared__ unsigned long long st_lds[TB_WAVES][TB_NSTAMP];
  unsigned long long* st_base = tb_stamps + ((size_t)(blockIdx.x < 512 ? blockIdx.x : 0) * 8 + wave) * TB_NSTAMP;
#endif
  TB_ST(0);
  const unsigned pan_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)pan;

  // ---- which rows: this lane's token of its cloud (rows past the cloud's end recompute its last row and are not stored)
  const int b = blockIdx.x / a.tiles_per_b;
  const int tk = (blockIdx.x % a.tiles_per_b) * (16 * TB_WAVES) + wave * 16 + fr + a.row0;
  const bool valid = tk < a.I;
  const long row = (long)b * a.I + (valid ? tk : a.I - 1);

  const unsigned char* kvp = a.kvimg + (size_t)b * (8 * TB_P64);
  // LDS-DMA of panel I into its ring slot, dealt to the waves (the global image IS the LDS image)
  auto dma = [&](auto IC) {
    constexpr int I = decltype(IC)::value;
    if constexpr (I < TbSched::NPAN)
      dma_pieces<TbSched::pieces(I) / TB_WAVES>((TbSched::kv(I) ? kvp : a.wimg) + TbSched::offset(I), pan + (I % TB_NBUF) * TB_PANEL_BYTES, wave,
                                                TB_WAVES, lane);
  };
  // Start of panel I: with two slots, panel I is the only DMA in flight (panel I + 1 goes out below, after the barrier), so
  // vmcnt(0) is exactly "this wave's pieces of panel I have landed".  The barrier then publishes the panel to the other waves and at the
  // same time retires panel I - 1 in every wave, whose ring slot the DMA of panel I + 1 overwrites.
  static_assert(TB_NBUF == 2, "a deeper ring needs counted waits");
  auto next_panel = [&](auto IC) -> unsigned {
    constexpr int I = decltype(IC)::value;
    TB_ST(4 + 3 * I);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TB_ST(5 + 3 * I);
#ifndef TB_ABL_NOBAR
    __syncthreads();
#endif
    TB_ST(6 + 3 * I);
#ifndef TB_ABL_NODMA
    dma(std::integral_constant<int, I + 1>{});
#endif
    return pan_lds + (I % TB_NBUF) * TB_PANEL_BYTES;
  };

  dma(std::integral_constant<int, 0>{});
  for (int i = t; i < TC_N; i += TB_WAVES * 64) cst[i] = a.consts[i];
  if (t < 256) ksm[t] = a.ksum[(size_t)b * 256 + t];

  // ---- X: the input rows D, split
  // the dense layer streams 134 MB of tokens in and out once: non-temporal, so that they do not evict the weight / kv images that
  // 2048 workgroups re-read from the L2 (FETCH_SIZE: 237 MB for 140 MB of compulsory reads with ordinary loads)
  half8 xh[8], xl[8];
  float sx = split_row256<true>(a.in + (size_t)row * 256, fg, xh, xl);

  // the split input rows D stay in registers for the residual add three products later (re-reading them cost a second
  // 134 MB pass over D per layer: 1.7x the layer's algorithmic traffic, rocprof FETCH_SIZE)
  half8 dh[8], dl[8];
  const float sd = sx;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    dh[s] = xh[s];
    dl[s] = xl[s];
    tb_opaque(dh[s]);
    tb_opaque(dl[s]);
  }

  TB_ST(1);
  f32x4 acc[16];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  constexpr int P0 = TbSched::P0;
  // ---- q = D Wq^T + b, focus, z
  zero_acc();
  static_for<0, 8>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const unsigned p = next_panel(std::integral_constant<int, j>{});
    tb_mma<8>(acc[2 * j], acc[2 * j + 1], p, xh, xl, fr, fg, half);
  });
  {
    const float inv = cst[TC_SC + 0] * (1.0f / sx);
    float n1 = 0.f, n3 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 bq = *reinterpret_cast<const float4*>(cst + TC_BQ + 16 * i + 4 * fg);
      const float4 is = *reinterpret_cast<const float4*>(cst + TC_ISP + 16 * i + 4 * fg);
      const float bb[4] = {bq.x, bq.y, bq.z, bq.w}, ii[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v = acc[i][u] * inv + bb[u];
        v = ((v > 0.f ? v : 0.f) + 1e-6f) * ii[u];
        n1 += v * v;
        const float c3 = (v * v) * v;
        n3 += c3 * c3;
        acc[i][u] = c3;
      }
    }
    const float f = sqrtf(tok_sum(n1)) / sqrtf(tok_sum(n3));  // phi = c3 / |c3| * |v|
#pragma unroll
    for (int hd = 0; hd < 4; ++hd) {
      float dot = 0.f;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int i = 4 * hd + ii;
        const float4 ks = *reinterpret_cast<const float4*>(ksm + 16 * i + 4 * fg);
        acc[i][0] *= f; acc[i][1] *= f; acc[i][2] *= f; acc[i][3] *= f;
        dot += (acc[i][0] * ks.x + acc[i][1] * ks.y) + (acc[i][2] * ks.z + acc[i][3] * ks.w);
      }
      const float z = 1.0f / (tok_sum(dot) + 1e-6f);
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        acc[4 * hd + ii][0] *= z; acc[4 * hd + ii][1] *= z; acc[4 * hd + ii][2] *= z; acc[4 * hd + ii][3] *= z;
      }
    }
    sx = tb_split_rows<16>(acc, xh, xl);
  }
  // ---- hidden_h = phi(q)_h kv_h  (K = 64 per head: k-steps 2h, 2h+1)
  zero_acc();
  static_for<0, 8>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const unsigned p = next_panel(std::integral_constant<int, 8 + j>{});
    tb_mma<2>(acc[2 * j], acc[2 * j + 1], p, xh + 2 * (j >> 1), xl + 2 * (j >> 1), fr, fg, half);
  });
  {
    const float4 kvi = *reinterpret_cast<const float4*>(a.kvinv + (size_t)b * 4);  // the four heads' image scales
    const float isx = 1.0f / sx;
    const float invh[4] = {kvi.x * isx, kvi.y * isx, kvi.z * isx, kvi.w * isx};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float inv = invh[i >> 2];  // accumulator tiles 4 h .. 4 h + 3 hold head h's 64 channels
      acc[i][0] *= inv; acc[i][1] *= inv; acc[i][2] *= inv; acc[i][3] *= inv;
    }
    sx = tb_split_rows<16>(acc, xh, xl);
  }

  // ---- y = LayerNorm(hidden Wlin^T + b + residual)
  zero_acc();
  static_for<0, 8>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const unsigned p = next_panel(std::integral_constant<int, P0 + j>{});
    tb_mma<8>(acc[2 * j], acc[2 * j + 1], p, xh, xl, fr, fg, half);
  });
  {
    const float inv = cst[TC_SC + 1] * (1.0f / sx);
    const float isd = 1.0f / sd;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float4 rv;  // D = (hi + lo) / scale: 22 significand bits of the fp32 input
      rv.x = ((float)dh[i >> 1][4 * (i & 1) + 0] + (float)dl[i >> 1][4 * (i & 1) + 0]) * isd;
      rv.y = ((float)dh[i >> 1][4 * (i & 1) + 1] + (float)dl[i >> 1][4 * (i & 1) + 1]) * isd;
      rv.z = ((float)dh[i >> 1][4 * (i & 1) + 2] + (float)dl[i >> 1][4 * (i & 1) + 2]) * isd;
      rv.w = ((float)dh[i >> 1][4 * (i & 1) + 3] + (float)dl[i >> 1][4 * (i & 1) + 3]) * isd;
      const float4 bl = *reinterpret_cast<const float4*>(cst + TC_BLIN + 16 * i + 4 * fg);
      acc[i][0] = (acc[i][0] * inv + bl.x) + rv.x;
      acc[i][1] = (acc[i][1] * inv + bl.y) + rv.y;
      acc[i][2] = (acc[i][2] * inv + bl.z) + rv.z;
      acc[i][3] = (acc[i][3] * inv + bl.w) + rv.w;
    }
    tb_layernorm(acc, cst + TC_G1, cst + TC_BE1, fg, a.eps);
    sx = tb_split_rows<16>(acc, xh, xl);  // y, kept as hi + lo for the second residual
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      tb_opaque(xh[s]);
      tb_opaque(xl[s]);
    }
  }
  const float sy = sx;

  // ---- out = relu(y Wexp^T + b) Wsq^T, the 512 hidden channels in 4 chunks of 128 that never leave the registers
  zero_acc();
  {
    const float inv_e = cst[TC_SC + 2] * (1.0f / sy), sh = cst[TC_SC + 4];
    static_for<0, 4>([&](auto CC) {
      constexpr int c = decltype(CC)::value;
      half8 hh[4], hl[4];
      static_for<0, 4>([&](auto U) {
        constexpr int u = decltype(U)::value;
        const unsigned p = next_panel(std::integral_constant<int, P0 + 8 + 12 * c + u>{});
        f32x4 ha[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        tb_mma<8>(ha[0], ha[1], p, xh, xl, fr, fg, half);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          const float4 be = *reinterpret_cast<const float4*>(cst + TC_BEXP + 128 * c + 32 * u + 16 * w + 4 * fg);
          const float bb[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
          for (int r = 0; r < 4; r += 2) {
            float v0 = ha[w][r] * inv_e + bb[r], v1 = ha[w][r + 1] * inv_e + bb[r + 1];
            v0 = (v0 > 0.f ? v0 : 0.f) * sh;
            v1 = (v1 > 0.f ? v1 : 0.f) * sh;
            sam6d_split2_f16(v0, v1, hh[u], hl[u], 4 * w + r);
          }
        }
      });
      static_for<0, 8>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const unsigned p = next_panel(std::integral_constant<int, P0 + 8 + 12 * c + 4 + j>{});
        tb_mma<4>(acc[2 * j], acc[2 * j + 1], p, hh, hl, fr, fg, half);
      });
    });
  }
  {
    const float inv = cst[TC_SC + 3], isy = 1.0f / sy;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 bs = *reinterpret_cast<const float4*>(cst + TC_BSQ + 16 * i + 4 * fg);
      const float bb[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = ((float)xh[i >> 1][4 * (i & 1) + r] + (float)xl[i >> 1][4 * (i & 1) + r]) * isy;
        acc[i][r] = (acc[i][r] * inv + bb[r]) + y;
      }
    }
    tb_layernorm(acc, cst + TC_G2, cst + TC_BE2, fg, a.eps);
  }
  TB_ST(2);
  if (valid) {
    float* o = a.out + (size_t)row * 256;
#pragma unroll
    for (int i = 0; i < 16; ++i) __builtin_nontemporal_store(acc[i], reinterpret_cast<f32x4*>(o + 16 * i + 4 * fg));
  }
  TB_ST(3);
#ifdef TB_STAMP
  if (blockIdx.x < 512)
    for (int i = lane; i < TB_NSTAMP; i += 64) st_base[i] = st_lds[wave][i];
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// The layer tail (mode 0) of the 197-token layers: output channels dealt to eight waves per tile.
//
// token_block_kernel gives a wave 16 tokens and ALL output channels: a launch takes one wave's serial chain of 1920 MFMAs + every row
// epilogue on 64 values per lane, behind 56 weight panels that go L2 -> LDS ring -> fragment reads with a workgroup barrier per step,
// whatever the number of workgroups -- and these launches have one small workgroup per CU.  Here a workgroup of eight waves (two per
// SIMD) owns TT x 16 tokens and wave w computes ALL tokens of the tile for its own 1/8 of the output channels of every product:
//     lin:  out channels 32 w .. 32 w + 31                       = panel w of the linear part            (K = 256)
//     exp:  hidden channels 32 e .. 32 e + 31, e = 8 hf + w      = expand panel e & 3 of chunk e >> 2    (K = 256; hf = 0, 1: two halves)
//     sq:   out channels 32 w .. 32 w + 31 over all 512 hidden   = squeeze panel w of the chunks 0 .. 3  (4 x K = 128, ascending)
//   * weights never touch LDS: a wave reads the A fragments of its own 32 rows from the packed image (the XOR-swizzled panels of
//     tb_pack_kernel, unchanged) straight into a register ring D k-steps ahead of the MFMAs; the ring runs on across the epilogues and
//     barriers (one stream of 40 k-steps per wave).  Per load instruction a row's four chunks are one aligned 64-byte segment, and the
//     k-steps 2 j, 2 j + 1 share their 128-byte lines.
//   * activations live in LDS as fp16 hi / lo in B-fragment order -- block (k-step, plane, token tile) = 1 KiB, lane l's 16 bytes at
//     16 l, so that writes and ds_read_b128 are linear -- written once by the epilogue that produces them (wave w's 32 channels ARE
//     k-step w of the next product), read by all eight waves: y 16 KiB per token tile, and one buffer of the same size that holds the
//     split input rows and then the two 256-wide halves of the FFN hidden row.
//   * a row statistic that needs all 256 channels is exchanged through LDS: per-wave partials red[w][token], one barrier, every lane
//     sums the eight partials in WAVE ORDER.  Five exchanges (LayerNorm mean / variance twice, the row maximum that fixes y's split
//     scale) + five publishing barriers = ten barriers per launch instead of 28 ring steps.  The hidden row keeps its pack-time scale.
// A token is one MFMA column: its result depends on its own row only -- not on M, its place in the tile, TT or its neighbours.
// Same arithmetic class as token_block_kernel (fp16 x3, fp32 accumulate, power-of-two scales undone exactly); the second residual adds
// y rebuilt from its hi + lo halves.
template <int G>
struct TtStep {  // k-step G (0 .. 39) of a wave's weight stream
  static constexpr bool sq = (G >= 16 && G < 24) || G >= 32;
  static constexpr int KS = sq ? 4 : 8;
  static constexpr int S = sq ? (G & 3) : (G & 7);                 // k-step inside its panel
  static constexpr int P = G < 8 ? 0 : G < 16 ? 1 : G < 24 ? 3 + ((G - 16) >> 2) : G < 32 ? 2 : 5 + ((G - 32) >> 2);  // pointer index
};
#define TT_NSTEP 40
#define TT_D2 6  // k-steps of weight fragments in flight: 32-token tiles
#define TT_D4 3  //                                          64-token tiles (4: 246 registers, 34.3 against 34.0 us -- no gain)
#define TT_LDS_BYTES(TT) ((TT) * (32768 + 25 * 16 * 4))

template <int TT, int D, bool HALF>
__global__ __launch_bounds__(512) void token_tail_kernel(TbArgs a) {
  constexpr int NTOK = 16 * TT, ACT = TT * 16384, RPW = NTOK / 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* yb = lds;                                  // y
  unsigned char* hb = lds + ACT;                            // the split input rows, then the hidden row's halves
  float* red = reinterpret_cast<float*>(lds + 2 * ACT);     // [3][8][NTOK] partial row statistics
  float* sxs = red + 3 * 8 * NTOK;                          // [NTOK] split scale of the input rows
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const long tile0 = (long)blockIdx.x * NTOK;
  const float* cst = a.consts;
  // LDS addresses as one lane-dependent base + immediate offsets; the bases are made opaque, or the compiler rebuilds every address of
  // the unrolled stream in a register of its own (and spills them)
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  typedef __attribute__((address_space(3))) float lds_f32;
  typedef __attribute__((address_space(3))) half8 lds_h8;
  typedef __attribute__((address_space(3))) u32x4 lds_u4;
  lds_u8* ybl = (lds_u8*)yb + lane * 16;
  lds_u8* hbl = (lds_u8*)hb + lane * 16;
  lds_f32* redl = (lds_f32*)red + fr;
  asm volatile("" : "+v"(ybl), "+v"(hbl), "+v"(redl));
  auto row_of = [&](int tok) -> long { return tile0 + tok < a.M ? tile0 + tok : a.M - 1; };

  // ---- requests first: this wave's input rows (whole rows: the row maximum needs no exchange) and its residual slices
  float4 xv[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) xv[i] = *reinterpret_cast<const float4*>(a.in + (size_t)row_of(wave * RPW + i) * 256 + lane * 4);
  f32x4 rv[TT][2];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      rv[tt][rt] = *reinterpret_cast<const f32x4*>(a.resid + (size_t)row_of(16 * tt + fr) * 256 + 32 * wave + 16 * rt + 4 * fg);

  // ---- the weight stream: pointers of this wave's panels, the lane part of a fragment address (see TbChunk), a ring of D + 1 k-steps
  // (buffer loads: one descriptor over the image, the panel in the scalar offset, the lane part in the 32-bit vector offset -- and a
  // fragment address outside the image would read zeros instead of faulting)
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.wimg), 0, TB_IMAGE_BYTES(0), 0x00020000);
  constexpr unsigned chunk0 = 8 * TB_P256;
  const unsigned wp[7] = {(unsigned)wave * TB_P256,
                          chunk0 + (unsigned)(wave >> 2) * TB_CHUNK_BYTES + (unsigned)(wave & 3) * TB_P256,
                          chunk0 + (unsigned)(2 + (wave >> 2)) * TB_CHUNK_BYTES + (unsigned)(wave & 3) * TB_P256,
                          chunk0 + 0 * TB_CHUNK_BYTES + 4 * TB_P256 + (unsigned)wave * TB_P128,
                          chunk0 + 1 * TB_CHUNK_BYTES + 4 * TB_P256 + (unsigned)wave * TB_P128,
                          chunk0 + 2 * TB_CHUNK_BYTES + 4 * TB_P256 + (unsigned)wave * TB_P128,
                          chunk0 + 3 * TB_CHUNK_BYTES + 4 * TB_P256 + (unsigned)wave * TB_P128};
  unsigned o8[4], o4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    o8[q] = fr * TB_ROWB(8) + (((4 * q + fg) ^ fr) << 4);
    o4[q] = fr * TB_ROWB(4) + (((4 * q + fg) ^ fr) << 4);
  }
  u32x4 ar[D + 1][4];
  auto wload = [&](auto GC) {
    constexpr int G = decltype(GC)::value;
    if constexpr (G < TT_NSTEP) {
      typedef TtStep<G> ST;
      typedef TbChunk<ST::KS, 0, ST::S> H;
      typedef TbChunk<ST::KS, 1, ST::S> L;
      constexpr int R1 = 16 * TB_ROWB(ST::KS);
      const unsigned o = ST::KS == 8 ? o8[H::q] : o4[H::q];
      u32x4* f = ar[G % (D + 1)];
      f[0] = __builtin_amdgcn_raw_buffer_load_b128(wr, o + H::off, wp[ST::P], 0);
      f[1] = __builtin_amdgcn_raw_buffer_load_b128(wr, o + L::off, wp[ST::P], 0);
      f[2] = __builtin_amdgcn_raw_buffer_load_b128(wr, o + H::off, wp[ST::P] + R1, 0);
      f[3] = __builtin_amdgcn_raw_buffer_load_b128(wr, o + L::off, wp[ST::P] + R1, 0);
    }
  };
  static_for<0, D>([&](auto GC) { wload(GC); });

  // NS k-steps starting at stream step G0: acc[rt][tt] += W(rows 16 rt ..) . B(token tile tt); B fragments one step ahead
  auto product = [&](auto G0C, auto NSC, f32x4 (&acc)[2][TT], const lds_u8* bbase) {
    constexpr int G0 = decltype(G0C)::value, NS = decltype(NSC)::value;
    half8 bq[2][TT][2];
    auto bload = [&](int s, half8 (&b)[TT][2]) {
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        b[tt][0] = *reinterpret_cast<const lds_h8*>(bbase + ((s * 2 + 0) * TT + tt) * 1024);
        b[tt][1] = *reinterpret_cast<const lds_h8*>(bbase + ((s * 2 + 1) * TT + tt) * 1024);
      }
    };
    bload(0, bq[0]);
    static_for<0, NS>([&](auto SC) {
      constexpr int S = decltype(SC)::value, G = G0 + S;
      wload(std::integral_constant<int, G + D>{});
      if constexpr (S + 1 < NS) bload(S + 1, bq[(S + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      const u32x4* f = ar[G % (D + 1)];
      const half8 ah[2] = {__builtin_bit_cast(half8, f[0]), __builtin_bit_cast(half8, f[2])};
      const half8 al[2] = {__builtin_bit_cast(half8, f[1]), __builtin_bit_cast(half8, f[3])};
      const half8(&b)[TT][2] = bq[S & 1];
      if constexpr (!HALF) {  // matmul mode 2 keeps the hi . hi product only
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int tt = 0; tt < TT; ++tt) acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt], b[tt][0], acc[rt][tt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int tt = 0; tt < TT; ++tt) acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], b[tt][1], acc[rt][tt], 0, 0, 0);
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], b[tt][0], acc[rt][tt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  auto zero = [&](f32x4 (&acc)[2][TT]) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) acc[rt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // row statistics over all channels: this wave's partial per token (in p) -> the total, the eight partials combined in wave order
  auto xsum = [&](float (&p)[TT], int k) {  // k: which of the three buffers
    lds_f32* buf = redl + k * 8 * NTOK;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const float s = tok_sum(p[tt]);
      if (fg == 0) buf[wave * NTOK + 16 * tt] = s;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      float s = buf[16 * tt];
#pragma unroll
      for (int w = 1; w < 8; ++w) s += buf[w * NTOK + 16 * tt];
      p[tt] = s;
    }
  };
  auto xmax = [&](float (&p)[TT], int k) {
    lds_f32* buf = redl + k * 8 * NTOK;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const float s = tok_max(p[tt]);
      if (fg == 0) buf[wave * NTOK + 16 * tt] = s;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      float s = buf[16 * tt];
#pragma unroll
      for (int w = 1; w < 8; ++w) s = fmaxf(s, buf[w * NTOK + 16 * tt]);
      p[tt] = s;
    }
  };
  // LayerNorm of v (this wave's 32 channels of every token) over the token's 256 channels
  auto layernorm = [&](f32x4 (&v)[2][TT], int goff, int boff) {
    float s[TT], q[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
      s[tt] = ((v[0][tt][0] + v[0][tt][1]) + (v[0][tt][2] + v[0][tt][3])) + ((v[1][tt][0] + v[1][tt][1]) + (v[1][tt][2] + v[1][tt][3]));
    xsum(s, 0);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const float mean = s[tt] * (1.0f / 256.0f);
      q[tt] = 0.f;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[rt][tt][r] -= mean;
          q[tt] += v[rt][tt][r] * v[rt][tt][r];
        }
    }
    xsum(q, 1);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const float4 gg = *reinterpret_cast<const float4*>(cst + goff + 32 * wave + 16 * rt + 4 * fg);
      const float4 bb = *reinterpret_cast<const float4*>(cst + boff + 32 * wave + 16 * rt + 4 * fg);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const float rstd = 1.0f / sqrtf(q[tt] * (1.0f / 256.0f) + a.eps);
        v[rt][tt][0] = v[rt][tt][0] * rstd * gg.x + bb.x;
        v[rt][tt][1] = v[rt][tt][1] * rstd * gg.y + bb.y;
        v[rt][tt][2] = v[rt][tt][2] * rstd * gg.z + bb.z;
        v[rt][tt][3] = v[rt][tt][3] * rstd * gg.w + bb.w;
      }
    }
  };
  // this wave's 32 channels of token tile tt (already scaled) -> k-step `ks` of an activation buffer
  auto put = [&](lds_u8* buf, int ks, int tt, const f32x4& v0, const f32x4& v1) {
    unsigned h0, l0, h1, l1, h2, l2, h3, l3;
    sam6d_split2_f16(v0[0], v0[1], h0, l0);
    sam6d_split2_f16(v0[2], v0[3], h1, l1);
    sam6d_split2_f16(v1[0], v1[1], h2, l2);
    sam6d_split2_f16(v1[2], v1[3], h3, l3);
    *reinterpret_cast<lds_u4*>(buf + ((ks * 2 + 0) * TT + tt) * 1024) = u32x4{h0, h1, h2, h3};
    *reinterpret_cast<lds_u4*>(buf + ((ks * 2 + 1) * TT + tt) * 1024) = u32x4{l0, l1, l2, l3};
  };

  // ---- the input rows, split: lane l holds channels 4 l .. 4 l + 3 = k-step l >> 3, lane group l & 3, slots 4 ((l >> 2) & 1) ..
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int tok = wave * RPW + i;
    const float m = wave_max_dpp(amax4(xv[i]));
    const float sx = pow2_scale(m);
    if (lane == 0) sxs[tok] = sx;
    unsigned h0, l0, h1, l1;
    sam6d_split2_f16(xv[i].x * sx, xv[i].y * sx, h0, l0);
    sam6d_split2_f16(xv[i].z * sx, xv[i].w * sx, h1, l1);
    unsigned char* dst = hb + (size_t)(tok >> 4) * 1024 + ((lane & 3) * 16 + (tok & 15)) * 16 + 8 * ((lane >> 2) & 1);
    *reinterpret_cast<u32x2*>(dst + ((lane >> 3) * 2 + 0) * TT * 1024) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(dst + ((lane >> 3) * 2 + 1) * TT * 1024) = u32x2{l0, l1};
  }
  __syncthreads();

  // ---- y = LayerNorm(hidden Wlin^T + b + x)
  float sy[TT];
  {
    f32x4 y[2][TT];
    zero(y);
    product(std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{}, y, hbl);
    const float iw = cst[TC_SC + 1];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const float4 bl = *reinterpret_cast<const float4*>(cst + TC_BLIN + 32 * wave + 16 * rt + 4 * fg);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const float inv = iw * (1.0f / sxs[16 * tt + fr]);
        y[rt][tt][0] = (y[rt][tt][0] * inv + bl.x) + rv[tt][rt][0];
        y[rt][tt][1] = (y[rt][tt][1] * inv + bl.y) + rv[tt][rt][1];
        y[rt][tt][2] = (y[rt][tt][2] * inv + bl.z) + rv[tt][rt][2];
        y[rt][tt][3] = (y[rt][tt][3] * inv + bl.w) + rv[tt][rt][3];
      }
    }
    layernorm(y, TC_G1, TC_BE1);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      float m = 0.f;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(y[rt][tt][r]));
      sy[tt] = m;
    }
    xmax(sy, 2);
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const float sc = sy[tt] = pow2_scale(sy[tt]);
      put(ybl, wave, tt, f32x4{y[0][tt][0] * sc, y[0][tt][1] * sc, y[0][tt][2] * sc, y[0][tt][3] * sc},
          f32x4{y[1][tt][0] * sc, y[1][tt][1] * sc, y[1][tt][2] * sc, y[1][tt][3] * sc});
    }
    __syncthreads();
  }

  // ---- out = LayerNorm(relu(y Wexp^T + b) Wsq^T + b + y), the hidden row in two halves of 256 channels
  f32x4 acc[2][TT];
  zero(acc);
  static_for<0, 2>([&](auto HC) {
    constexpr int hf = decltype(HC)::value;
    f32x4 ha[2][TT];
    zero(ha);
    product(std::integral_constant<int, 8 + 16 * hf>{}, std::integral_constant<int, 8>{}, ha, ybl);
    const float ie = cst[TC_SC + 2], sh = cst[TC_SC + 4];
    if constexpr (hf == 1) __syncthreads();  // every wave has left the first half of the hidden row
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      const float inv = ie * (1.0f / sy[tt]);
      f32x4 hv[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const float4 be = *reinterpret_cast<const float4*>(cst + TC_BEXP + 32 * (8 * hf + wave) + 16 * rt + 4 * fg);
        const float bb[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = ha[rt][tt][r] * inv + bb[r];
          hv[rt][r] = (v > 0.f ? v : 0.f) * sh;
        }
      }
      put(hbl, wave, tt, hv[0], hv[1]);
    }
    __syncthreads();
    product(std::integral_constant<int, 16 + 16 * hf>{}, std::integral_constant<int, 8>{}, acc, hbl);
  });
  {
    const float inv = cst[TC_SC + 3];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const float4 bs = *reinterpret_cast<const float4*>(cst + TC_BSQ + 32 * wave + 16 * rt + 4 * fg);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        // y = (hi + lo) / scale, read back from this lane's own fragment chunk (22 significand bits, as in token_block_kernel)
        const half8 yh = *reinterpret_cast<const lds_h8*>(ybl + ((wave * 2 + 0) * TT + tt) * 1024);
        const half8 yl = *reinterpret_cast<const lds_h8*>(ybl + ((wave * 2 + 1) * TT + tt) * 1024);
        const float isy = 1.0f / sy[tt];
        const float bb[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][tt][r] = (acc[rt][tt][r] * inv + bb[r]) + ((float)yh[4 * rt + r] + (float)yl[4 * rt + r]) * isy;
      }
    }
    layernorm(acc, TC_G2, TC_BE2);
  }
#pragma unroll
  for (int tt = 0; tt < TT; ++tt)
    if (tile0 + 16 * tt + fr < a.M) {
      float* o = a.out + (size_t)(tile0 + 16 * tt + fr) * 256 + 32 * wave + 4 * fg;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
        *reinterpret_cast<float4*>(o + 16 * rt) = make_float4(acc[rt][tt][0], acc[rt][tt][1], acc[rt][tt][2], acc[rt][tt][3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Measured and removed, round 4: the layer tail with the FFN split over TWO waves per 16-token group.  The primary
// wave of a group ran linear + residual + LayerNorm and handed the normalised row (fp16 hi / lo fragments, 16 KB per group) to a
// secondary wave through LDS; primary and secondary then ran the hidden chunks {0, 1} and {2, 3} at once (a 64 KB ring slot held one
// panel pair of either role, 20 steps instead of 56 panels per chain), and the secondary's partial squeeze accumulators came back
// through LDS for the second residual + LayerNorm: two LDS exchanges per layer (round 3's rejected form split every product and needed
// seven), primary and secondary of a group on one SIMD so that one's row epilogues sit under the other's MFMAs.  232 VGPRs, no spills,
// all 63 tests of tests/test_block_gpu.py green (the hidden chunks summed as (0 + 1) + (2 + 3)).  Times (scratch/run_block.py, one box,
// us per launch): 12608 rows 43.7 against 40.7 for token_block_kernel, 6304 rows 39.7 against 34.0 (the 32-token shape below).
// Why it does not pay: the chain is bound by the LDS, not by the serial epilogues.  Every 16-token wave reads each weight panel from
// LDS whole -- 2 KB of fragments per three MFMAs, i.e. 43 B / clk per wave at the full MFMA rate, 171 B / clk for four waves beside the
// ring's DMA writes, against the ~130-150 B / clk a CU delivers in practice -- so a K = 256 panel takes ~1420 cycles for 768 cycles of
// MFMA issue, and eight computing waves per workgroup double the reads per step while the two roles' panel pairs double the DMA bytes
// in flight: a step of the split kernel took ~3 000 cycles.  Fewer LDS bytes per MFMA would need 32-token waves on v_mfma_f32_32x32x16
// (twice the flops per fragment byte), whose operands + accumulators (128 + 128 registers before the FFN hidden chunks) only fit one
// wave per SIMD and leave half of the SIMDs without a wave at 49 tokens per CU -- priced at 36 us per launch, not built.
// What did help: two computing waves per workgroup where the rows still fill the chip (sam6d_token_block below).
// ---------------------------------------------------------------------------------------------------------------------
// Front of the RPE self-attention layer (RPEMultiHeadAttention.forward, PEM/model/transformer.py:395-405, with proj_p folded into the
// query as attention.hip / rpe.hip describe): one launch instead of three GEMMs
//     qkv = x Wqkv^T + b          (M, 768)   written (q | k | v)
//     qp[n, h, :] = Wp_h^T q_h    (M, 4, 256) the query folded through proj_p, per head (K = 64)
//     qd[n, h, :] = D_c^T qp_h    (M*4, 32)   Chebyshev coefficients of proj_d applied to the folded query
// Same register-chained transposed scheme as token_block_kernel: q stays in the accumulators, becomes the B operand of the proj_p
// fold, whose output becomes the B operand of the D_c product.  Always fp16 x3 (these are the "geometry" folds of matmul mode 2).
// Image: qkv 24 panels (K = 256) | per head 8 panels of Wp_h^T (K = 64) | D_c^T 1 panel (K = 256).
#define RF_IMAGE_BYTES (24 * TB_P256 + 32 * TB_P64 + TB_P256)
struct RfArgs {
  const float* x;            // (M, 256)
  const unsigned char* wimg;
  const float* bias;         // (768)
  float* qkv;                // (M, 768)
  float* qp;                 // (M, 1024)
  float* qd;                 // (M * 4, 32)
  long M;
  float inv_qkv, inv_wp, inv_dc;
  float* vT;                 // optional: (M / n clouds, 256, ldp) the values transposed per cloud (the W operand of the P.v GEMM);
  int n, ldp;                //   then the v third of qkv is not written
};

// VT: the values go to vT (8 scattered 4-byte stores per value panel) instead of the v third of qkv (2 float4 stores).
// Stores are issued for every lane: rows past M are clamped to row M - 1 and rewrite its values.
// Four loader waves beside the four computing ones issue the panel DMA, as in token_block_kernel; the computing waves then never wait on
// the vector-memory counter (their stores stay in flight across panels).
template <bool VT>
__global__ __launch_bounds__(512, 1) void rpe_front_kernel(RfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* pan = lds;  // 2 x TB_PANEL_BYTES
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const unsigned pan_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)pan;
  const long r0 = (long)blockIdx.x * 64 + wave * 16 + fr;
  const bool valid = r0 < a.M;
  const long row = valid ? r0 : a.M - 1;
  constexpr int NPAN = 24 + 4 * 3;
  // LDS-DMA unit i (32 KiB each): 0..23 the qkv panels (K256); then per head h: two groups of four Wp_h^T panels (K64, 8 KiB each,
  // contiguous in the image: one barrier per group instead of one per panel), then the D_c^T panel (K256)
  auto dma = [&](auto IC) {
    constexpr int I = decltype(IC)::value;
    if constexpr (I < NPAN) {
      constexpr size_t off = I < 24 ? (size_t)I * TB_P256
                                    : (((I - 24) % 3) == 2 ? 24 * (size_t)TB_P256 + 32 * (size_t)TB_P64
                                                           : 24 * (size_t)TB_P256 + (size_t)(((I - 24) / 3) * 8 + ((I - 24) % 3) * 4) * TB_P64);
      dma_pieces<32 / 4>(a.wimg + off, pan + (I & 1) * TB_PANEL_BYTES, wave - 4, 4, lane);
    }
  };
  // the computing waves' side of the loader waves' barrier of unit I
  auto next_panel = [&](auto IC) -> unsigned {
    constexpr int I = decltype(IC)::value;
    __syncthreads();
    return pan_lds + (I & 1) * TB_PANEL_BYTES;
  };
  if (wave >= 4) {  // a loader wave: unit I + 1 goes out once unit I has landed and every wave has left unit I - 1
    dma(std::integral_constant<int, 0>{});
    static_for<0, NPAN>([&](auto IC) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      dma(std::integral_constant<int, decltype(IC)::value + 1>{});
    });
    return;
  }

  half8 xh[8], xl[8];
  const float sx = split_row256<false>(a.x + (size_t)row * 256, fg, xh, xl);
  // ---- qkv: 24 panels; the q tiles (first 8 panels) are kept for the folds
  f32x4 qa[16];
  const float inv0 = a.inv_qkv * (1.0f / sx);
  float* orow = a.qkv + (size_t)row * 768;
  static_for<0, 24>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const unsigned p = next_panel(std::integral_constant<int, j>{});
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = f32x4{0.f, 0.f, 0.f, 0.f};
    tb_mma<8>(c0, c1, p, xh, xl, fr, fg, false);
    const float4 b0 = *reinterpret_cast<const float4*>(a.bias + 32 * j + 4 * fg);
    const float4 b1 = *reinterpret_cast<const float4*>(a.bias + 32 * j + 16 + 4 * fg);
    c0 = f32x4{c0[0] * inv0 + b0.x, c0[1] * inv0 + b0.y, c0[2] * inv0 + b0.z, c0[3] * inv0 + b0.w};
    c1 = f32x4{c1[0] * inv0 + b1.x, c1[1] * inv0 + b1.y, c1[2] * inv0 + b1.z, c1[3] * inv0 + b1.w};
    {
      if constexpr (VT && j >= 16) {  // v channel c of token tok of its cloud -> vT[cloud][c][tok]: 16 consecutive tokens per lane group
        float* vt = a.vT + (size_t)(row / a.n) * 256 * a.ldp + (row % a.n);
        const int cb = 32 * (j - 16) + 4 * fg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vt[(size_t)(cb + r) * a.ldp] = c0[r];
          vt[(size_t)(cb + 16 + r) * a.ldp] = c1[r];
        }
      } else {
        *reinterpret_cast<float4*>(orow + 32 * j + 4 * fg) = make_float4(c0[0], c0[1], c0[2], c0[3]);
        *reinterpret_cast<float4*>(orow + 32 * j + 16 + 4 * fg) = make_float4(c1[0], c1[1], c1[2], c1[3]);
      }
    }
    if constexpr (j < 8) {
      qa[2 * j] = c0;
      qa[2 * j + 1] = c1;
    }
  });
  half8 qh[8], ql[8];
  const float sq = tb_split_rows<16>(qa, qh, ql);
  // ---- per head: qp_h = Wp_h^T q_h (8 panels, K = 64 = k-steps 2h, 2h+1 of q), then qd_h = D_c^T qp_h (1 panel, K = 256)
  const float inv1 = a.inv_wp * (1.0f / sq);
  static_for<0, 4>([&](auto HH) {
    constexpr int h = decltype(HH)::value;
    f32x4 pa[16];
    static_for<0, 2>([&](auto GG) {
      constexpr int gq = decltype(GG)::value;
      const unsigned p4 = next_panel(std::integral_constant<int, 24 + 3 * h + gq>{});
      static_for<0, 4>([&](auto U) {
        constexpr int j = 4 * gq + decltype(U)::value;
        f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = f32x4{0.f, 0.f, 0.f, 0.f};
        tb_mma<2>(c0, c1, p4 + decltype(U)::value * TB_P64, qh + 2 * h, ql + 2 * h, fr, fg, false);
        pa[2 * j] = f32x4{c0[0] * inv1, c0[1] * inv1, c0[2] * inv1, c0[3] * inv1};
        pa[2 * j + 1] = f32x4{c1[0] * inv1, c1[1] * inv1, c1[2] * inv1, c1[3] * inv1};
      });
    });
    {
      float* o = a.qp + (size_t)row * 1024 + 256 * h;
#pragma unroll
      for (int i = 0; i < 16; ++i) *reinterpret_cast<float4*>(o + 16 * i + 4 * fg) = make_float4(pa[i][0], pa[i][1], pa[i][2], pa[i][3]);
    }
    half8 ph[8], pl[8];
    const float sp = tb_split_rows<16>(pa, ph, pl);
    const unsigned p = next_panel(std::integral_constant<int, 24 + 3 * h + 2>{});
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = f32x4{0.f, 0.f, 0.f, 0.f};
    tb_mma<8>(c0, c1, p, ph, pl, fr, fg, false);
    {
      const float inv2 = a.inv_dc * (1.0f / sp);
      float* o = a.qd + ((size_t)row * 4 + h) * 32;
      *reinterpret_cast<float4*>(o + 4 * fg) = make_float4(c0[0] * inv2, c0[1] * inv2, c0[2] * inv2, c0[3] * inv2);
      *reinterpret_cast<float4*>(o + 16 + 4 * fg) = make_float4(c1[0] * inv2, c1[1] * inv2, c1[2] * inv2, c1[3] * inv2);
    }
  });
}

extern "C" long sam6d_rpe_front_image_bytes(void) { return RF_IMAGE_BYTES; }

static int rpe_front_launch(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc,
                            float* qkv, float* qp, float* qd, long M, float* vT, int n, int ldp, void* stream);
extern "C" int sam6d_rpe_front(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc,
                               float* qkv, float* qp, float* qd, long M, void* stream) {
  return rpe_front_launch(x, wimage, bias_qkv, inv_qkv, inv_wp, inv_dc, qkv, qp, qd, M, nullptr, 1, 1, stream);
}
extern "C" int sam6d_rpe_front_vt(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc,
                                  float* qkv, float* qp, float* qd, long M, float* vT, int n, int ldp, void* stream) {
  SAM6D_REQUIRE(vT && n > 0 && ldp >= n && M % n == 0, "rpe_front_vt: vT (M / n, 256, ldp) needs n > 0, ldp >= n, M a multiple of n");
  return rpe_front_launch(x, wimage, bias_qkv, inv_qkv, inv_wp, inv_dc, qkv, qp, qd, M, vT, n, ldp, stream);
}
static int rpe_front_launch(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc,
                            float* qkv, float* qp, float* qd, long M, float* vT, int n, int ldp, void* stream) {
  SAM6D_REQUIRE(x && wimage && bias_qkv && qkv && qp && qd && M >= 0, "rpe_front: bad arguments");
  SAM6D_REQUIRE(((((size_t)x) | ((size_t)wimage) | ((size_t)bias_qkv) | ((size_t)qkv) | ((size_t)qp) | ((size_t)qd)) & 15) == 0,
                "rpe_front: pointers must be 16-byte aligned");
  if (M == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "rpe_front", {{(const void*)rpe_front_kernel<false>, 2 * TB_PANEL_BYTES},
                                                      {(const void*)rpe_front_kernel<true>, 2 * TB_PANEL_BYTES}}))
    return rc;
  RfArgs a{x, (const unsigned char*)wimage, bias_qkv, qkv, qp, qd, M, inv_qkv, inv_wp, inv_dc, vT, n, ldp};
  const dim3 g((unsigned)((M + 63) / 64));
  if (vT)
    hipLaunchKernelGGL(rpe_front_kernel<true>, g, dim3(512), 2 * TB_PANEL_BYTES, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rpe_front_kernel<false>, g, dim3(512), 2 * TB_PANEL_BYTES, (hipStream_t)stream, a);
  SAM6D_LAUNCH_CHECK("rpe_front");
}

// ---------------------------------------------------------------------------------------------------------------------
// out_proj + F.normalize + the operand split of the fine similarity in one pass over the dense tokens
// (FinePointMatching.forward: out_proj, PEM/model/fine_point_matching.py:70-72; compute_feature_similarity: F.normalize(dim=2),
// PEM/utils/model_utils.py:141-142):   y = x W^T + b;   fh | fl = fp16 hi / lo of (y / max(|y|, 1e-12)) * 2^10
// -- what sam6d_gemm_nt followed by finematch.hip's fm_prep_kernel produce (a 134 MB fp32 intermediate written and read back at
// B = 32).  One workgroup = 64 token rows on four waves, the same register-chained transposed product as token_block_kernel; rows are
// read non-temporally (each exactly once).
struct OsArgs {
  const float* x;            // (M, 256)
  const unsigned char* wimg; // sam6d_pack_panels(W, 256 rows, k0 = 0, ksteps = 8): 8 panels
  const float* bias;         // (256)
  _Float16* fh;              // (M, 256)
  _Float16* fl;
  long M;
  float inv_w;               // 1 / pack scale of W
  int half;
};

// The four waves issue their own DMA, one panel per slot (64 KB of LDS: two workgroups per CU, one's row loads / stores beside the
// other's products) -- the shape for this pure streaming pass.
__global__ __launch_bounds__(256, 2) void out_split_kernel(OsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const unsigned pan_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
  auto dma_step = [&](int T) {  // panel T into slot T & 1, dealt to the four waves
    dma_pieces<8>(a.wimg + (size_t)T * TB_PANEL_BYTES, lds + (T & 1) * TB_PANEL_BYTES, wave, 4, lane);
  };
  dma_step(0);
  const long r0 = (long)blockIdx.x * 64 + wave * 16 + fr;
  const bool valid = r0 < a.M;
  const long row = valid ? r0 : a.M - 1;
  half8 xh[8], xl[8];
  const float sx = split_row256<true>(a.x + (size_t)row * 256, fg, xh, xl);
  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool half = a.half != 0;
  static_for<0, 8>([&](auto J) {
    constexpr int j = decltype(J)::value;
    // panel j has landed and is published; the slot of panel j - 1 is free
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (j + 1 < 8) dma_step(j + 1);
    const unsigned p = pan_lds + (j & 1) * TB_PANEL_BYTES;
    tb_mma<8>(acc[2 * j], acc[2 * j + 1], p, xh, xl, fr, fg, half);
  });
  const float inv = a.inv_w * (1.0f / sx);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float4 bb = *reinterpret_cast<const float4*>(a.bias + 16 * i + 4 * fg);
    acc[i][0] = acc[i][0] * inv + bb.x;
    acc[i][1] = acc[i][1] * inv + bb.y;
    acc[i][2] = acc[i][2] * inv + bb.z;
    acc[i][3] = acc[i][3] * inv + bb.w;
    ss += (acc[i][0] * acc[i][0] + acc[i][1] * acc[i][1]) + (acc[i][2] * acc[i][2] + acc[i][3] * acc[i][3]);
  }
  const float d = fmaxf(sqrtf(tok_sum(ss)), 1e-12f);
  if (valid) {
    _Float16* oh = a.fh + (size_t)row * 256 + 4 * fg;
    _Float16* ol = a.fl + (size_t)row * 256 + 4 * fg;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      unsigned h01, l01, h23, l23;
      sam6d_split2_f16((acc[i][0] / d) * 1024.0f, (acc[i][1] / d) * 1024.0f, h01, l01);
      sam6d_split2_f16((acc[i][2] / d) * 1024.0f, (acc[i][3] / d) * 1024.0f, h23, l23);
      *reinterpret_cast<u32x2*>(oh + 16 * i) = u32x2{h01, h23};
      *reinterpret_cast<u32x2*>(ol + 16 * i) = u32x2{l01, l23};
    }
  }
}

// (Measured and removed, round 4: the same pass as a PERSISTENT kernel -- one workgroup per CU, four computing + four loader waves, the
// loader waves streaming the eight panels round and round without a bubble at the tile seams, each computing wave requesting the NEXT
// tile's rows right after splitting the current ones (no LDS-DMA in the computing waves' vector-memory queue, so nothing orders the row
// loads behind a panel wait).  Same bits; 117.5 / 117.9 us against 111.8 us per launch at M = 131 136 (scratch/ub_stream.py).  The row
// latency was not the bound: every 64-row tile re-streams the 256 KB weight image through the LDS-DMA path, 2048 tiles x 256 KB = 537 MB
// per launch at ~18 GB/s per CU (4.6 TB/s chip-wide) -- the pass moves twice as many weight bytes L2 -> LDS as token bytes HBM -> registers.
// Fewer weight bytes per row need wider row tiles (128 rows on eight computing waves without loader waves) or resident weights (256 KB
// of fp16 hi / lo do not fit the 160 KB of LDS; half the output channels do, but the row norm needs all 256).)
extern "C" int sam6d_linear_norm_split(const float* x, const void* wimage, const float* bias, float inv_w_scale, void* fh, void* fl,
                                       long M, void* stream) {
  SAM6D_REQUIRE(x && wimage && bias && fh && fl && M >= 0 && inv_w_scale > 0.f, "linear_norm_split: bad arguments");
  SAM6D_REQUIRE(((((size_t)x) | ((size_t)wimage) | ((size_t)bias) | ((size_t)fh) | ((size_t)fl)) & 15) == 0,
                "linear_norm_split: pointers must be 16-byte aligned");
  if (M == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "linear_norm_split", {{(const void*)out_split_kernel, 2 * TB_PANEL_BYTES}})) return rc;
  OsArgs a{x, (const unsigned char*)wimage, bias, (_Float16*)fh, (_Float16*)fl, M, inv_w_scale, sam6d_half_for(1)};
  hipLaunchKernelGGL(out_split_kernel, dim3((unsigned)((M + 63) / 64)), dim3(256), 2 * TB_PANEL_BYTES, (hipStream_t)stream, a);
  SAM6D_LAUNCH_CHECK("linear_norm_split");
}

// ---------------------------------------------------------------------------------------------------------------------
// y = x W^T + b for a few thousand 256-channel token rows (the sparse-token projections: in_proj / out_proj of the coarse stage,
// [proj_k; proj_v] of the dense layers' memory tokens -- PEM/model/coarse_point_matching.py:35-38, 61; PEM/model/transformer.py:556-558):
// 197 workgroups of 64 rows on panel machinery like token_block_kernel's, with loader waves of its own (four computing + four loader
// waves, two panels per ring slot) instead of the generic GEMM's 64 x 64 tiles, whose ~1600 single-k-chunk workgroups are launch-latency-bound at this size.
// Rows may be strided per cloud on both sides (row R = cloud R / rpb, token R % rpb): the bg slot of a token buffer is skipped in place.
struct RlArgs {
  const float* x;
  const unsigned char* wimg;  // sam6d_pack_panels(W, 32 NP rows, k0 = 0, ksteps = 8): NP panels
  const float* bias;          // (32 NP) or null
  float* out;
  long M;
  int rpb;                    // rows per cloud
  long x_bs, x_r0, o_bs, o_r0;  // input / output: rows between two clouds, first row of a cloud
  float inv_w;
  int half;
};

template <int NP>
__global__ __launch_bounds__(512, 1) void rows_linear_kernel(RlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), fr = lane & 15, fg = lane >> 4;
  const unsigned pan_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
  constexpr int SLOT = 2 * TB_PANEL_BYTES, NSTEP = NP / 2;
  static_assert(NP % 2 == 0, "two panels per step");
  if (wave >= 4) {  // loader waves
    auto dma_step = [&](int T) {
      dma_pieces<16>(a.wimg + (size_t)T * SLOT, lds + (T & 1) * SLOT, wave - 4, 4, lane);
    };
    dma_step(0);
#pragma unroll
    for (int T = 0; T < NSTEP; ++T) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (T + 1 < NSTEP) dma_step(T + 1);
    }
    return;
  }
  const long r0 = (long)blockIdx.x * 64 + wave * 16 + fr;
  const bool valid = r0 < a.M;
  const long R = valid ? r0 : a.M - 1;
  const long cb = R / a.rpb, cr = R - cb * a.rpb;
  half8 xh[8], xl[8];
  const float sx = split_row256<false>(a.x + (size_t)(cb * a.x_bs + a.x_r0 + cr) * 256, fg, xh, xl);
  const bool half = a.half != 0;
  const float inv = a.inv_w * (1.0f / sx);
  float* orow = a.out + (size_t)(cb * a.o_bs + a.o_r0 + cr) * (32 * NP);
  static_for<0, NP>([&](auto J) {
    constexpr int j = decltype(J)::value;
    if constexpr ((j & 1) == 0) __syncthreads();  // step j / 2 has landed (loader waves) and is published
    const unsigned p = pan_lds + ((j >> 1) & 1) * SLOT + (j & 1) * TB_PANEL_BYTES;
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = f32x4{0.f, 0.f, 0.f, 0.f};
    tb_mma<8>(c0, c1, p, xh, xl, fr, fg, half);
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if (a.bias) {
      b0 = *reinterpret_cast<const float4*>(a.bias + 32 * j + 4 * fg);
      b1 = *reinterpret_cast<const float4*>(a.bias + 32 * j + 16 + 4 * fg);
    }
    if (valid) {
      *reinterpret_cast<float4*>(orow + 32 * j + 4 * fg) = make_float4(c0[0] * inv + b0.x, c0[1] * inv + b0.y, c0[2] * inv + b0.z, c0[3] * inv + b0.w);
      *reinterpret_cast<float4*>(orow + 32 * j + 16 + 4 * fg) = make_float4(c1[0] * inv + b1.x, c1[1] * inv + b1.y, c1[2] * inv + b1.z, c1[3] * inv + b1.w);
    }
  });
}

extern "C" int sam6d_rows_linear(const float* x, const void* wimage, int npanels, const float* bias, float inv_w_scale, float* out,
                                 long M, int rows_per_cloud, long x_cloud_rows, long x_row0, long out_cloud_rows, long out_row0,
                                 void* stream) {
  SAM6D_REQUIRE(x && wimage && out && M >= 0 && inv_w_scale > 0.f, "rows_linear: bad arguments");
  SAM6D_REQUIRE(npanels == 8 || npanels == 16, "rows_linear: built for 256 or 512 output channels (8 or 16 panels), got %d panels", npanels);
  SAM6D_REQUIRE(rows_per_cloud > 0 && x_cloud_rows >= rows_per_cloud && out_cloud_rows >= rows_per_cloud && x_row0 >= 0 && out_row0 >= 0,
                "rows_linear: bad row mapping");
  SAM6D_REQUIRE(((((size_t)x) | ((size_t)wimage) | ((size_t)bias) | ((size_t)out)) & 15) == 0, "rows_linear: pointers must be 16-byte aligned");
  if (M == 0) return 0;
  static unsigned long long done = 0;
  if (int rc = sam6d_reserve_lds(&done, "rows_linear", {{(const void*)rows_linear_kernel<8>, 4 * TB_PANEL_BYTES},
                                                        {(const void*)rows_linear_kernel<16>, 4 * TB_PANEL_BYTES}}))
    return rc;
  RlArgs a{x, (const unsigned char*)wimage, bias, out, M, rows_per_cloud, x_cloud_rows, x_row0, out_cloud_rows, out_row0, inv_w_scale,
           sam6d_half_for(1)};
  const dim3 g((unsigned)((M + 63) / 64));
  if (npanels == 8)
    hipLaunchKernelGGL(rows_linear_kernel<8>, g, dim3(512), 4 * TB_PANEL_BYTES, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(rows_linear_kernel<16>, g, dim3(512), 4 * TB_PANEL_BYTES, (hipStream_t)stream, a);
  SAM6D_LAUNCH_CHECK("rows_linear");
}

// The launched shapes: the dense layer (sam6d_linattn_layer) runs token_block_kernel, 64 tokens per workgroup; the 197-token layers
// (sam6d_token_block) run token_tail_kernel: eight waves per 32- or 64-token tile, output channels dealt to the waves.
static int tb_reserve_lds(const char* name) {
  static unsigned long long done = 0;
  return sam6d_reserve_lds(&done, name, {{(const void*)token_block_kernel, TB_LDS_BYTES},
                                         {(const void*)token_tail_kernel<2, TT_D2, false>, TT_LDS_BYTES(2)},
                                         {(const void*)token_tail_kernel<4, TT_D4, false>, TT_LDS_BYTES(4)},
                                         {(const void*)token_tail_kernel<2, TT_D2, true>, TT_LDS_BYTES(2)},
                                         {(const void*)token_tail_kernel<4, TT_D4, true>, TT_LDS_BYTES(4)}});
}

extern "C" int sam6d_token_block(const float* hidden, const float* x, const void* wimage, const float* consts, float* out, long M,
                                 float eps, void* stream) {
  SAM6D_REQUIRE(hidden && x && wimage && consts && out && M >= 0, "token_block: bad arguments");
  SAM6D_REQUIRE(((((size_t)hidden) | ((size_t)x) | ((size_t)out) | ((size_t)wimage)) & 15) == 0, "token_block: pointers must be 16-byte aligned");
  if (M == 0) return 0;
  if (int rc = tb_reserve_lds("token_block")) return rc;
  TbArgs a{hidden, x, out, (const unsigned char*)wimage, consts, nullptr, nullptr, nullptr, M, 0, 0, 0, eps,
           sam6d_half_for(1)};
  // The tile shape is a function of M and the CU count only: 32-token tiles while they all fit the chip in one round (6304 rows = 197
  // workgroups on 256 CUs), 64-token tiles beyond (12608 rows = 197 workgroups; each streams the weight image once, so 64 tokens halve
  // the L2 bytes per token).  Measured at 12608 rows: 394 x 32 tokens 45.6 us (two 512-thread workgroups of 208 registers per lane do not
  // share a CU, so 138 CUs run two tiles one after the other), 197 x 64 tokens 34.0 us.  A token's arithmetic does not depend on the
  // shape (token_tail_kernel): bit-identical results either way.
  int cus = sam6d_cu_count();
  if (cus <= 0) cus = 256;  // (an unknown device: the MI355X's count)
  const bool small = (M + 31) / 32 <= cus;
  const dim3 grid((unsigned)(small ? (M + 31) / 32 : (M + 63) / 64));
  const int ldsb = small ? TT_LDS_BYTES(2) : TT_LDS_BYTES(4);
  auto kernel = small ? (a.half ? token_tail_kernel<2, TT_D2, true> : token_tail_kernel<2, TT_D2, false>)
                      : (a.half ? token_tail_kernel<4, TT_D4, true> : token_tail_kernel<4, TT_D4, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(512), ldsb, (hipStream_t)stream, a);
  SAM6D_LAUNCH_CHECK("token_block");
}

extern "C" int sam6d_linattn_layer(const float* D, const void* wimage, const float* consts, const void* kvimage, const float* kvinv,
                                   const float* ksum, float* Dout, int B, int I, int row0, float eps, void* stream) {
  SAM6D_REQUIRE(D && wimage && consts && kvimage && kvinv && ksum && Dout && B >= 0 && I > 0 && row0 >= 0 && row0 < I,
                "linattn_layer: bad arguments");
  // (kvinv: the kernel reads a cloud's four head scales as one 16-byte load)
  SAM6D_REQUIRE(((((size_t)D) | ((size_t)Dout) | ((size_t)wimage) | ((size_t)kvimage) | ((size_t)kvinv)) & 15) == 0,
                "linattn_layer: pointers must be 16-byte aligned");
  if (B == 0) return 0;
  if (int rc = tb_reserve_lds("linattn_layer")) return rc;
  const int tiles = (I - row0 + 16 * TB_WAVES - 1) / (16 * TB_WAVES);  // 64-token workgroups
  SAM6D_REQUIRE((long)B * tiles < 2147483647L, "linattn_layer: too many tiles");
  TbArgs a{D, nullptr, Dout, (const unsigned char*)wimage, consts, (const unsigned char*)kvimage, kvinv, ksum, 0, I, row0, tiles, eps,
           sam6d_half_for(1)};
  hipLaunchKernelGGL(token_block_kernel, dim3((unsigned)(B * tiles)), dim3(TB_WAVES * 64), TB_LDS_BYTES, (hipStream_t)stream, a);
  SAM6D_LAUNCH_CHECK("linattn_layer");
}
