/*
 * libsam6d_hip.so -- C ABI of the MI355X (gfx950) implementation of SAM-6D's geometric-matching hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / ATen types.  Every pointer is a
 * DEVICE pointer unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default stream);
 * launches are asynchronous on that stream, never synchronise, never allocate, and are graph-capturable.
 * Tensors are dense row-major float32 / int32 exactly as the reference's call sites hand them over
 * (callers `.contiguous()` first: PEM/utils/model_utils.py:77-79, PEM/model/fine_point_matching.py:128,136).
 *
 * Return value: 0 on success; <0 for a rejected argument (SAM6D_EINVAL = -1, the analogue of the reference's
 * TORCH_CHECK in EXT/include/utils.h:20-45); >0 = hipError_t of a failed launch (the reference prints and exit(-1)s,
 * EXT/include/cuda_utils.h:42-51).  sam6d_last_error() returns the message of the last failure on this thread.
 *
 * Path shorthands: PEM = SAM-6D/Pose_Estimation_Model, EXT = PEM/model/pointnet2/_ext_src,
 *                  ISM = SAM-6D/Instance_Segmentation_Model (all under the reference repository root).
 */
#ifndef SAM6D_HIP_H
#define SAM6D_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* sam6d_last_error(void);
/* ABI version of this header: bumped on any change of a signature OR of the size / layout of a buffer an entry reads or writes.
 * A consumer compares sam6d_abi_version() of the loaded library with the SAM6D_ABI_VERSION it was compiled against and refuses a
 * mismatch (sam6d_hip/_lib.py and tests/cabi/cabi_check.c do).
 *   1  rounds 1-3
 *   2  sam6d_set_thread_matmul_mode added; round 3's layout change made visible: sam6d_linattn_kv_pack / sam6d_linattn_kv_image write 4*B floats to `inv` (one image
 *      scale per head), sam6d_linattn_layer reads kvinv as (B,4) -- a version-1 consumer allocated B floats
 *   4  sam6d_gemm_ln256 removed (nothing selected it since its switch SAM6D_FUSED_LN was retired)
 *   5  sam6d_draw_choice added
 *   6  sam6d_render_views and sam6d_mesh_sample added, with their _workspace_bytes */
#define SAM6D_ABI_VERSION 6
int sam6d_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * B1: the `pointnet2._ext` seam (EXT/src/bindings.cpp:11-24).  Semantics = the reference's CPU loops, bit-exact.
 * ---------------------------------------------------------------------------------------------------------- */

/* replaces `at::Tensor furthest_point_sampling(at::Tensor points, const int nsamples)`
 * (EXT/src/sampling.cpp:184-212; loop :76-118).  xyz (B,N,3) f32 -> idx (B,m) i32.
 * temp: (B,N) f32 scratch, required only when N > 4096 (the reference allocates the same `tmp`, :192-194). */
int sam6d_furthest_point_sampling(const float* xyz, int B, int N, int m, float* temp, int* idx, void* stream);
/* Test hook of the multi-workgroup FPS (N > 4096; EXT/src/sampling.cpp:76-118 is the loop it replaces): the number of polls a
 * workgroup waits at the grid-wide arg-max of a round before it gives the cloud up to the one-workgroup kernel queued behind it
 * (cap < 0: the default, 2^24; 0: give up at once).  Results are identical on both paths. */
int sam6d_fps_debug_spin_cap(long cap);

/* replaces `at::Tensor gather_points(at::Tensor points, at::Tensor idx)` (EXT/src/sampling.cpp:120-150; loop :23-44).
 * points (B,C,N) f32, idx (B,M) i32 -> out (B,C,M) f32; out-of-range index -> 0. */
int sam6d_gather_points(const float* points, const int* idx, int B, int C, int N, int M, float* out, void* stream);

/* replaces `at::Tensor ball_query(at::Tensor new_xyz, at::Tensor xyz, const float radius, const int nsample)`
 * (EXT/src/ball_query.cpp:64-93; loop :16-62).  new_xyz (B,M,3), xyz (B,N,3) -> idx (B,M,nsample) i32,
 * every slot written (empty ball -> zeros, like the reference's zero-initialised output). */
int sam6d_ball_query(const float* new_xyz, const float* xyz, int B, int N, int M, float radius, int nsample, int* idx,
                     void* stream);
/* sam6d_ball_query for two radii over the same (queries, cloud) in one pass -- PositionalEncoding queries r1 = 0.1 / 32 samples
 * and r2 = 0.2 / 64 samples around the same points (PEM/model/fine_point_matching.py:108-131, EXT/src/ball_query.cpp:16-62);
 * idx1 (B,M,nsample1), idx2 (B,M,nsample2), each identical to the single-radius call. */
int sam6d_ball_query2(const float* new_xyz, const float* xyz, int B, int N, int M, float radius1, int nsample1, int* idx1,
                      float radius2, int nsample2, int* idx2, void* stream);
/* sam6d_ball_query2 with spatial pruning (same call site, PEM/model/fine_point_matching.py:108-131; semantics EXT/src/ball_query.cpp:16-62,
 * identical outputs): the cloud is bucketed into a uniform grid first and a query only tests the points of the 27 cells around it;
 * the first-nsample-in-index-order rule is kept by collecting hits in a per-query bit mask.  ws: sam6d_ball_query2_grid_workspace_bytes(B, N)
 * bytes of scratch, 16-byte aligned.  N > 8192 falls back to the all-pairs scan. */
size_t sam6d_ball_query2_grid_workspace_bytes(int B, int N);
int sam6d_ball_query2_grid(const float* new_xyz, const float* xyz, int B, int N, int M, float radius1, int nsample1, int* idx1,
                           float radius2, int nsample2, int* idx2, void* ws, size_t ws_bytes, void* stream);
/* sam6d_ball_query2_grid (PEM/model/fine_point_matching.py:108-131; EXT/src/ball_query.cpp:16-62) that also reports how many slots of
 * a query hold hits: cnt1, cnt2 (B,M) i32, cnt = clamp(hits, 1, nsample).  The slots from cnt on repeat slot 0, as the reference pads
 * them (ball_query.cpp:44-49); an empty ball counts 1, its slots all being index 0.  idx1 / idx2 are those of sam6d_ball_query2_grid.
 * (New entry only, so SAM6D_ABI_VERSION stays.) */
int sam6d_ball_query2_grid_counts(const float* new_xyz, const float* xyz, int B, int N, int M, float radius1, int nsample1, int* idx1,
                                  float radius2, int nsample2, int* idx2, void* ws, size_t ws_bytes, int* cnt1, int* cnt2,
                                  void* stream);

/* replaces `at::Tensor group_points(at::Tensor points, at::Tensor idx)` (EXT/src/group_points.cpp:79-108; loop :20-45).
 * points (B,C,N) f32, idx (B,M,S) i32 -> out (B,C,M,S) f32. */
int sam6d_group_points(const float* points, const int* idx, int B, int C, int N, int M, int S, float* out,
                       void* stream);

/* Row-major companion of gather_points used inside the pipeline (the reference transposes to (B,C,N), gathers and
 * transposes back: PEM/utils/model_utils.py:76-80, PEM/model/transformer.py:667-705):
 * out[b,j,:] = feats[b, idx[b,j] + idx_off, :], rows of C floats (C % 4 == 0); batch strides in floats. */
int sam6d_gather_rows(const float* feats, const int* idx, int B, int N, int M, int C, long in_stride_b,
                      long out_stride_b, int idx_off, float* out, void* stream);

/* The same with row 0 of every feats[b] supplied separately: lead[b] (rows lead_stride_b floats apart) stands for feats[b,0,:], which
 * need not be written.  out[b,0,:] = lead[b,:], out[b,1+j,:] = feats[b, idx[b,j] + idx_off, :] (an index that lands on row 0 reads
 * lead[b]) -- the sparse tokens of SparseToDenseTransformer in one launch: bg token + FPS rows of the cat [bg; dense]
 * (PEM/model/transformer.py:667-705).  `out` rows 0 .. M. */
int sam6d_gather_rows_lead(const float* feats, const int* idx, int B, int N, int M, int C, long in_stride_b, long out_stride_b,
                           int idx_off, const float* lead, long lead_stride_b, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * B2: building blocks of the PEM Python modules (CoarsePointMatching / FinePointMatching / GeometricTransformer /
 * model_utils).  The reference runs these as torch ops; here each is one or a few HIP launches.
 * ---------------------------------------------------------------------------------------------------------- */

/* C = act(((A . W^T) / divisor) * colscale + bias) + residual  on the fp32 matrix cores.
 * replaces nn.Linear / 1x1-conv call sites (PEM/model/transformer.py:127-129,186-188,390-393,548-550;
 * PEM/model/coarse_point_matching.py:35-38) and the similarity contraction (PEM/utils/model_utils.py:144-150).
 * A (M,K) lda; W (N,K) ldw; C (M,N) ldc; residual (M,N) ldr or NULL; bias/colscale (N) or NULL; act 0 none / 1 ReLU /
 * 2 exact erf GELU (nn.GELU of the ViT MLP, PEM/model/feature_extraction.py:21-35), + 16 marks a geometric operand (the proj_p / Chebyshev folds of the RPE query) that keeps the fp16 x3 split in matmul mode 2,
 * + 32 asks for the whole-tile kernel where M and N are multiples of 128 and K of 32, with pre-split weights in matmul modes 1 and 2 (mode 0
 * ignores it): 128 x 128 tiles from 256 of them on (instead of 1024) and the unchecked whole-tile kernel also with act 2 (SAM's image encoder, 4096 rows per image,
 * ISM/segment_anything/modeling/image_encoder.py:166-182; no effect on other shapes);
 * `batch` independent problems with strides sA/sW/sC/sR (floats).  divisor = 1 disables the division. */
int sam6d_gemm_nt(const float* A, const float* W, const float* bias, const float* colscale, const float* residual,
                  float* C, int M, int N, int K, long lda, long ldw, long ldc, long ldr, int batch, long sA, long sW,
                  long sC, long sR, float divisor, int act, void* stream);
/* sam6d_gemm_nt with the weight operand cut into fp16 hi / lo halves ONCE, at weight-load time: Wh / Wl = the two outputs of
 * sam6d_split_f16(W, n, w_scale) -- same (N,K) layout, ldw and batch stride as W, w_scale a power of two that puts max |W| into
 * [2^13, 2^14).  Staging the weight tile is then a copy instead of a per-k-step split (the same nn.Linear call sites,
 * PEM/model/transformer.py:127-129,186-188,390-393,548-550).  W (fp32) is still required: out-of-range activation tiles are
 * recomputed with the exact fp32 loop.  In matmul mode 0 this is sam6d_gemm_nt. */
int sam6d_gemm_nt_w16(const float* A, const float* W, const void* Wh, const void* Wl, float w_scale, const float* bias,
                      const float* colscale, const float* residual, float* C, int M, int N, int K, long lda, long ldw, long ldc,
                      long ldr, int batch, long sA, long sW, long sC, long sR, float divisor, int act, void* stream);
/* sam6d_gemm_nt with a second (inner) batch level and no epilogue: problem (b1, b2) uses A + b1*sA + b2*sA2 etc.
 * (the per-cloud, per-head q.k^T and P.v products of the attention: PEM/model/transformer.py:137-149, 408-419). */
int sam6d_gemm_nt_b2(const float* A, const float* W, float* C, int M, int N, int K, long lda, long ldw, long ldc, int batch,
                     long sA, long sW, long sC, int batch2, long sA2, long sW2, long sC2, void* stream);
#define SAM6D_GEMM_ROUTE_EXACT 0      /* bits 0-1: exact fp32 MFMA loop (mode 0, or K < 32) */
#define SAM6D_GEMM_ROUTE_H3 1         /*           fp16 split, weight tile split per k-step */
#define SAM6D_GEMM_ROUTE_H3_W16 2     /*           fp16 split, pre-split weight halves */
#define SAM6D_GEMM_ROUTE_TILE128 4    /* 128 x 128 workgroup tiles (else 64 x 64) */
#define SAM6D_GEMM_ROUTE_FAST 8       /* whole-tile pre-split specialisation (no bounds checks) */
#define SAM6D_GEMM_ROUTE_WIDE 16      /* 16-byte epilogue (split kernels only) */
#define SAM6D_GEMM_ROUTE_HALF 32      /* single hi.hi product (matmul mode 2) */
#define SAM6D_GEMM_ROUTE_PLAIN 0      /* bits 6-7: workgroup order -- plain row-tile-major */
#define SAM6D_GEMM_ROUTE_COLGROUP 64  /*           column tiles of 8 row tiles grouped per XCD, last group padded */
#define SAM6D_GEMM_ROUTE_FOLD 128     /*           batch folded into grid.x, one element per XCD, last group of 8 padded */
#define SAM6D_GEMM_ROUTE_NONE 256     /* M, N or batch is 0: no launch */
/* The kernel route a GEMM launch with these arguments takes (the launch decision itself, shared with the launch; nothing is launched
 * and no pointer is dereferenced) for the nn.Linear / similarity call sites of sam6d_gemm_nt (PEM/model/transformer.py:127-129;
 * PEM/utils/model_utils.py:144-150).  Arguments: those of sam6d_gemm_nt_w16 (Wh = Wl = NULL: sam6d_gemm_nt) plus the inner batch
 * level of sam6d_gemm_nt_b2 (batch2 = 1, sA2 = sW2 = sC2 = 0 otherwise).  Reads the calling thread's matmul mode as the
 * launch does.  Returns a bit code >= 0 (SAM6D_GEMM_ROUTE_* above), or < 0 with the error the launch would report. */
int sam6d_gemm_route(const float* A, const float* W, const void* Wh, const void* Wl, float w_scale, const float* bias,
                     const float* colscale, const float* residual, const float* C, int M, int N, int K, long lda, long ldw, long ldc,
                     long ldr, int batch, long sA, long sW, long sC, long sR, float divisor, int act, int batch2, long sA2, long sW2,
                     long sC2);

/* Matrix-core arithmetic of gemm_nt / geo_embed: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain),
 * 1 = fp16 x3 split (x = hi + lo in fp16, 3 MFMAs, ~1e-6 relative; default), 2 = fp16 single product (hi . hi only, fp32
 * accumulate, ~1e-3 relative: the "fp16 MFMA GeometricTransformer" arithmetic of BASELINE.json config 5; applies to sam6d_gemm_nt,
 * the fused block / cross-attention / fine-match kernels and the RPE score contraction; the geometric indices, the outlier embedding
 * rows and the PE MLP keep the split).  All replace the same F.linear call sites (PEM/model/transformer.py:127-129); the mode is
 * process-wide.
 * Operand range in mode 1: ANY finite fp32 input is accepted.  sam6d_gemm_nt keeps the split for tiles whose operands lie in
 * [2^-6, 2^15) in magnitude (by their tile maximum; what the matching path produces itself is always there) and recomputes a tile
 * whose A or W block leaves that range with the exact fp32 MFMA loop of mode 0, so |x| >= 65520 cannot become inf - inf and uniformly
 * tiny operands do not lose their fp16 lo halves; the fused block kernels (sam6d_token_block, sam6d_linattn_layer,
 * sam6d_fine_match) scale every operand row / matrix by a power of two instead (exact to undo). */
int sam6d_set_matmul_mode(int mode);
int sam6d_get_matmul_mode(void);
/* The calling THREAD's override of the process-wide mode (same F.linear call sites, PEM/model/transformer.py:127-129): 0 / 1 / 2 as
 * above, -1 = follow the process default again.  sam6d_get_matmul_mode() returns the override while one is set.  A host that serves
 * two weight sets with different arithmetic in one process brackets each call sequence with it (sam6d_hip/pem.py does, from the
 * Options object its entry points take) instead of flipping the process default under another thread's launches. */
int sam6d_set_thread_matmul_mode(int mode);
int sam6d_get_thread_matmul_mode(void);

/* nn.LayerNorm(256) over `rows` rows (PEM/model/transformer.py:158,189,436,597).  eps as in torch (1e-5). */
int sam6d_layernorm256(const float* x, const float* gamma, const float* beta, float* y, long rows, long ldx, long ldy,
                       float eps, void* stream);

/* Fused transformer-block kernels (csrc/block.hip): a tile of 128 token rows (256 channels) stays on chip from the block's input to
 * its second LayerNorm; split-precision (fp16 x3) MFMA arithmetic with power-of-two operand scaling (range-safe for any finite fp32
 * input: no operand can overflow fp16).
 * sam6d_token_block: the tail of every attention layer -- AttentionLayer / RPEAttentionLayer after the attention itself, then
 *   AttentionOutput (PEM/model/transformer.py:152-160, 184-199, 436-444):
 *     y = LayerNorm(hidden . Wlin^T + b + x);  out = LayerNorm(relu(y . Wexp^T + b) . Wsq^T + b + y)        all (M,256)
 * sam6d_linattn_layer: the whole LinearTransformerLayer of the dense lift (PEM/model/transformer.py:532-622) on rows row0 .. I-1 of
 *   each of the B clouds of D (B,I,256): proj_q, focused kernel function, z, (phi(q) kv) z per head, then the tail above with x = D.
 *   kvimage / kvinv: sam6d_linattn_kv_pack of the (B,4,64,64) kv^T that sam6d_linattn_kv returns -- kvinv (B,4): the inverse
 *   power-of-two image scale of every head (16-byte aligned like D, Dout and the images: one load per cloud); ksum (B,256) its key
 *   sums.
 * wimage: the layer's weights as the kernels' LDS panel image (sam6d_token_block_image_bytes(mode) bytes, mode 1 = with proj_q),
 *   written by sam6d_pack_panels: rows x K fp32 -> 32-row panels of fp16 hi/lo halves, K in `ksteps` steps of 16 from column k0,
 *   values multiplied by `scale` (a power of two).  Image order: linear (8 panels, K=256) | 4 x { expand rows 128c.. (4 panels,
 *   K=256), squeeze columns 128c.. (8 panels, K=128) } | proj_q (8 panels, K=256; mode 1).
 * consts: 2568 floats: b_q | 1/softplus(scale) | b_lin | gamma1 | beta1 | b_expand (512) | b_squeeze | gamma2 | beta2 |
 *   {1/s_q, 1/s_lin, 1/s_exp, 1/(s_sq s_h), s_h, 0, 0, 0} with s_* the pack scales and s_h the scale of the FFN hidden row. */
int sam6d_pack_panels(const float* W, long ldw, int rows, int k0, int ksteps, float scale, void* dst, void* stream);
/* Front of RPEMultiHeadAttention.forward (PEM/model/transformer.py:395-405) in one launch: qkv (M,768) = x [Wq;Wk;Wv]^T + b, the
 * query folded through proj_p per head, qp (M,4,256) = Wp_h^T q_h (see sam6d_attention), and qd (M*4,32) = D_c^T qp_h (see
 * sam6d_rpe_scores).  wimage (sam6d_rpe_front_image_bytes() bytes) = sam6d_pack_panels of [Wq;Wk;Wv] (768 rows, ksteps 8), then per
 * head h of proj_p.weight^T (256 rows, k0 = 64 h, ksteps 2), then of D_c^T (32 rows, ksteps 8); inv_* = 1 / the three pack scales. */
long sam6d_rpe_front_image_bytes(void);
int sam6d_rpe_front(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc, float* qkv,
                    float* qp, float* qd, long M, void* stream);
/* The same launch with the values written TRANSPOSED per cloud of n tokens, vT (M / n, 256, ldp) -- the W operand of the P.v product
 * (sam6d_gemm_nt_b2), i.e. the `torch.matmul(attention_scores, v)` of PEM/model/transformer.py:416 -- instead of into the v third of
 * qkv (which is then left untouched): no separate sam6d_transpose pass. */
int sam6d_rpe_front_vt(const float* x, const void* wimage, const float* bias_qkv, float inv_qkv, float inv_wp, float inv_dc, float* qkv,
                       float* qp, float* qd, long M, float* vT, int n, int ldp, void* stream);
long sam6d_token_block_image_bytes(int mode);
long sam6d_linattn_kv_image_bytes(void);
int sam6d_linattn_kv_pack(const float* kvT, int B, void* image, float* inv, void* stream);
/* The k / v side of LinearAttention (PEM/model/transformer.py:547-572) in one launch: kv (B clouds, J rows of [256 k | 256 v] channels,
 * row stride ld, cloud stride `stride`, UNfocused keys) -> phi(k), kv^T and the key sums of the 4 heads, and the packed image of kv^T:
 * the same bits as sam6d_linattn_focus_k + sam6d_linattn_kv + sam6d_linattn_kv_pack (kv itself is left untouched). */
int sam6d_linattn_kv_image(const float* kv, const float* scale, int B, int J, long ld, long stride, void* image, float* inv,
                           float* ksum, void* stream);
int sam6d_token_block(const float* hidden, const float* x, const void* wimage, const float* consts, float* out, long M, float eps,
                      void* stream);
int sam6d_linattn_layer(const float* D, const void* wimage, const float* consts, const void* kvimage, const float* kvinv,
                        const float* ksum, float* Dout, int B, int I, int row0, float eps, void* stream);

/* replaces GeometricStructureEmbedding.forward (PEM/model/transformer.py:343-363; indices :306-341; sinusoid :259-285).
 * points (B,n,3) (bg point already prepended) -> out (B,n,n,256).  Workspaces: knn_ws (B*n*3 + 1) i32 (the last int is
 * the "index beyond the fast-sincos range" flag), idx_ws (B*n*n*4) f32. */
int sam6d_geo_embedding(const float* points, int B, int n, const float* div_term, const float* Wd, const float* bd,
                        const float* Wa, const float* ba, float sigma_d, float factor_a, int angle_k, int hidden,
                        int* knn_ws, float* idx_ws, float* out, void* stream);
/* the two halves of sam6d_geo_embedding: get_embedding_indices (PEM/model/transformer.py:306-341) -> idx_ws
 * (B,n,n,4) = {d_idx, a_idx[0..2]}, and the sinusoid + proj_d/proj_a + max contraction (:343-363) over `pairs` rows. */
int sam6d_geo_indices(const float* points, int B, int n, float sigma_d, float factor_a, int angle_k, int* knn_ws,
                      float* idx_ws, void* stream);
int sam6d_geo_embed(const float* idx_ws, long pairs, const float* div_term, const float* Wd, const float* bd,
                    const float* Wa, const float* ba, int hidden, const int* flag, int only_if_large, float* out,
                    void* stream);

/* fp16 x3 split-precision form of sam6d_geo_embed (same call site, PEM/model/transformer.py:343-363): w_packed =
 * [16][2][256][40] halves = per 16-wide K chunk, per matrix (proj_d, proj_a), per output column: 16 hi | 16 lo | 8 pad halves of
 * weight*1024, produced with sam6d_split_f16 (x -> fp16(x*scale), fp16(x*scale - hi)) at weight-load time.
 * `flag` = the last int of knn_ws written by sam6d_geo_indices: when an embedding index exceeds the range of the
 * branch-free sincos (1e5; never for radius-normalised clouds) the h3 kernel returns at once and a following
 * sam6d_geo_embed(..., flag, only_if_large = 1, ...) launch produces the result with the library sincosf. */
int sam6d_split_f16(const float* x, long n, float scale, void* hi, void* lo, void* stream);
int sam6d_geo_embed_h3(const float* idx_ws, long pairs, const float* div_term, const void* w_packed, const float* bd,
                       const float* ba, int hidden, const int* flag, float* out, void* stream);
/* Same contract as sam6d_geo_embed_h3 (PEM/model/transformer.py:343-363) with the sinusoid contraction replaced by a
 * 32-term Chebyshev expansion of proj_d(sinusoid(x)) / proj_a(sinusoid(x)) on [0, xmax] (w_cheb: 2 x 256 rows of
 * 144 B = 32 hi | 32 lo | 8 pad fp16 halves of coefficient * 1024, built at weight-load time in float64).  Pairs with
 * an index outside [0, xmax] are marked in pos_ws (pairs ints) / collected in list_ws (1 + pairs ints) and computed by the sinusoid kernel
 * (div_term, w_packed as for sam6d_geo_embed_h3), so the result is independent of xmax up to the ~1e-7 split-precision
 * error.  No-op when *flag != 0 (indices beyond the fast-sincos range: follow with sam6d_geo_embed(only_if_large=1)). */
int sam6d_geo_embed_cheb(const float* idx_ws, long pairs, const void* w_cheb, float xmax, const float* div_term,
                         const void* w_packed, const float* bd, const float* ba, int hidden, const int* flag, int* pos_ws,
                         int* list_ws, float* out, void* stream);

/* Fused RPE self-attention (RPETransformerLayer, PEM/model/transformer.py:366-420, on top of
 * GeometricStructureEmbedding :343-363) WITHOUT a materialised embedding.  Three entry points:
 *
 * sam6d_geo_outliers: after sam6d_geo_indices.  pos_ws[pair] (pairs ints) = -1 when all four indices of the pair lie in
 *   [0, xmax], else its row in `rows` (pairs x 256 floats capacity; only the listed rows are written): the bias-free
 *   embedding proj_d(sin(d)) + max_k proj_a(sin(a_k)) of that pair from the sinusoid kernels (w_packed / Wd / Wa, flag as
 *   for sam6d_geo_embed_h3 / sam6d_geo_embed).  list_ws: 1 + pairs ints of scratch.
 * sam6d_rpe_scores: P[q][h][0..n) (row stride ldp) = softmax_m((qk[q][h][m] + qp[q][h][:] . E[q][m][:]) / 8) for the Q = B*n
 *   queries, E rebuilt per key tile from the 32-term Chebyshev basis (wa_cheb = the proj_a half of the sam6d_geo_embed_cheb
 *   image; qd[q][h][0..32) = D_c^T qp[q][h], D_c = Chebyshev coefficients of proj_d) or read from `rows` for listed pairs.
 *   qp (Q,4,256) = proj_p folded into the query (see sam6d_attention), qk (Q,4,ldp) = q_h . k_h[m]; qk is updated in place
 *   (the geometric term of the listed pairs is added to it first, one wave per pair of list_ws).
 * sam6d_transpose: dst[b][c][j] = src[b][j][c] (the values as the N x K operand of the P.V GEMM).
 * sam6d_geo_outliers2 / sam6d_rpe_scores2: the same two steps with a range of their own for the three angular indices
 *   ([0, xmax_a]; the angle of GeometricStructureEmbedding.get_embedding_indices, transformer.py:326-341, times 180 / (sigma_a pi) never
 *   exceeds 180 / sigma_a = 12) -- wa_cheb then holds proj_a's expansion on [0, xmax_a] -- and `products` = 3 (every split product over
 *   all 32 orders) or 2 (the cross terms of the orders 0..15 in one MFMA, those of the orders >= 16 dropped: the caller guarantees
 *   that 2^-10 sum_{p >= 16} |c[ch][p]| is negligible for every channel).  The entries without the suffix = xmax_a = xmax, products = 3. */
int sam6d_geo_outliers(const float* idx_ws, long pairs, float xmax, const float* div_term, const void* w_packed, const float* Wd,
                       const float* Wa, const int* flag, int* pos_ws, int* list_ws, float* rows, void* stream);
int sam6d_rpe_scores(const float* idx_ws, const int* pos_ws, const int* list_ws, const float* rows, const void* wa_cheb, float xmax,
                     const float* qp, const float* qd, float* qk, float* P, long Q, int n, int ldp, void* stream);
int sam6d_geo_outliers2(const float* idx_ws, long pairs, float xmax, float xmax_a, const float* div_term, const void* w_packed,
                        const float* Wd, const float* Wa, const int* flag, int* pos_ws, int* list_ws, float* rows, void* stream);
int sam6d_rpe_scores2(const float* idx_ws, const int* pos_ws, const int* list_ws, const float* rows, const void* wa_cheb, float xmax,
                      float xmax_a, int products, const float* qp, const float* qd, float* qk, float* P, long Q, int n, int ldp,
                      void* stream);
/* The same layer with the attention itself in one launch per (cloud, head) (RPEMultiHeadAttention.forward,
 * PEM/model/transformer.py:405-416): sam6d_rpe_geo_scores writes only the geometric score term G[q][h][0..n) = qp[q][h] . E[q][m]
 * (row stride ldp, not yet divided by 8; arguments as sam6d_rpe_scores2 without qk); sam6d_rpe_self_attention then computes, for
 * qkv (B n, 768) = q | k | v of sam6d_rpe_front, hidden[:, 64h .. 64h+64) = softmax((q_h k_h^T + G) / 8) v_h  (n <= 208, ldp a
 * multiple of 4).  Replaces the q.k^T GEMM, the softmax inside sam6d_rpe_scores2 and the P.v GEMM. */
int sam6d_rpe_geo_scores(const float* idx_ws, const int* pos_ws, const int* list_ws, const float* rows, const void* wa_cheb, float xmax,
                         float xmax_a, int products, const float* qp, const float* qd, float* G, long Q, int n, int ldp, void* stream);
int sam6d_rpe_self_attention(const float* qkv, const float* G, float* hidden, int B, int n, int ldp, void* stream);
int sam6d_transpose(const float* src, long ld_src, long stride_src, int B, int n, int ncol, float* dst, long ld_dst,
                    long stride_dst, void* stream);

/* Cross attention of a TransformerLayer with the query projection inside (PEM/model/transformer.py:95-150: proj_q, per-head
 * softmax(q k^T / 8) v for 4 heads x 64) on the matrix cores, one workgroup per (cloud, head).  x (B,n,256) query-side tokens;
 * kv (B,m,512) = [proj_k | proj_v] of the memory tokens (one sam6d_gemm_nt); wq_image = sam6d_pack_panels(proj_q.weight, 256 rows,
 * k0 = 0, ksteps = 8, scale s) (256 KiB), inv_wq_scale = 1 / s; bq (256).  out (B,n,256) = the attention output before
 * AttentionLayer.linear.  n <= 256, m <= 208. */
int sam6d_cross_attention(const float* x, const float* kv, const void* wq_image, const float* bq, float inv_wq_scale, float* out,
                          int B, int n, int m, void* stream);
/* sam6d_cross_attention with the key-side projection inside as well (MultiHeadAttention.forward, PEM/model/transformer.py:127-129:
 * proj_k / proj_v of the memory tokens): mem (B,m,256) the memory tokens; wkv_image (sam6d_cross_attention_kv_image_bytes() bytes) =
 * per head h the sam6d_pack_panels images of proj_k.weight rows 64h..64h+64 then proj_v.weight rows 64h..64h+64 (K = 256, ksteps 8,
 * one common pack scale, inv_wkv_scale its inverse); bkv (512) = proj_k.bias | proj_v.bias.  k and v never reach HBM. */
long sam6d_cross_attention_kv_image_bytes(void);
int sam6d_cross_attention_kv(const float* x, const float* mem, const void* wq_image, const float* bq, float inv_wq_scale,
                             const void* wkv_image, const float* bkv, float inv_wkv_scale, float* out, int B, int n, int m,
                             void* stream);

/* replaces MultiHeadAttention.forward / RPEMultiHeadAttention.forward core (PEM/model/transformer.py:131-148,395-418):
 * 4 heads x 64, softmax((q.k [+ qp.E]) / 8) v.  q (B,n,256) ldq/sq; k,v (B,m,256); out (B,n,256).
 * RPE form: qp (B,n,4,256) = per-head query folded through proj_p, E (B,n,m,256); pass both NULL for the plain form. */
int sam6d_attention(const float* q, const float* k, const float* v, const float* qp, const float* E, float* out, int B,
                    int n, int m, long ldq, long ldk, long ldv, long ldo, long sq, long sk, long sv, long so,
                    void* stream);
/* Stand-alone pieces for callers of a single attention sub-module (the fused kernels never materialise the probabilities):
 * sam6d_scaled_softmax: out[r][0..n) = softmax_m((a[r][m] + b[r][m]) * scale), b may be NULL -- the softmax of MultiHeadAttention.forward
 *   (PEM/model/transformer.py:134-143) and, with b = the q . proj_p(E) term, of RPEMultiHeadAttention.forward (:404-412).
 * sam6d_sinusoid_embed: SinusoidalPositionalEmbedding.forward (PEM/model/transformer.py:269-285): x (n) -> out (n, d_model),
 *   out[i][2j] = sin(x_i div_term_j), out[i][2j+1] = cos(x_i div_term_j). */
int sam6d_scaled_softmax(const float* a, const float* b, float scale, long rows, int n, long lda, long ldb, float* out, long ldo,
                         void* stream);
int sam6d_sinusoid_embed(const float* x, long n, const float* div_term, int d_model, float* out, void* stream);

/* LinearAttention.forward pieces (PEM/model/transformer.py:546-578, kv path :569-572). */
int sam6d_linattn_focus_k(float* k, const float* scale, long rows, long ld, void* stream);
int sam6d_linattn_kv(const float* k, const float* v, int B, int J, long ldk, long ldv, long sk, long sv, float* kvT,
                     float* ksum, void* stream);
int sam6d_linattn_focus_q(float* q, const float* scale, const float* ksum, int B, long rows_per_b, long ld,
                          void* stream);

/* PositionalEncoding, one scale (PEM/model/fine_point_matching.py:126-139): QueryAndGroup
 * (PEM/model/pointnet2/pointnet2_utils.py:383-396) + SharedMLP 6->32->64->128 with eval BatchNorm folded to per-channel
 * scale/shift (PEM/model/pointnet2/pytorch_utils.py:25-50) + max over the ball, fused.  idx (B,N,S) from sam6d_ball_query
 * with new_xyz = pts + 1e-8; writes out[(b*N+j)*ldo + off + c], c < 128.  S must be a multiple of 32.
 * Range (split-precision mode): the six input features of a neighbour are scaled by a power of two chosen per neighbour, so layer 1
 * is accurate for coordinates of any magnitude; the hidden activations of layers 2 / 3 are split into fp16 halves unscaled and must
 * stay below 65504 -- coordinates below ~1e4 for weights of order one (PEM encodes radius-normalised clouds, |x| < 10).  Matmul mode 0
 * (exact fp32) has no such limit. */
int sam6d_pe_mlp_max(const float* pts, const int* idx, int B, int N, int S, const float* W1, const float* sc1,
                     const float* sh1, const float* W2, const float* sc2, const float* sh2, const float* W3,
                     const float* sc3, const float* sh3, float* out, long ldo, int off, void* stream);
/* sam6d_pe_mlp_max (PositionalEncoding's SharedMLPs, PEM/model/fine_point_matching.py:113-144) with an upper bound on the persistent
 * workgroups of the split-precision kernel (0 = fill the chip, 3 per CU): a launch that runs beside another stream's kernels leaves
 * them LDS and registers with 256 or 512. */
int sam6d_pe_mlp_max_wg(const float* pts, const int* idx, int B, int N, int S, const float* W1, const float* sc1, const float* sh1,
                        const float* W2, const float* sc2, const float* sh2, const float* W3, const float* sc3, const float* sh3,
                        float* out, long ldo, int off, int max_wg, void* stream);
/* sam6d_pe_mlp_max_wg (PEM/model/fine_point_matching.py:126-139) for indices whose padding is counted, as
 * sam6d_ball_query2_grid_counts returns them (the reference pads a ball's unused slots with its first hit, EXT/src/ball_query.cpp:44-49).
 * CONTRACT: cnt (B,N) i32 with 1 <= cnt[p] <= S for every point, and every slot l >= cnt[p] of row p of idx repeats an index that
 * occurs in a slot < cnt[p] of that row.  Under this contract the output equals sam6d_pe_mlp_max_wg on the same idx bit for bit: the
 * split-precision modes evaluate only the first cnt[p] slots of a point (rounded up to 8), packed four points' 8-slot pieces to a
 * 32-row tile -- a repeated neighbour cannot change a maximum.  Matmul mode 0 runs the exact-fp32 kernel over all slots and ignores
 * cnt.  A count outside [1, S] is clamped; indices that break the contract give the maximum over the counted slots only.
 * (New entry only, so SAM6D_ABI_VERSION stays.) */
int sam6d_pe_mlp_max_counted(const float* pts, const int* idx, int B, int N, int S, const float* W1, const float* sc1, const float* sh1,
                             const float* W2, const float* sc2, const float* sh2, const float* W3, const float* sc3, const float* sh3,
                             float* out, long ldo, int off, int max_wg, const int* cnt, void* stream);

/* y = (x - t) @ R per batch element (PEM/model/fine_point_matching.py:45). */
int sam6d_rigid_inverse(const float* x, const float* R, const float* t, int B, int N, float* y, void* stream);
/* strided row-block copy (the torch.cat call sites that add the bg token, PEM/model/coarse_point_matching.py:36-38). */
int sam6d_put_rows(const float* src, long s_src_b, long ld_src, float* dst, long s_dst_b, long ld_dst, int B, int rows,
                   int C, void* stream);
/* cat([bg_point(100,100,100), pts]) (PEM/model/pose_estimation_model.py:30-34). */
int sam6d_prepend_bg_point(const float* pts, int B, int n, float* out, void* stream);
/* y = x + s (new_xyz = pts + 1e-8, PEM/model/fine_point_matching.py:117) and a flat device copy of n floats
 * (batch stacking: the .repeat / torch.cat call sites PEM/run_inference_custom_pytorch.py:445-446). */
int sam6d_add_scalar(const float* x, float s, long n, float* y, void* stream);
/* flag[0] = 1 if x (B, n) holds B bitwise-identical rows, else 0: recognises the template tensors the reference's caller
 * `.repeat`s per instance (PEM/run_inference_custom_pytorch.py:445-446), whose pose-independent work then runs once. */
int sam6d_batch_rows_equal(const float* x, int B, long n, int* flag, void* stream);
int sam6d_copy_f32(const float* src, float* dst, long n, void* stream);
/* F.normalize(dim=-1) on 256-wide rows (PEM/utils/model_utils.py:141-142). */
int sam6d_l2norm256(const float* x, float* y, long rows, long ldx, long ldy, void* stream);

/* Soft assignment statistics and labels (PEM/utils/model_utils.py:229-235, 320-324): att (B,R,C);
 * rmax/rsum (B,R), cmax/csum (B,C), label1 (B,R-1) i32, label2 (B,C-1) i32; ws: scratch of >= 32*B*C floats. */
int sam6d_soft_assign(const float* att, int B, int R, int C, float* rmax, float* rsum, float* cmax, float* csum,
                      int* label1, int* label2, float* ws, long ws_floats, void* stream);
/* sam6d_soft_assign + sam6d_coarse_weights in one launch for matrices that fit the 160 KB of LDS of a CU (R * C + 3 R + 3 C floats:
 * the 197 x 197 coarse attention; 199 x 199 is the largest square), one workgroup per proposal; for R <= 256 every output has the
 * bits of the two-call form (same per-element arithmetic, same summation orders: PEM/utils/model_utils.py:229-240).  A taller matrix
 * that still fits (R > 256, C small) keeps this arithmetic -- expf and one sequential column sum, the reference's -- while
 * sam6d_soft_assign switches to 16 row slices and the hardware exponential there, so the two agree to rounding only.  rc < 0 for
 * larger matrices. */
int sam6d_coarse_soft_assign(const float* att, int B, int R, int C, float* rmax, float* rsum, float* cmax, float* csum, int* label1,
                             int* label2, float* weights, float* w1, void* stream);
/* replaces pairwise_distance(x, y) (PEM/utils/model_utils.py:101-128; normalized = False, channel-last): x (B,N,3), y (B,M,3) ->
 * out (B,N,M) = clamp((|x|^2 - 2 x.y) + |y|^2, min = 0) with the bits of torch's CPU evaluation (K = 3 matmul = an fma chain, plain
 * sums of squares: SURVEY 8c n1/n2).  The path's kernels inline the same device function; this entry is the direct check. */
int sam6d_pairwise_distance(const float* x, const float* y, int B, int N, int M, float* out, void* stream);
/* Sampling weights (S[1:,1:] * w1 * w2) ** 1.5 -> (B,(R-1)*(C-1)), w1 (B,R-1) (PEM/utils/model_utils.py:234-238). */
int sam6d_coarse_weights(const float* att, int B, int R, int C, const float* rmax, const float* rsum, const float* cmax,
                         const float* csum, const int* label1, const int* label2, float* weights, float* w1,
                         void* stream);
/* replaces cumsum + weighted_sampling_onnx_compatible (PEM/utils/model_utils.py:241-250, 277-305): `rand` (B,ns) are
 * the uniforms the reference draws with torch.rand (:292); idx (B,ns) i32; cum_ws (B,L) f32 scratch. */
int sam6d_weighted_sample(const float* weights, const float* rand, int B, int L, int ns, float* cum_ws, int* idx,
                          void* stream);
/* 3-point Procrustes per hypothesis + residual (PEM/utils/model_utils.py:244-257): idx (B,3*nh) -> Rs (B,nh,9),
 * ts (B,nh,3), dis (B,nh). */
int sam6d_coarse_hypotheses(const int* idx, const float* pts1, const float* pts2, int B, int N1, int N2, int nh,
                            float* Rs, float* ts, float* dis, void* stream);
/* torch.topk(k, largest=False) indices, ascending (PEM/utils/model_utils.py:258).  Equal values (-0 equals +0) come in
 * index order; a NaN of either sign ranks after +inf, lower index first, as torch.topk places it.  The order is total:
 * every slot of sel is written exactly once for any row, whichever kernel n and k select. */
int sam6d_select_smallest(const float* dis, int B, int n, int k, int* sel, void* stream);
/* Hypothesis scoring + argmax (PEM/utils/model_utils.py:261-270); model (B,P,3) raw, radius (B).  P <= 8192 (16 bytes of LDS a CAD
 * point, reserved on first use). */
int sam6d_score_select_hypotheses(const int* sel, const float* Rs, const float* ts, const float* pts1, const float* w1,
                                  const float* model, const float* radius, int B, int N1, int P, int nh, int k,
                                  float* scores, float* R, float* t, int* best, void* stream);
/* The same scoring + arg-max (PEM/utils/model_utils.py:258-275; the distance contraction is the reference's own torch.matmul,
 * :117) with the K = 3 products on the fp32 matrix cores -- identical distance bits -- and the weighted distances staged in `ws`
 * (sam6d_score_select_workspace_bytes(B, N1, k) bytes), summed per hypothesis in a fixed order.  P <= 4096. */
size_t sam6d_score_select_workspace_bytes(int B, int N1, int k);
int sam6d_score_select_hypotheses_ws(const int* sel, const float* Rs, const float* ts, const float* pts1, const float* w1,
                                     const float* model, const float* radius, int B, int N1, int P, int nh, int k, float* scores,
                                     float* R, float* t, int* best, float* ws, size_t ws_bytes, void* stream);
/* Fine-stage similarity + soft assignment as one pipeline (csrc/finematch.hip): compute_feature_similarity
 * (PEM/utils/model_utils.py:131-153: F.normalize both sides, f1 f2^T / temp) followed by the head of compute_fine_Rt (:308-331: the
 * two softmaxes, both arg-max label vectors, the masked assignment's row sums and weighted targets) without materialising the
 * attention matrix more than once.  f (2B, n, 256): out_proj outputs, scene clouds 0..B-1 then template clouds; n = 2049 (fine_npoint
 * 2048) or 4097 (BASELINE config 5: 4096-point fine matching; the label and assignment passes then run per 2048-column chunk and two
 * small kernels merge the chunks in ascending column order) -- rc < 0 otherwise: use sam6d_gemm_nt + sam6d_soft_assign +
 * sam6d_fine_assign.  pts2 (B, n-1, 3) template points.
 * -> label1, label2 (B, n-1) i32, pred (B, n-1, 3), weight (B, n-1).  ws: sam6d_fine_match_workspace_bytes_n(B, n) bytes
 * (sam6d_fine_match_workspace_bytes(B): the n = 2049 size).
 * temp >= sam6d_fine_match_min_temp() = 2 log2(e) / 125 = 0.0231 -- rc < 0 below it: the pipeline replaces the softmax's running maximum
 * (torch.softmax, PEM/utils/model_utils.py:320-321) by the fixed shift 1 / temp, which |cos| <= 1 allows, and exp(-2 / temp) must stay a
 * normal float32; smaller temperatures take sam6d_gemm_nt + sam6d_soft_assign + sam6d_fine_assign.  (New entry and a refusal of
 * inputs whose results were not finite, so SAM6D_ABI_VERSION stays.) */
float sam6d_fine_match_min_temp(void);
size_t sam6d_fine_match_workspace_bytes(int B);
size_t sam6d_fine_match_workspace_bytes_n(int B, int n);
int sam6d_fine_match(const float* f, int B, int n, float temp, const float* pts2, int* label1, int* label2, float* pred,
                     float* weight, void* ws, size_t ws_bytes, void* stream);
/* y = x W^T + b for M token rows of 256 channels on the panel kernel (the sparse-token projections: CoarsePointMatching's in_proj /
 * out_proj, PEM/model/coarse_point_matching.py:35-38, 61; [proj_k; proj_v] of a LinearAttention layer's memory tokens,
 * PEM/model/transformer.py:556-558).  wimage = sam6d_pack_panels(W, 32 npanels rows, k0 = 0, ksteps = 8, scale s), npanels 8 or 16
 * (256 or 512 outputs), inv_w_scale = 1 / s, bias may be null.  Row R = (cloud R / rows_per_cloud, token R % rows_per_cloud) is read
 * at row cloud * x_cloud_rows + x_row0 + token of x and written at row cloud * out_cloud_rows + out_row0 + token of out (32 npanels
 * floats per row): the bg slot of a token buffer is skipped in place on either side. */
int sam6d_rows_linear(const float* x, const void* wimage, int npanels, const float* bias, float inv_w_scale, float* out, long M,
                      int rows_per_cloud, long x_cloud_rows, long x_row0, long out_cloud_rows, long out_row0, void* stream);

/* sam6d_fine_match with the operands already prepared: sam6d_linear_norm_split computes y = x W^T + b for the M rows of x (M, 256), W as the
 * 8-panel image of sam6d_pack_panels (256 rows, k0 = 0, ksteps = 8, scale s; inv_w_scale = 1 / s) -- FinePointMatching's out_proj,
 * PEM/model/fine_point_matching.py:70-72 -- and writes fh | fl (M, 256) fp16 = hi / lo halves of (y / max(|y|, 1e-12)) * 2^10, the
 * F.normalize of compute_feature_similarity (PEM/utils/model_utils.py:141-142) and the operand split of the similarity product in one
 * pass; sam6d_fine_match_split takes those halves instead of f (same workspace size). */
int sam6d_linear_norm_split(const float* x, const void* wimage, const float* bias, float inv_w_scale, void* fh, void* fl, long M,
                            void* stream);
int sam6d_fine_match_split(const void* fh, const void* fl, int B, int n, float temp, const float* pts2, int* label1, int* label2,
                           float* pred, float* weight, void* ws, size_t ws_bytes, void* stream);
/* Fine soft-assignment reduction (PEM/utils/model_utils.py:325-331): pred (B,R-1,3), weight (B,R-1). */
int sam6d_fine_assign(const float* att, int B, int R, int C, const float* rmax, const float* rsum, const float* cmax,
                      const float* csum, const int* label1, const int* label2, const float* pts2, float* pred,
                      float* weight, void* stream);
/* replaces weighted_procrustes (PEM/utils/model_utils.py:343-436; CustomSVD/CustomDet :469-526); weights may be NULL. */
int sam6d_weighted_procrustes(const float* src, const float* ref, const float* weights, int B, int N,
                              float weight_thresh, float eps, float* R, float* t, void* stream);
/* Fine pose score and translation rescale (PEM/utils/model_utils.py:331-339; PEM/model/fine_point_matching.py:78);
 * t is scaled in place by (radius + 1e-6); cnt_ws (2*B) f32 scratch. */
int sam6d_fine_score(const float* pts1, const float* R, float* t, const float* model, const float* radius,
                     const int* label1, int B, int N, int P, float dis_thres, float* cnt_ws, float* score, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * B3: ISM template scoring (Instance_Segmentation_Model methods + model.loss classes).
 * ---------------------------------------------------------------------------------------------------------- */

/* replaces PairwiseSimilarity.forward (ISM/model/loss.py:27-44): query (Nq,D), ref (No,Nt,D) -> scores (Nq,No,Nt) in [0,1]. */
int sam6d_ism_cosine(const float* query, const float* ref, int Nq, int No, int Nt, int D, float* scores, void* stream);
/* replaces the tail of compute_semantic_score + best_template_pose (ISM/model/detector.py:198-207, 265-296):
 * per query the aggregated score (mode 0 avg_5 / 1 mean / 2 max), arg-max object and its best template; `sel` = ascending
 * indices of the queries with score > thresh, *nsel their count (device int).  0 <= Nq <= 65535 (SAM's 32 x 32 point grid
 * yields up to 3072 raw proposals), Nt <= 256; ties: the first maximal template, the first maximal object; avg_5 is the mean of the
 * min(5, Nt) largest scores, equal values counted once each. */
int sam6d_ism_semantic(const float* scores, int Nq, int No, int Nt, int mode, float thresh, float* sem, int* obj, int* best,
                       int* sel, int* nsel, void* stream);
/* sam6d_ism_semantic with the survivors written out compacted as the tensors the reference's caller holds after its boolean-mask
 * indexing (ISM/model/detector.py:284-296, best_template_pose :198-207): sel / obj_sel / best_sel (Nq) i64, sem_sel (Nq) f32, the first
 * nsel[0] entries valid; sem_ws / obj_ws / best_ws (Nq) are per-query scratch. */
int sam6d_ism_semantic_compact(const float* scores, int Nq, int No, int Nt, int mode, float thresh, float* sem_ws, int* obj_ws,
                               int* best_ws, long long* sel, long long* obj_sel, float* sem_sel, long long* best_sel, int* nsel,
                               void* stream);
/* replaces compute_straight + compute_visible_ratio reductions (ISM/model/loss.py:52-76) over sim (Ns,P,P). */
int sam6d_ism_patch_scores(const float* sim, const float* q_appe, int Ns, int P, int D, float thred, float* appe, float* vis,
                           void* stream);
/* compute_appearance_score + compute_visible_ratio (ISM/model/detector.py:298-308, 310-322; ISM/model/loss.py:52-76) WITHOUT the
 * (Ns,P,P) similarity tensor and without gathering the chosen templates' descriptors: proposal p multiplies query patches
 * q[qsel ? qsel[p] : p] (P,D) with ref[obj[p]][best[p]] (P,D) read in place (ref: (No,Nt,P,D)); the tile epilogue keeps row / column
 * maxima only.  sam6d_ism_patch_fused fills the workspace (sam6d_ism_patch_fused_workspace_bytes(Ns, P) bytes), sam6d_ism_patch_fused_scores
 * turns it into appe (Ns) and / or vis (Ns) for a threshold (either output may be NULL).  Descriptors must be L2-normalised rows
 * (|x| <= 1, as ISM/model/dinov2.py:322-324 produces them; masked patches all-zero); P a multiple of 128, D of 32; indices int64. */
size_t sam6d_ism_patch_fused_workspace_bytes(int Ns, int P);
int sam6d_ism_patch_fused(const float* q, const long long* qsel, const float* ref, const long long* obj, const long long* best, int Ns,
                          int Nt, int P, int D, void* ws, size_t ws_bytes, void* stream);
int sam6d_ism_patch_fused_scores(const void* ws, int Ns, int P, float thred, float* appe, float* vis, void* stream);
/* replaces project_template_to_image + Calculate_the_query_translation (ISM/model/detector.py:209-246,
 * ISM/utils/trimesh_utils.py:77-105): masks (Ns,H,W) f32, depth (H,W) i32, K (3,3) f64, poses (Nt,4,4) f32,
 * pointcloud (No,Npc,3) -> image_vu (Ns,Npc,2) i32, xyxy (Ns,4) i32, translate (Ns,3); part_ws (Ns*64*4) f64 scratch. */
int sam6d_ism_project(const float* masks, const int* depth, const double* K, double depth_scale, const float* poses,
                      const float* pointcloud, const int* best, const int* obj, int Ns, int H, int W, int Npc,
                      double* part_ws, int* image_vu, int* xyxy, float* translate, void* stream);
/* sam6d_ism_project with the masks read IN PLACE as a 16-byte-per-lane stream (same call sites: ISM/model/detector.py:209-246,
 * ISM/utils/trimesh_utils.py:77-105): masks (Nq,H,W) with mask_bytes = 1 (uint8 / bool, non-zero = inside: SAM's binary proposals) or
 * 4 (float32, as Detections.masks holds them, ISM/model/utils.py:80-95); mask_index (Ns) i64 or NULL: proposal i uses mask
 * mask_index[i] -- the class-token selection of detector.py:289-296 applied without the gathered (Ns,H,W) copy Detections.filter makes.
 * The masked-depth sums are exact integer sums in float64 and the divisions by fx / fy happen once per proposal.  The fast path needs
 * W % 16 == 0, depth_scale > 0 and 16-byte aligned masks / depth; otherwise float32 masks without an index fall back to
 * sam6d_ism_project.  part_ws: sam6d_ism_project_workspace_doubles(Ns, H, W) doubles. */
size_t sam6d_ism_project_workspace_doubles(int Ns, int H, int W);
int sam6d_ism_project2(const void* masks, int mask_bytes, const long long* mask_index, const int* depth, const double* K,
                       double depth_scale, const float* poses, const float* pointcloud, const int* best, const int* obj, int Ns, int H,
                       int W, int Npc, double* part_ws, int* image_vu, int* xyxy, float* translate, void* stream);

/* replaces depth_image_to_pointcloud_translate_torch(depth, scale, K) itself (ISM/utils/trimesh_utils.py:77-105) for a direct caller:
 * masked_depth (N,H,W) f32 = N already-masked depth maps (mm), K (3,3) f64 row-major, -> translate (N,3) f32 = the mean back-projected
 * point of each map over its pixels with Z > 0; float64 per-pixel terms and sums like the reference's real caller, divided by the fp32
 * count + 1e-8f (how torch evaluates the reference's int64 count + 1e-8; sam6d_ism_project / _project2 likewise).  part_ws: N * 64 * 4 doubles of scratch.  One launch pair for all maps. */
int sam6d_ism_translate_maps(const float* masked_depth, const double* K, double depth_scale, int N, int H, int W, double* part_ws,
                             float* translate, void* stream);
/* replaces compute_iou (ISM/utils/bbox_utils.py:197-222): boxes (Ns,4) int64; *all_positive = 0 when any pair has a
 * non-positive overlap (the reference then returns the scalar 0.0). */
int sam6d_ism_iou(const int* xyxy, const long long* boxes, int Ns, float* iou, int* all_positive, void* stream);
/* final score (ISM/model/detector.py:384): (sem[sel] + appe + geo*vis) / (2 + vis); geo NULL = the scalar-0.0 IoU case. */
int sam6d_ism_final_score(const float* sem, const float* appe, const float* geo, const float* vis, const int* sel, int Ns,
                          float* out, void* stream);
/* sam6d_ism_final_score (ISM/model/detector.py:384) with the IoU quirk of ISM/utils/bbox_utils.py:214-220 decided on the DEVICE: geo is
 * used only while all_positive[0] (the flag sam6d_ism_iou leaves) is non-zero, else the geometric term is 0 for every proposal -- no host
 * read-back between the IoU and the final score. */
int sam6d_ism_final_score_flag(const float* sem, const float* appe, const float* geo, const float* vis, const int* all_positive, int Ns,
                               float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Rows SURVEY 8f marks "next" (callers either side of the path).
 * ---------------------------------------------------------------------------------------------------------- */

/* replaces the radius normalisation of ViTEncoder.forward (PEM/model/feature_extraction.py:133-137):
 * radius (B) = max_n |dense_po[b,n]|; po_out = dense_po / (radius + 1e-6); pm_out = pts / (radius + 1e-6). */
int sam6d_radius_normalize(const float* dense_po, const float* pts, int B, int Npo, int Npm, float* radius, float* po_out,
                           float* pm_out, void* stream);
/* replaces the masked patch-descriptor post-processing of CustomDINOv2 (ISM/model/dinov2.py:265-269, 322-324):
 * out = F.normalize(feats * [AvgPool2d(patch)(masks) > thresh], dim=-1); feats (N,P,D), masks (N,H,W) f32. */
int sam6d_masked_patch_normalize(const float* feats, const float* masks, int N, int P, int D, int H, int W, int patch,
                                 float thresh, float* out, void* stream);
/* replaces get_point_cloud_from_depth (PEM/utils/data_utils.py:92-110) on a resident depth map (H,W) f32, metres:
 * cloud (r1-r0, c1-c0, 3) for the crop bbox [rmin=r0, rmax=r1, cmin=c0, cmax=c1] (the whole image: 0,H,0,W).  An empty
 * window writes nothing and accepts a null cloud. */
int sam6d_depth_to_cloud(const float* depth, int H, int W, int r0, int r1, int c0, int c1, float fx, float fy, float cx,
                         float cy, float* cloud, void* stream);
/* replaces the test of Detections.remove_very_small_detections (ISM/model/utils.py:96-102): keep[i] (u8) =
 * box_area(boxes[i]) / (H*W) > thr_box && masks[i].sum() / (H*W) > thr_mask; boxes (N,4) int64 xyxy, masks (N,H,W) f32.
 * thr_box = min_box_size**2, thr_mask = min_mask_size. */
int sam6d_detections_small_keep(const long long* boxes, const float* masks, int N, int H, int W, float thr_box,
                                float thr_mask, unsigned char* keep, void* stream);
/* boolean-mask indexing (ISM/model/utils.py:104-105): idx (N) i64 = positions of the non-zero keep bytes, count[0] = K.
 * Nothing is written to idx beyond K; N == 0 accepts a null keep and gives K = 0. */
int sam6d_mask_to_indices(const unsigned char* keep, int N, long long* idx, int* count, void* stream);
/* replaces `getattr(self, key)[idxs]` of Detections.filter / apply_nms* (ISM/model/utils.py:105,119,126,190) for a
 * tensor of any dtype: dst[j,:] = src[idx[j],:], rows of row_bytes bytes, idx (M) i64 (negative = from the end;
 * out-of-range rows come back zero). */
int sam6d_take_rows(const void* src, const long long* idx, long n_src, int M, long row_bytes, void* dst, void* stream);
/* replaces mask_to_rle(force_binary_mask(mask)) of convert_npz_to_json, the `segmentation` field of detection_ism.json
 * (ISM/model/utils.py:25-43, 199-216; ISM/utils/bbox_utils.py:190-192): uncompressed COCO RLE of (mask > 0), runs counted in
 * column-major order starting with the zero run.  masks (N,H,W) f32.  Two calls: nruns[i] (N) i32 = number of counts of
 * mask i; then, with offsets (N+1) i64 = exclusive prefix sum of nruns, counts[offsets[i] .. offsets[i+1]) i32 = its runs
 * (a mask whose offsets do not match its run count is left unwritten). */
int sam6d_mask_rle_count(const float* masks, int N, int H, int W, int* nruns, void* stream);
int sam6d_mask_rle_encode(const float* masks, int N, int H, int W, const long long* offsets, int* counts, void* stream);
/* the inverse, as PEM's get_test_data reads the file back (cocomask.decode of an uncompressed RLE,
 * PEM/run_inference_custom_pytorch.py:308-317; same format as ISM/segment_anything/utils/amg.py:138-150):
 * masks (N,H,W) u8 from counts / offsets as above; ws_ends = i32 scratch as long as counts.  Positions beyond the
 * encoded runs come back 0. */
int sam6d_mask_rle_decode(const int* counts, const long long* offsets, int N, int H, int W, int* ws_ends,
                          unsigned char* masks, void* stream);
/* replaces torchvision.ops.nms as Detections.apply_nms (ISM/model/utils.py:121-124, group == NULL) and
 * apply_nms_per_object_id (:107-117, group = object_ids) call it: boxes (N,4) f32 xyxy, scores (N) f32.
 * keep_idx (N) i64 receives the surviving indices, ids ascending, score descending inside an id (stable); count[0] = K.
 * Inside an id the order is torch.sort(descending=True, stable=True)'s: a NaN score of either sign before every number,
 * equal scores (-0 equals +0) by the lower index.  It is total, so keep_idx[:K] holds distinct indices in [0, N) for any
 * scores.  A NaN IoU (0/0 of two empty boxes, NaN coordinates) never suppresses: the test is IoU > thresh.
 * ws: sam6d_nms_workspace_bytes(N) bytes of device memory. */
size_t sam6d_nms_workspace_bytes(int N);
int sam6d_nms(const float* boxes, const float* scores, const long long* group, int N, float thresh, long long* keep_idx,
              int* count, void* ws, size_t ws_bytes, void* stream);
/* Proposal geometry of get_test_data (PEM/run_inference_custom_pytorch.py:316-355) on resident data; masks (N,H,W) u8, depth (H,W)
 * f32 metres.
 * sam6d_mask_bbox: bbox (N,4) i32 = get_bbox((mask > 0) & (depth > 0)) (PEM/utils/data_utils.py:125-160), count (N) valid pixels.
 * sam6d_crop_masked_points: the valid pixels of each crop in row-major order: choose (N,cap) i32 flat crop indices, cloud (N,cap,3)
 *   back-projected points (get_point_cloud_from_depth, data_utils.py:92-110), n_valid (N) (:326-330).
 * sam6d_radius_filter: in-place removal of the points farther than radius * 1.2 from their mean (:331-337); n_keep (N), center (N,3).
 * sam6d_choose_points: pts (N,ns,3) = cloud[sel], rgb_choose (N,ns) i64 = get_resize_rgb_choose(choose[sel], bbox, img_size)
 *   (data_utils.py:113-123); sel (N,ns) i32 is the caller's np.random.choice (:339-345). */
int sam6d_mask_bbox(const unsigned char* masks, const float* depth, int N, int H, int W, int* bbox, int* count, void* stream);
int sam6d_crop_masked_points(const unsigned char* masks, const float* depth, int N, int H, int W, const int* bbox, float fx, float fy,
                             float cx, float cy, int cap, int* choose, float* cloud, int* n_valid, void* stream);
int sam6d_radius_filter(int N, int cap, const int* n_valid, float radius, int* choose, float* cloud, int* n_keep, float* center,
                        void* stream);
int sam6d_choose_points(int N, int cap, const int* choose, const float* cloud, const int* bbox, const int* sel, int ns, int img_size,
                        float* pts, long long* rgb_choose, void* stream);
/* Template geometry of _get_template (PEM/run_inference_custom_pytorch.py:199-219); masks (T,H,W) u8, one per render.
 * sam6d_template_bbox: bbox (T,4) i32 = get_bbox(mask == 255) (:201-203, PEM/utils/data_utils.py:125-160), no depth condition;
 *   count (T) = mask pixels in the image.
 * sam6d_template_crop_points: the mask pixels of each crop in row-major order (:214): choose (T,cap) i32 flat crop indices,
 *   xyz (T,cap,3) f32 = xyz_mm[y1:y2, x1:x2] / 1000 (:200, :219) with xyz_mm (T,H,W,3) f32, n_valid (T) = min(count in crop, cap).
 *   The caller's choice (:215-218) then goes through sam6d_choose_points (xyz[sel] and get_resize_rgb_choose, :221). */
int sam6d_template_bbox(const unsigned char* masks, int T, int H, int W, int* bbox, int* count, void* stream);
int sam6d_template_crop_points(const unsigned char* masks, const float* xyz_mm, int T, int H, int W, const int* bbox, int cap, int* choose,
                               float* xyz, int* n_valid, void* stream);
/* The random choice of get_test_data (PEM/run_inference_custom_pytorch.py:337-340) and of _get_template (:215-218),
 * np.random.choice(np.arange(n), ns, replace = n > ns), drawn on the device for N rows at once.  NOT numpy's stream: a counter-based
 * draw with an integer definition of its own, equal to the reference in distribution only.  All arithmetic modulo 2^32:
 *   fmix(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
 *   a = fmix(seed ^ 0x9E3779B9), b = fmix(a + row), h(r) = fmix(fmix(r ^ b) + a), row = row0 + i for row i of this call.
 * n (N) i32 on the device (n_keep of sam6d_radius_filter, n_valid of sam6d_template_crop_points), sel (N,ns) i32, ready for
 * sam6d_choose_points.  n[i] > ns: the ns values r in [0, n[i]) with the smallest h(r), in ascending order of h (distinct);
 * 1 <= n[i] <= ns: sel[i, j] = (h(j) * n[i]) >> 32 with the 64-bit product; n[i] <= 0: zeros.  n[i] above 2^24 counts as 2^24.
 * A function of (seed, row, n[i], ns) alone.  1 <= ns <= 8192 (the chosen pairs are sorted in 64 KB of LDS) and N >= 0, anything else
 * returns non-zero without a launch; N == 0 is a no-op, also with null pointers. */
int sam6d_draw_choice(const int* n, int N, int ns, unsigned seed, unsigned row0, int* sel, void* stream);
/* The rgb input (PEM/run_inference_custom_pytorch.py:344-350 proposals, :207-212 templates): img[y1:y2, x1:x2][:, :, ::-1], times the
 * mask bit, cv2.resize to (img_size, img_size) with INTER_LINEAR (OpenCV 4.x fixed point, restated; a 2*img_size crop takes OpenCV's
 * INTER_AREA fast path), then ToTensor + Normalize (:151-153).  N items in one launch.
 * images: (H,W,channels) u8 per item at byte stride image_stride (0: all items share one image); channels 1 (grayscale, as :293-294)
 * or 3.  bbox (N,4) i32 = (y1, y2, x1, x2).  mask_mode 0: no mask (rgb_mask_flag False); 1: (masks[i] > 0) & (depth > 0) (:318);
 * 2: masks[i] == 255 (:201).  masks (N,H,W) u8, depth (H,W) f32.
 * out (N,3,img_size,img_size) f32; out_u8 (N,img_size,img_size,3) u8 the resized crops, or NULL; status (N) i32, or NULL: 1 where
 * bbox[i] is not inside the image (that item is written as an all-masked crop), else 0.  img_size <= 1024; W <= 8191. */
int sam6d_rgb_crop_resize(const unsigned char* images, long image_stride, int channels, int H, int W, const unsigned char* masks,
                          const float* depth, int mask_mode, int N, const int* bbox, int img_size, float* out, unsigned char* out_u8,
                          int* status, void* stream);

/* ViT-B/16 image encoder of the feature extraction (PEM/model/feature_extraction.py:21-35, :98-118, :141-142); the residual stream is
 * X (B*197, 768) f32 row-major, row 0 of each image the cls token.  The dense projections are sam6d_gemm_nt / _w16 (fc1 with act 2).
 * sam6d_vit_patch_rows: images (B,3,224,224) -> A (B*196, 768), row 14 py + px = the 16 x 16 patch in the Conv2d weight's (c, kh, kw)
 *   order (patch_embed.proj, feature_extraction.py:21-35), and the cls rows X[197 b] = cls_token + pos_embed[0] (768 floats each). */
int sam6d_vit_patch_rows(const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B, void* stream);
/* nn.LayerNorm(768, eps) over `rows` rows of each of nimg images (feature_extraction.py:21-35 norm1 / norm2 / norm): row r of image b
 * is x + b sx + r ldx -> y + b sy + r ldy (floats; strides multiples of 4, pointers 16-byte aligned).  Also writes the pyramid taps
 * into their concat buffer (:98-118). */
int sam6d_vit_layernorm768(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx, long sx,
                           long ldy, long sy, float eps, void* stream);
/* Multi-head self-attention of a ViT-B block (feature_extraction.py:21-35): qkv (B*n, 2304) = [q | k | v], head h at columns
 * 64h .. 64h+63 of each part -> out (B*n, 768) = softmax(q_h k_h^T / 8) v_h per head, in x.transpose(1,2).reshape(B,n,768) order.
 * n <= 208.  fp16 x3 split MFMA products with power-of-two operand scales (fp32 softmax); the probabilities stay on chip. */
int sam6d_vit_attention(const float* qkv, float* out, int B, int n, void* stream);
/* output_upscaling -> F.interpolate(56 -> 224, bilinear, align_corners=False) -> get_chosen_pixel_feats (feature_extraction.py:98-118,
 * PEM/utils/model_utils.py:86-98) without the dense map: U (B*196, 4096) = the output_upscaling GEMM output (bias included),
 * choose (B,N) i64 pixel indices -> out (B,N,256).  An index outside [0, 224*224) yields a NaN row. */
int sam6d_vit_upsample_gather(const float* U, const long long* choose, float* out, int B, int N, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ISM's proposal descriptors: CropResizePad and the DINOv2 ViT-L/14 (ISM/model/dinov2.py:115-326).  The residual stream is
 * X (N*257, 1024) f32 row-major, row 0 of each image the cls token; the dense projections are sam6d_gemm_nt / _w16 (fc1 with act 2,
 * LayerScale folded into the proj / fc2 weights by the caller).  (New entries only: no existing signature or buffer layout changed,
 * so SAM6D_ABI_VERSION stays.)
 * ---------------------------------------------------------------------------------------------------------- */

/* process_rgb_proposals + process_masks_proposals (ISM/model/dinov2.py:160-173, :221-232) through CropResizePad(224)
 * (ISM/utils/bbox_utils.py:89-126) for all N proposals in one launch: ToTensor + Normalize(mean 0.485/0.456/0.406, std
 * 0.229/0.224/0.225) of image (H,W,3) u8, times masks[i] (N,H,W) f32, the crop boxes[i] = (x1, y1, x2, y2) i64 with exclusive ends,
 * F.interpolate(scale_factor = 224 / max(box side), formed as torch does: fl32(1 / side) * 224) in nearest mode, zero padding to 224 x 224 (top / left get
 * max((224 - side) // 2, 0)) and the second interpolate.  out_rgb (N,3,224,224) f32 and out_mask (N,224,224) f32 (the same gather
 * of the mask); either may be NULL, and image too when out_rgb is.  Bit-exact: every source index is the one torch computes.  Boxes are expected inside the image
 * (they are clipped to it; Python's negative-index wrap is not reproduced); a box whose resized crop is empty, which raises in the
 * reference, gives an all-zero crop.  A square resized crop has side 223 or 224 for every box side, and the second interpolate of
 * side 223 gives 224 pixels in torch too, so no box makes the output size differ from the reference's.  N <= 65535. */
int sam6d_dino_crop_proposals(const unsigned char* image, const float* masks, const long long* boxes, int N, int H, int W,
                              float* out_rgb, float* out_mask, void* stream);
/* PatchEmbed + cls token of prepare_tokens_with_masks (ISM/model/vision_transformer.py:209-216): images (B,3,224,224) -> A (B*256, 608),
 * row 16 py + px = the 14 x 14 patch in the Conv2d weight's (c, kh, kw) order (588 values) followed by 20 zeros (K padded to 19
 * k-steps of 32; the packed weight's columns 588..607 are zero too), and the cls rows X[257 b] = cls_token + pos_embed[0]
 * (1024 floats each; pos_embed already interpolated to the 16 x 16 grid). */
int sam6d_dino_patch_rows(const float* img, const float* cls_token, const float* pos_embed, float* A, float* X, int B, void* stream);
/* nn.LayerNorm(1024, eps) over `rows` rows of each of nimg images (ISM/model/layers/block.py:82-98 norm1 / norm2,
 * vision_transformer.py:259-265 norm): row r of image b is x + b sx + r ldx -> y + b sy + r ldy (floats; strides multiples of 4,
 * pointers 16-byte aligned), so the final norm writes x_norm_clstoken and x_norm_patchtokens straight into their own tensors. */
int sam6d_dino_layernorm1024(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx, long sx,
                             long ldy, long sy, float eps, void* stream);
/* Multi-head self-attention of a DINOv2 ViT-L block (ISM/model/layers/attention.py:49-62): qkv (B*n, 3072) = [q | k | v], head h at
 * columns 64h .. 64h+63 of each part -> out (B*n, 1024) = softmax(q_h k_h^T / 8) v_h per head, 16 heads, in
 * x.transpose(1,2).reshape(B,n,1024) order.  n <= 272 (the 257 tokens of a 224 x 224 image are not padded: the key tail is masked in
 * the kernel).  fp16 x3 split MFMA products with power-of-two operand scales (fp32 softmax); the probabilities stay on chip. */
int sam6d_dino_attention(const float* qkv, float* out, int B, int n, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SAM's automatic mask generator after the mask decoder (ISM/model/sam.py:52-148 CustomSamAutomaticMaskGenerator,
 * ISM/segment_anything/automatic_mask_generator.py:266-321).  The network itself (image encoder, prompt encoder, mask decoder) is not
 * part of the library.  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ---------------------------------------------------------------------------------------------------------- */

/* Sam.postprocess_masks (ISM/segment_anything/modeling/sam.py:133-162), calculate_stability_score
 * (ISM/segment_anything/utils/amg.py:156-176), the `> mask_threshold` of _process_batch (automatic_mask_generator.py:308) and
 * batched_mask_to_box (amg.py:303-346) for one point batch, without the S x S or the full-resolution logits in memory:
 * low (M, lh, lw) f32 low-resolution logits -> for every mask with live[m] != 0 (u8) and every pixel of the out_h x out_w crop the
 * value of F.interpolate(F.interpolate(low, (S, S))[..., :in_h, :in_w], (out_h, out_w)) (bilinear, align_corners=False; the fp32
 * recipe is written down in csrc/amg.hip and does not depend on the tiling), and from it
 *   n_hi[m], n_lo[m] (i32) = pixels > mask_threshold + offset and > mask_threshold - offset (stability score = n_hi / n_lo),
 *   area[m] (i32) and box[m] = (x0, y0, x1, y1) (i32, inclusive; [0, 0, 0, 0] for an empty mask) of the pixels > mask_threshold,
 *   bits (M, out_h, ceil(out_w / 32)) u32: that binary mask, pixel x of a row in bit x % 32 of word x / 32 (unused bits 0),
 *   logits_out (M, out_h, out_w) f32: the values themselves; NULL in the product path (a test measures the arithmetic with it).
 * Rows with live[m] == 0 are left untouched in every output.  M <= 65535; in_h, in_w <= S.
 * ws: sam6d_amg_mask_stats_workspace_bytes(M, lh, lw, S, in_h, out_h) bytes of device memory (per-band partial results; 0 = sizes
 * the entry refuses). */
size_t sam6d_amg_mask_stats_workspace_bytes(int M, int lh, int lw, int S, int in_h, int out_h);
int sam6d_amg_mask_stats(const float* low, const unsigned char* live, int M, int lh, int lw, int S, int in_h, int in_w, int out_h,
                         int out_w, float mask_threshold, float stability_score_offset, int* n_hi, int* n_lo, int* area, int* box,
                         unsigned* bits, float* logits_out, void* ws, size_t ws_bytes, void* stream);
/* replaces uncrop_masks + mask_to_rle_pytorch (ISM/segment_anything/utils/amg.py:255-264, :107-135) and the rle_to_mask loop with its
 * torch.stack and upload (ISM/model/sam.py:146-148) for the masks that survived: out[k] (K, H, W), u8 or (as_f32 != 0) f32, 0 / 1, =
 * row idx[k] (i64) of bits (n_src, out_h, ceil(out_w / 32)) placed at (x0, y0) of the H x W image, zero outside the crop.  An index
 * outside [0, n_src) gives an all-zero mask.  K <= 65535. */
int sam6d_amg_unpack_masks(const unsigned* bits, const long long* idx, long n_src, int K, int out_h, int out_w, int x0, int y0,
                           int H, int W, int as_f32, void* out, void* stream);

/* 8-connected component labelling of K binary masks, what cv2.connectedComponentsWithStats(.., 8) is asked for in remove_small_regions
 * (ISM/segment_anything/utils/amg.py:267-291), in a canonical form: masks (K, H, W) u8, foreground = masks != 0 (invert == 0) or
 * masks == 0 (invert != 0);
 *   labels (K, H, W) i32 = 0 off the foreground, else 1 + the smallest row-major pixel index (y * W + x) of the pixel's component,
 *   areas  (K, H, W) i32 = the pixel count of the pixel's component, 0 off the foreground.
 * The result is a function of the mask alone (it does not depend on scheduling).  1 <= K <= 65535, H * W <= 2^31 - 2.
 * ws: sam6d_mask_components_workspace_bytes(K, H, W) bytes of device memory (two i32 planes; 0 = sizes the entry refuses).
 * (New entries only, so SAM6D_ABI_VERSION stays.) */
size_t sam6d_mask_components_workspace_bytes(int K, int H, int W);
int sam6d_mask_components(const unsigned char* masks, int K, int H, int W, int invert, int* labels, int* areas, void* ws,
                          size_t ws_bytes, void* stream);
/* replaces the per-mask host loop of postprocess_small_regions (ISM/segment_anything/automatic_mask_generator.py:324-372) with its two
 * remove_small_regions calls (ISM/segment_anything/utils/amg.py:267-291) and the batched_mask_to_box after it (amg.py:303-346): masks
 * (K, H, W) u8 are cleaned in place to 0 / 1.  First every 8-connected component of ~m with fewer than min_area pixels is filled
 * (components that touch the image border included), then, on that result, m becomes the union of its components with at least
 * min_area pixels, or, if there is none, its largest component (among equals the one whose first pixel in row-major order comes
 * first: the library's rule, cv2's label numbering decides in the reference).  A pass that finds no component below min_area leaves
 * the mask as it is.  changed (K) u8 = 1 where either pass found one; box (K, 4) i32 = (x0, y0, x1, y1) of the cleaned mask
 * (inclusive; [0, 0, 0, 0] for an empty mask).  1 <= K <= 65535, H * W <= 2^31 - 2, min_area >= 1 (a size s is below a float
 * threshold t exactly when s < ceil(t): the caller passes the ceiling).
 * ws: sam6d_amg_small_regions_workspace_bytes(K, H, W) bytes of 8-byte aligned device memory (0 = sizes the entry refuses). */
size_t sam6d_amg_small_regions_workspace_bytes(int K, int H, int W);
int sam6d_amg_small_regions(unsigned char* masks, int K, int H, int W, int min_area, unsigned char* changed, int* box, void* ws,
                            size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The two resizes of `segmentor_width_size` round the mask generator (ISM/model/sam.py:77-100; csrc/segresize.hip).  Both refuse
 * without a launch: a non-zero return writes nothing.  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ---------------------------------------------------------------------------------------------------------- */

/* preprocess_resize (ISM/model/sam.py:77-83): dst (h, w, 3) u8, contiguous, = cv2.resize(src, (w, h)) with the default INTER_LINEAR of a
 * CV_8UC3 image as OpenCV 4.x computes it (imgproc/src/resize.cpp: 11-bit fixed point, the vectorised vertical pass for every column;
 * the recipe is written down in csrc/rgbprep.hip).  Pixel (y, x) of src is at src + y row_stride + 3 x (bytes, row_stride >= 3 W: a
 * crop view is read in place).  H == 2 h and W == 2 w is OpenCV's INTER_AREA fast path, the rounded 2 x 2 mean; equal sizes copy.
 * H, W, h, w 1 .. 4096 (h = int(width * H / W) can be 0, where cv2 raises: refused); channels must be 3; dst must not overlap src. */
int sam6d_image_resize_linear(const unsigned char* src, long row_stride, int H, int W, int channels, unsigned char* dst, int h, int w,
                              void* stream);
/* postprocess_resize (ISM/model/sam.py:85-100), its masks: masks (K, h, w) u8, any non-zero byte = 1 (a bool tensor's bytes) -> out
 * (K, H, W) f32, contiguous, = F.interpolate(masks.unsqueeze(1).float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0],
 * enlarging or shrinking (two taps per axis, no antialiasing): upsample_bilinear2d's fp32 expression, written down in
 * csrc/segresize.hip, a function of (mask, y, x) alone.  K 0 .. 65535 (0: no launch), sizes 1 .. 8192, out 4-byte aligned (16 bytes
 * and W % 4 == 0 for 16-byte stores).  K H W may pass 2^31. */
int sam6d_masks_resize_bilinear(const unsigned char* masks, int K, int h, int w, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SAM's mask decoder for point prompts (ISM/segment_anything/modeling/mask_decoder.py:112-149, its TwoWayTransformer
 * ISM/segment_anything/modeling/transformer.py:62-106): what lies between the dense projections over the P x 4096 image rows, which are
 * sam6d_gemm_nt / _w16 launches.  Specialised for transformer_dim 256, 8 heads, 7 tokens per prompt and a 64 x 64 grid: every entry
 * takes (dim, heads, tokens, grid_h, grid_w) and refuses anything else without a launch.  fp32 throughout.  P <= 65535.
 * (New entries only, so SAM6D_ABI_VERSION stays.)
 * ---------------------------------------------------------------------------------------------------------- */

/* The image -> token half of a TwoWayAttentionBlock (ISM/segment_anything/modeling/transformer.py:175-180, Attention.forward :218-240)
 * with out_proj folded into the values: q (row n of prompt p at q + p sq + n ldq, 128 floats; sq = 0: one table for every prompt) is
 * q_proj(keys + key_pe); ktok (P,7,128) = k_proj(queries + query_pe); fold (P,56,256), row 8 j + h = out_proj.weight[:, 16h:16h+16] .
 * v_proj(queries)[j, 16h:16h+16]; bias (256) = out_proj.bias.  Per image row: 8 x 7 scores / 4, softmax over the 7 tokens of each head,
 * the 56 -> 256 contraction, + bias + keys (row n of prompt p at keys + p skeys + 256 n; skeys = 0: the same image rows for every
 * prompt, as in layer 0), norm4 = LayerNorm(256, eps) with gamma / beta -> out (P,4096,256).  Neither the probabilities nor a
 * 128-wide attention output reach memory.  q, out, gamma, beta 16-byte aligned, ldq and sq multiples of 4. */
int sam6d_samdec_image_to_token(const float* q, long ldq, long sq, const float* ktok, const float* fold, const float* bias,
                                const float* keys, long skeys, const float* gamma, const float* beta, float eps, float* out, int P,
                                int dim, int heads, int tokens, int grid_h, int grid_w, void* stream);
/* The token -> image attention of a TwoWayAttentionBlock and the final one (ISM/segment_anything/modeling/transformer.py:163-167,
 * :100-102, Attention.forward :225-237) up to, not including, out_proj: q (P,7,128) = q_proj(queries + query_pe); k, v: row n of prompt p
 * at k + p skv + n ld and v + p skv + n ld (128 floats each; skv = 0: per-image tables shared by every prompt) -> out (P,7,128) =
 * softmax(q_h k_h^T / 4) v_h for the 8 heads of 16 channels, in _recombine_heads order.  The 4096 keys of a prompt are split over 32
 * workgroups that leave partial (max, sum, weighted v) in ws (sam6d_samdec_token_to_image_workspace_bytes(P) bytes); a second launch
 * merges them.  The scores do not reach memory.  k 16-byte aligned, ld and skv multiples of 4. */
size_t sam6d_samdec_token_to_image_workspace_bytes(int P);
int sam6d_samdec_token_to_image(const float* q, const float* k, const float* v, long ld, long skv, float* out, int P, int dim, int heads,
                                int tokens, int grid_h, int grid_w, void* ws, size_t ws_bytes, void* stream);
/* output_upscaling after its first ConvTranspose2d, and the mask product (ISM/segment_anything/modeling/mask_decoder.py:53-59, :137-144;
 * LayerNorm2d ISM/segment_anything/modeling/common.py:38-43) for multimask_output=True: ct1 (row n of prompt p at ct1 + p sp + n ld, 256
 * floats = sub-pixel 2 kh + kw times 64 channels, bias included) is ConvTranspose2d(256, 64, 2, 2) of the keys as a GEMM; per
 * sub-pixel LayerNorm2d over the 64 channels (biased variance, eps) and erf GELU, ConvTranspose2d(64, 32, 2, 2) with w2 (128,64), row
 * 32 (2 kh + kw) + o = weight[:, o, kh, kw], and b2 (128) = bias tiled, GELU, and the dot products with hyper (P,3,32) = hyper_in[:, 1:4]
 * -> low (P,3,256,256).  Image token (y, x) writes the 4 x 4 block at (4y, 4x).  Neither upscaled tensor reaches memory, and mask
 * token 0's map is not computed.  ct1 16-byte aligned, ld and sp multiples of 4. */
int sam6d_samdec_upscale_masks(const float* ct1, long ld, long sp, const float* ln_gamma, const float* ln_beta, float eps, const float* w2,
                               const float* b2, const float* hyper, float* low, int P, int dim, int heads, int tokens, int grid_h,
                               int grid_w, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SAM's ViT-H image encoder (ISM/segment_anything/modeling/image_encoder.py:17-116 ImageEncoderViT): what lies around the dense
 * projections, which are sam6d_gemm_nt / _w16 launches.  Specialised for a 1024 x 1024 image in 16 x 16 patches (a 64 x 64 token grid),
 * width 1280 in heads of 80, 14 x 14 windows and a neck to 256 channels; `heads` is an argument (the rows are 3 * 80 * heads wide) so
 * that a kernel can be run on a slice of the heads.  fp16 x3 split MFMA products with power-of-two operand scales, fp32 softmax, in
 * matmul modes 0 and 1 alike.  B <= 65535.  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ---------------------------------------------------------------------------------------------------------- */

/* PatchEmbed's Conv2d(3, 1280, 16, stride 16) as GEMM rows (image_encoder.py:387-395): img (B,3,1024,1024) -> A (B*4096, 768), row
 * 64 py + px = the patch's values in the weight's (c, kh, kw) order.  There is no cls row; pos_embed (image_encoder.py:108-109) is the
 * patch GEMM's residual. */
int sam6d_sam_patch_rows(const float* img, float* A, int B, void* stream);
/* nn.LayerNorm(1280, eps) of Block.norm1 / norm2 (image_encoder.py:151, 161, 168, 180); arguments as sam6d_vit_layernorm768. */
int sam6d_sam_layernorm1280(const float* x, const float* gamma, const float* beta, float* y, int nimg, int rows, long ldx, long sx,
                            long ldy, long sy, float eps, void* stream);
/* Attention.forward of a windowed Block between its qkv and proj Linears, with the window partition around it
 * (image_encoder.py:170-177, 224-237, window_partition :243-264, window_unpartition :267-289, add_decomposed_rel_pos :325-361):
 * qkv (B*4096, 3*80*heads) = [q | k | v] in image row order, head h at columns 80h .. 80h+79 of each part -> out (B*4096, 80*heads).
 * The grid is padded to 70 x 70 = 5 x 5 windows of 14 x 14 by index arithmetic.  A padded position is a key like any other: the
 * reference pads after norm1, so its token is zero and its k and v are the bias of the qkv Linear, pad_qkv (3*80*heads); it enters
 * every softmax of its window with its own relative-position terms, and is never a query.  Score of (query, key) in a window:
 * (q . k) / sqrt(80) + q . rel_h[qh - kh + 13] + q . rel_w[qw - kw + 13], the last two with the unscaled q; rel_h, rel_w (27, 80).
 * Neither a (B*25*196, ...) tensor nor the probabilities reach memory.  All pointers 16-byte aligned. */
int sam6d_sam_window_attention(const float* qkv, const float* pad_qkv, const float* rel_h, const float* rel_w, float* out, int B,
                               int heads, void* stream);
/* The same for a global Block (window_size 0; image_encoder.py:224-237, :325-361): 4096 queries x 4096 keys per (image, head), tables
 * rel_h, rel_w (127, 80) and offset 63; online softmax over tiles of 64 keys, neither scores nor probabilities reach memory.  The k
 * and v tiles are cut into fp16 halves by every workgroup that reads them: no workspace. */
int sam6d_sam_global_attention(const float* qkv, const float* rel_h, const float* rel_w, float* out, int B, int heads, void* stream);
/* The neck's Conv2d(256, 256, 3, padding 1, no bias) as a gather for one GEMM (image_encoder.py:96-102): x (B*4096, 256), the
 * channel-last 64 x 64 map -> rows (B*4096, 2304), columns 256 (3 ky + kx) + c of row (y, x) = x at (y + ky - 1, x + kx - 1), zeros
 * outside the grid.  The 1 x 1 convolution is a GEMM, LayerNorm2d (common.py:38-43) is sam6d_layernorm256 on channel-last rows (the
 * same biased variance) and the (B, 256, 64, 64) output is a sam6d_transpose.  B <= 4096. */
int sam6d_sam_neck_gather(const float* x, float* rows, int B, void* stream);

#define SAM6D_SAM_FRONT_X 0    /* the `layout` argument of sam6d_sam_front */
#define SAM6D_SAM_FRONT_ROWS 1
/* SAM's image front in one launch: B uint8 images (H, W, 3) of one size -> what the image encoder is called on.  That is
 * ResizeLongestSide.apply_image (ISM/segment_anything/utils/transforms.py:26-31, get_preprocess_shape :91-102: the longest side to
 * `side` through torchvision's resize of a PIL image, i.e. Pillow's 8-bit bilinear ImagingResample), the predictor's channel flip
 * for another image_format (ISM/segment_anything/predictor.py:56-58; reverse != 0 reads channel 2 - c) and Sam.preprocess
 * (ISM/segment_anything/modeling/sam.py:164-173): (x - mean) / std in fp32, zeros below and to the right up to side x side.
 * Pixel (y, x) of image b is at img + b image_stride + y row_stride + 3 x (strides in bytes, row_stride >= 3 W: a crop view works).
 * xtab (for W -> ow) and ytab (for H -> oh), int32 in device memory, are Pillow's fixed-point coefficients, computed on the host in
 * double: for an axis with n outputs and t = xtaps / ytaps table columns, lo[n] (first source index), count[n], k[n][t] (22-bit
 * coefficients, zeros behind the count).  A pass is byte = min((2^21 + sum_j pixel[lo + j] k[j]) >> 22, 255), horizontal first,
 * rounded to a byte before the vertical pass; the intermediate image stays in LDS.  Always horizontal first: Pillow's Image.resize
 * (12.2.0) runs the vertical pass first for H > 100 W when the image shrinks vertically, which the caller has to keep away.  Indices
 * derived from the tables are clamped to the buffers.
 * layout SAM6D_SAM_FRONT_X: out (B, 3, side, side), Sam.preprocess's tensor.  SAM6D_SAM_FRONT_ROWS: out (B * (side / 16)^2, 768), what
 * sam6d_sam_patch_rows makes of that tensor (row (side / 16) py + px, columns in (c, kh, kw) order; image_encoder.py:387-395) without
 * the tensor.  H, W 1 .. 4096; side a multiple of 16, 16 .. 1024; at most 9 taps per axis (shrinking by up to 4); out 16-byte
 * aligned; B <= 65535.  Anything else returns non-zero without a launch.  (A new entry, so SAM6D_ABI_VERSION stays.) */
int sam6d_sam_front(const unsigned char* img, long row_stride, long image_stride, int B, int H, int W, int reverse, const int* xtab,
                    int xtaps, const int* ytab, int ytaps, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                    int side, float* out, int layout, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Onboarding a CAD model (Render/render_custom_templates.py): rendered templates and surface samples
 * ------------------------------------------------------------------------------------------------------------ */
/* The template renderer's part of Render/render_custom_templates.py:55-106 (BlenderProc's render() and render_nocs() per camera pose)
 * as a deterministic triangle rasteriser: T views of one mesh in one call.  The geometry is defined by the recipe at the top of
 * csrc/raster.hip and is bitwise reproducible; the shading of rgb is the package's own (parity unpinned against Cycles).
 * vertices (V,3) f32 in CAD units, faces (F,3) i32, normals (V,3) f32 or NULL (then the face normal shades), colors (V,3) u8 or NULL,
 * view (T,3,4) f32 row-major object -> camera matrices (x right, y down, z forward), light (T,3) f32 in the camera frame, pinhole
 * intrinsics fx fy cx cy in pixels (pixel (i, j) has its centre at (j + 0.5, i + 0.5)), near > 0, base_color the grey albedo used when
 * colorize != 0 or colors is NULL, srgb_lut 4096 u8 on the device (the sRGB transfer of k / 4095, built on the host), wave_area: a
 * face whose clamped bounding box has at least this many pixels is rasterised by a whole wave, 0 = the default (256).
 * Outputs: mask (T,H,W) u8 0 / 255, face (T,H,W) i32 (-1 = background), depth (T,H,W) f32 camera z (0 = background), xyz (T,H,W,3) f32
 * the object-space point in CAD units (0 = background; 2 * (nocs - 0.5) of :104-106), rgb (T,H,W,3) u8, n_dropped (T) i32: the faces
 * of a view dropped whole because a vertex is nearer than `near` (there is no clipper) or an index is outside [0, V).
 * Visibility is the per-pixel minimum of (depth bits << 32 | face id), taken with 64-bit atomic mins on the workspace: a function of
 * the inputs alone.  H, W 1 .. 2048, T 1 .. 1024, F 1 .. 2^24, workspace 8-byte aligned and at least
 * sam6d_render_views_workspace_bytes(T, H, W) (0 for sizes outside the limits); anything else returns non-zero without a launch or a
 * write. */
size_t sam6d_render_views_workspace_bytes(int T, int H, int W);
int sam6d_render_views(const float* vertices, int V, const int* faces, int F, const float* normals, const unsigned char* colors,
                       const float* view, const float* light, int T, float fx, float fy, float cx, float cy, int H, int W, float near,
                       float base_color, int colorize, const unsigned char* srgb_lut, int wave_area, unsigned char* mask, int* face,
                       float* depth, float* xyz, unsigned char* rgb, int* n_dropped, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The same renderer for a textured model: Render/render_custom_templates.py:60 loads its --cad_path with bproc.loader.load_obj, which
 * takes an OBJ with its MTL and diffuse image (and a PLY that names a texture file) as well as a vertex-coloured PLY.  The arguments,
 * the workspace, the outputs and the geometry are sam6d_render_views's; visibility is the same pass.  Only the albedo of rgb differs: it
 * is the bilinear, repeat-wrapped lookup of `texture` at the perspective-correct attribute of face_uv (the TEXTURE recipe at the top of
 * csrc/texture.hip, restated in tests/texture_ref.py).  face_uv (F,3,2) f32: (u, v) of each face's three corners in stored order,
 * v = 0 at the bottom edge of the image.  texture (Ht,Wt,4) u8 on the device, 4-byte aligned, row 0 the top row, bytes R G B and one
 * ignored byte.  texel_lut 256 f32 on the device: the albedo of a byte (k / 255 in fp32 gives the vertex-colour path's values; the
 * host may pass the sRGB-to-linear table instead).  There is no colorize and no colors here: a caller that wants the grey render calls
 * sam6d_render_views; base_color keeps its place in the argument list and is not used.  Ht, Wt 1 .. 8192; every limit of sam6d_render_views holds; anything else returns non-zero without a launch or
 * a write.  (New entry only, so SAM6D_ABI_VERSION stays.) */
int sam6d_render_views_textured(const float* vertices, int V, const int* faces, int F, const float* normals, const float* view,
                                const float* light, int T, float fx, float fy, float cx, float cy, int H, int W, float near,
                                float base_color, const unsigned char* srgb_lut, int wave_area, const float* face_uv,
                                const unsigned char* texture, int Ht, int Wt, const float* texel_lut, unsigned char* mask, int* face,
                                float* depth, float* xyz, unsigned char* rgb, int* n_dropped, void* workspace, size_t workspace_bytes,
                                void* stream);
/* trimesh.sample.sample_surface as the reference calls it (Render/render_custom_templates.py:35, ISM/run_inference_custom.py:232-234,
 * PEM/run_inference_custom_pytorch.py:298-300): n area-weighted points of the surface.  NOT trimesh's or numpy's stream: an integer
 * definition of its own (csrc/meshsample.hip, restated in tests/meshsample_ref.py), equal to the reference in distribution only:
 * fp32 face areas, integer weights floor(area / area_max * 2^24) (at least 1 for a face with area, 0 without), their uint64 prefix
 * sums, and per sample three keys of sam6d_draw_choice's hash: one picks the face, two the barycentric pair.  Sample j is sample
 * row + j of the stream `seed`, so a call with row = r continues a call that drew r samples.  points (n,3) f32, face (n) i32.
 * n and F 1 .. 2^24, workspace 8-byte aligned and at least sam6d_mesh_sample_workspace_bytes(F) (0 for F outside the limits); a mesh
 * whose faces all have zero area is refused before the outputs are written (one read-back of area_max: the call synchronises the
 * stream).  Anything else returns non-zero without a launch. */
size_t sam6d_mesh_sample_workspace_bytes(int F);
int sam6d_mesh_sample(const float* vertices, int V, const int* faces, int F, int n, unsigned seed, unsigned row, float* points, int* face,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The result pictures of the two inference scripts (vis_ism.png, vis_pem.png), built on the device
 * ------------------------------------------------------------------------------------------------------------ */
/* `draw_detections` of PEM/utils/draw_utils.py:75-97 as PEM/run_inference_custom.py:110-134 (`visualize`) uses it, for N poses in one
 * call, with the side-by-side paste of :128-133.  rgb (H,W,3) u8, pixel (y, x) at rgb + y row_stride + 3 x (row_stride in bytes, at
 * least 3 W: a crop view works); R (N,3,3), t (N,3), K (N,3,3) f32 row-major; box (8,3) f32, the corners in the order of
 * draw_utils.py:20-49, and pts (P,3) f32, both in model units; colors (N,3) u8; thickness T of the box edges and radius r of the
 * points in pixels (the reference draws with 3 and 1).  canvas (H, 2W, 3) u8: the left half is rgb, the right half rgb with the
 * detections painted over it; n_skipped (N) i32: the primitives of an instance that were not drawn.
 * Contract (the recipe at the top of csrc/overlay.hip, restated in tests/overlay_ref.py; bitwise reproducible): projection in fp32,
 * P = ((R0 x + R1 y) + R2 z) + t per row, q = K P in the same association, u = (int)(q0 / q2), v = (int)(q1 / q2) truncating like the
 * reference's int32 cast (draw_utils.py:13-16).  A point is skipped when q2 > 0 is false or a quotient is outside -8192 .. 8191
 * (compared in fp32); an edge when either corner is; each adds one to n_skipped[i] (the reference has no rule and divides by zero).
 * Paint order per instance as draw_utils.py:51-97: ground edges (4,5) (5,7) (6,4) (7,6) in int(0.3 c), pillars (k, k+4) in int(0.6 c),
 * top edges (0,1) (1,3) (2,0) (3,2) in c, the P points in c; later paint wins, a later instance over an earlier one.  The thick line
 * (round caps, integer distance predicate) and the disc (dx^2 + dy^2 <= r^2) are the package's own shapes, NOT cv2.line / cv2.circle:
 * equal in kind only.  The painter keeps the largest key 4 i + stage + 1 per pixel with 32-bit atomic maxima on the workspace, and a
 * second kernel is the only writer of the canvas: a function of the inputs alone.
 * H, W 1 .. 8192, N 0 .. 65535, P 0 .. 65536, T 1 .. 15, r 0 .. 15; workspace 4-byte aligned and at least
 * sam6d_draw_detections_workspace_bytes(H, W) (0 for sizes outside the limits); anything else returns non-zero without a launch or a
 * write.  (New entries only, so SAM6D_ABI_VERSION stays.) */
size_t sam6d_draw_detections_workspace_bytes(int H, int W);
int sam6d_draw_detections(const unsigned char* rgb, long row_stride, int H, int W, const float* R, const float* t, const float* K, int N,
                          const float* box, const float* pts, int P, const unsigned char* colors, int thickness, int radius,
                          unsigned char* canvas, int* n_skipped, void* workspace, size_t workspace_bytes, void* stream);
/* The picture of ISM/run_inference_custom.py:48-84 (`visualize`) for M masks in one call (M = 1 is the reference), with the
 * side-by-side paste of :79-84.  rgb as above; masks (M,H,W) u8 or bool, non-zero = inside, drawn in the order given (later over
 * earlier); lut (M,3,256) u8, the blend of :70-72 tabulated on the host per mask, channel and grey value; canvas (H, 2W, 3) u8: the
 * left half is rgb, the right half the picture.
 * Contract (csrc/overlay.hip, tests/overlay_ref.py; bitwise reproducible): grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's
 * published 8-bit RGB2GRAY fixed point, restated, not pinned against cv2); a pixel covered by masks shows lut[m][c][grey] of the last
 * such m, another pixel grey in all channels; with draw_edge != 0 a pixel in the edge of any mask is 255.  The edge is the package's
 * own, NOT skimage's canny (:62), equal in kind only: mask pixels with a 4-neighbour inside the image that is not mask, dilated by
 * the reference's binary_dilation(edge, np.ones((2, 2))) (:63) exactly.  A gather with one writer per byte, no atomics, no workspace.
 * H, W 1 .. 8192, M 0 .. 4096 (M = 0: the grey picture; masks and lut may be NULL); anything else returns non-zero without a launch
 * or a write.  (New entries only, so SAM6D_ABI_VERSION stays.) */
int sam6d_overlay_masks(const unsigned char* rgb, long row_stride, int H, int W, const unsigned char* masks, int M,
                        const unsigned char* lut, int draw_edge, unsigned char* canvas, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Checking poses against the depth image: the CAD model rendered at each pose (csrc/verify.hip, restated in
 * tests/verify_ref.py).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* The window of each of N poses: what a pose's render covers, before anything is rendered.  The reference has no check of a pose
 * against the depth image -- it multiplies the detection score by the PEM score (PEM/run_inference_custom_pytorch.py:460-482) -- so the
 * check and its thresholds are the package's own; the geometry is the template renderer's (Render/render_custom_templates.py:55-106 as
 * sam6d_render_views restates it: the same device functions, unchanged).  vertices (V,3) f32, faces (F,3) i32, view (N,3,4) f32
 * row-major object -> camera, one per pose; fx fy cx cy, H, W, near as sam6d_render_views has them.
 * box (N,4) i32 = [x0, y0, x1, y1], inclusive: over the pose's live faces (not dropped, not of zero area) whose pixel box clamped to
 * the image is not empty, the minimum x0, y0 and the maximum x1, y1 of those boxes; [0, 0, -1, -1] when there are none.  n_dropped (N)
 * i32 with the meaning it has in sam6d_render_views.  Integer atomic min / max / add: a function of the inputs alone.
 * H, W 1 .. 2048, N 1 .. 1024, F 1 .. 2^24, V >= 1, near > 0; anything else, or a null pointer, returns non-zero without a launch or a
 * write. */
int sam6d_pose_windows(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy, float cx,
                       float cy, int H, int W, float near, int* box, int* n_dropped, void* stream);
/* Renders the model at each of N poses into the pose's own window, classifies every rendered pixel against the observed depth and
 * composites all poses into one instance map.  Beside PEM/run_inference_custom_pytorch.py:460-482, which has no such check: the check
 * and its thresholds are the package's own (the renderer: Render/render_custom_templates.py:55-106 as sam6d_render_views restates it).
 * Mesh, view, camera and wave_area as above and as in sam6d_render_views.  box (N,4) i32 from sam6d_pose_windows; offset (N+1) i64 on
 * the device: the exclusive prefix sums of the windows' areas (x1 - x0 + 1) * (y1 - y0 + 1), 0 for an empty window; total: the host's
 * copy of offset[N].  depth_obs (H,W) f32 in the unit of camera z; masks (N,H,W) u8 or NULL; tau >= 0, finite.
 * Per rendered pixel of pose n with r its rendered depth and o = depth_obs[y][x]: unknown when o > 0 is false (also a NaN); else with
 * e = o - r behind when e > tau, occluded when e < -tau, inlier otherwise; inter when masks[n][y][x] != 0.
 * counts (N,8) i32 = n_render, n_inlier, n_occluded, n_behind, n_unknown, n_mask (the non-zero bytes of masks[n] over the whole
 * image), n_inter, n_dropped; columns 1 .. 4 sum to column 0, columns 5 and 6 are 0 without masks.  ids (H,W) i32 or NULL: the pose
 * whose render is nearest at the pixel, on a tie the lower index, -1 = background; depth_out (H,W) f32 or NULL: that depth, 0 =
 * background.  total == 0: counts all 0 (column 7 too: it is counted by the raster pass, which is not launched), ids -1, depth_out 0.
 * The recipe is at the top of csrc/verify.hip; 64-bit atomic minima and 32-bit atomic adds only: a function of the inputs alone.  The
 * kernels clamp every box to the image and address no word at or beyond `total`, whatever box and offset hold.
 * Limits of sam6d_pose_windows, wave_area >= 0, total 0 .. N H W, workspace 8-byte aligned and at least
 * sam6d_pose_verify_workspace_bytes(total, H, W) = 8 (total + H W) (0 for sizes outside the limits); anything else, a null pointer
 * or a negative or non-finite tau returns non-zero without a launch or a write. */
size_t sam6d_pose_verify_workspace_bytes(long total, int H, int W);
int sam6d_pose_verify(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy, float cx,
                      float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset, long total,
                      const float* depth_obs, const unsigned char* masks, float tau, int* counts, int* ids, float* depth_out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The picture of an instance map: the rendered silhouettes where PEM/utils/draw_utils.py:75-97 draws a box and points
 * (PEM/run_inference_custom_pytorch.py:480-482), the package's own.  rgb (H,W,3) u8 with a byte row_stride >= 3 W, ids (H,W) i32 (an id
 * outside [0, N) counts as -1), colors (N,3) u8, alpha an integer in 0 .. 256.  canvas (H, 2W, 3) u8: the left half is rgb; on the
 * right a pixel with id >= 0 shows (rgb_c * (256 - alpha) + color_c * alpha + 128) >> 8, or color_c unblended when one of its four
 * neighbours inside the image has another id (the silhouette and the line between two instances; the image border is no edge), and a
 * background pixel shows rgb.  A gather with one writer per byte, no atomics, no workspace.  H, W 1 .. 2048, N 1 .. 1024; anything
 * else or a null pointer returns non-zero without a launch or a write. */
int sam6d_overlay_instances(const unsigned char* rgb, long row_stride, int H, int W, const int* ids, const unsigned char* colors, int N,
                            int alpha, unsigned char* canvas, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Refining poses against the depth image: projective point-to-plane steps on the renders of csrc/verify.hip
 * (csrc/refine.hip, restated in tests/refine_ref.py).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* One Gauss-Newton iteration of a projective point-to-plane refinement for N poses at once.  The reference has no refinement: its
 * poses leave PEM's weighted SVD as they are (PEM/run_inference_custom_pytorch.py:460-471); the method, its gates and its status codes
 * are the package's own.  Mesh, camera, near, wave_area, box, offset, total, depth_obs and masks as in sam6d_pose_verify; box and
 * offset are the caller's and stay the same for every iteration (sam6d_hip.refine: sam6d_pose_windows of the initial poses, grown by a
 * margin).  state (N,12) f64, in and out: R row-major, then t.  scale: CAD units into the unit of t, non-zero and finite.
 * The step (the recipe is at the top of csrc/refine.hip): view = [fl32(R * scale) | fl32(t)] is rastered into the windows with the
 * raster pass of sam6d_pose_verify (one copy of the kernel: the same keys).  A rendered pixel with depth r on face f and observed
 * depth o is a pair when o > 0, |o - r| <= gate and, with masks, masks[n][y][x] != 0; its residual e = nrm . (q - p) and its row
 * J = [(q - t) x nrm, nrm] (q, p the observed and rendered points on the pixel's ray, nrm the face's unit normal towards the camera)
 * are fp32, lengths times inv_unit (1 / the model's radius in the unit of t), and a pixel with |q - t| inv_unit > 16 or |e| > 16 is no
 * pair.  The 28 products J_i J_j, J_i e, e e are formed exactly in float64, times 2^30, rounded to the nearest even integer and added
 * with 64-bit integer atomics: acc (N,32) i64 = the upper triangle of [J e]^T [J e] row-major (words 0 .. 27; word 27 is sum e e),
 * the pair count (28), zeros (29 .. 31) -- a function of the inputs alone.  Then per pose: A_ii += damping * A_ii, Cholesky,
 * xi = (omega, v); R <- C(omega) R with the Cayley map C, t <- t + v / inv_unit, float64 with + - * / sqrt only.
 * stats (N,4) i32 = pairs, status, the low and the high 32 bits of acc[n][27].  status: 0 stepped, 1 fewer than min_pairs pairs,
 * 2 a pivot not positive, 3 |xi| > max_step (also a NaN), 4 the window is empty; with any but 0 state[n] keeps its bits.
 * Limits of sam6d_pose_verify; gate >= 0, inv_unit > 0 and damping >= 0 finite, min_pairs >= 1, max_step > 0 (infinity: no bound);
 * workspace, state and acc 8-byte aligned, the workspace at least sam6d_pose_refine_workspace_bytes(total, N) = 8 total + 80 N
 * (0 for N outside 1 .. 1024 or total outside 0 .. 2^22 N); anything else or a null pointer returns non-zero without a launch or a
 * write.  The kernels clamp every box to the image and address no word at or beyond `total`, whatever box and offset hold. */
size_t sam6d_pose_refine_workspace_bytes(long total, int N);
int sam6d_pose_refine_step(const float* vertices, int V, const int* faces, int F, float scale, int N, float fx, float fy, float cx,
                           float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset, long total,
                           const float* depth_obs, const unsigned char* masks, float gate, float inv_unit, double damping,
                           int min_pairs, double max_step, double* state, long long* acc, int* stats, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ISM's reference data from a template set: boxes and 224 x 224 crops of T templates, each on its own image
 * (csrc/refdata.hip).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
#define SAM6D_TEMPLATE_CUSTOM 0 /* ISM/run_inference_custom.py:138-140: rgb / 255 times mask / 255, no Normalize */
#define SAM6D_TEMPLATE_BOP 1    /* ISM/provider/bop.py:68-81: rgb / 255, T.Normalize after the padding, no mask product */
/* `mask.getbbox()` of ISM/run_inference_custom.py:136 (`image.getbbox()` of an RGBA template, ISM/provider/bop.py:66, with the alpha
 * band given) for T single-band u8 images in one launch: boxes (T,4) i64 on the device = (left, upper, right + 1, lower + 1) over the
 * pixels != 0, and (0,0,0,0) for an image without one (PIL returns None there).  Pixel (y, x) of image t is the byte
 * band + t image_stride + (y W + x) pixel_stride (strides in bytes), so the alpha band of an interleaved (T,H,W,4) tensor is read in
 * place with band = rgba + 3, pixel_stride 4.  No atomics and no workspace: the result does not depend on any order.
 * T <= 65535, H W <= 2^29, pixel_stride 1 .. 64, image_stride >= 0; anything else returns non-zero without a launch. */
int sam6d_template_boxes(const unsigned char* band, int T, int H, int W, long pixel_stride, long image_stride, long long* boxes,
                         void* stream);
/* The template crops of ISM/run_inference_custom.py:138-155 (flavour SAM6D_TEMPLATE_CUSTOM) and ISM/provider/bop.py:68-83
 * (SAM6D_TEMPLATE_BOP) through CropResizePad(224) (ISM/utils/bbox_utils.py:89-126) for T templates in one launch, template t reading
 * its own image through boxes[t] = (x1, y1, x2, y2) i64 on the device (exclusive ends; no read-back).  Channel c of pixel (y, x) of
 * template t is the byte rgb + t rgb_image_stride + (y W + x) rgb_pixel_stride + c (3 for an RGB tensor, 4 for the colours of an RGBA
 * one), its mask the byte mask + t mask_image_stride + (y W + x) mask_pixel_stride.  out_rgb (T,3,224,224) f32: custom
 * fl32(u8 / 255) * fl32(mask / 255) with padding 0; bop (fl32(u8 / 255) - mean) / std in fp32 with padding (0 - mean) / std (mean
 * 0.485/0.456/0.406, std 0.229/0.224/0.225).  out_mask (T,224,224) f32 = fl32(mask / 255), padding 0.  Either output may be NULL,
 * rgb too when out_rgb is, and mask when neither out_mask nor the custom product needs it.  The gather is the one of
 * sam6d_dino_crop_proposals (one index recipe, csrc/crop_index.h): bit-exact; a box with side <= 0 or an empty resized crop is all
 * padding.  T <= 65535, H W <= 2^29, rgb_pixel_stride 3 .. 64, mask_pixel_stride 1 .. 64, image strides >= 0; anything else returns
 * non-zero without a launch. */
int sam6d_template_crops(const unsigned char* rgb, long rgb_pixel_stride, long rgb_image_stride, const unsigned char* mask,
                         long mask_pixel_stride, long mask_image_stride, const long long* boxes, int T, int H, int W, int flavour,
                         float* out_rgb, float* out_mask, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Scoring poses against ground truth: MSSD, MSPD, ADD and VSD (csrc/poseerr.hip, restated in tests/poseerr_ref.py).
 * (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* The point errors of N estimated poses against their ground truths.  Beside PEM/run_inference_custom_pytorch.py:460-471, which
 * writes its poses and has no evaluation: the errors are the published ones (Hodan et al., BOP Challenge 2020; ADD: Hinterstoisser
 * et al. 2012), restated by the package and pinned against its numpy restatement, not against bop_toolkit.
 * points (V,3) f32 model vertices in CAD units; est, gt (N,3,4) f32 row-major object -> camera; syms (S,3,4) f32 the object's symmetry
 * transforms in CAD units (row 0 the identity by convention, not enforced); fx fy cx cy the camera; inv_unit > 0, finite.
 * Per pose n and symmetry s, G = fl32(gt[n] o syms[s]) (formed in float64); per point e = est[n] x, g = G x, d2 = |e - g|^2, and
 * p2 = the squared pixel distance of their projections u = fx * (x / z) + cx, v = fy * (y / z) + cy, all fp32 in the order of the
 * recipe at the top of csrc/poseerr.hip.  A point with e_z > 0 or g_z > 0 false takes no part in the pair's p2 maximum; n_skipped[n]
 * counts such points for s = 0.
 * mssd[n] = sqrtf(min_s max_x d2), mspd[n] = sqrtf(min_s max_x p2) f32; mssd_sym[n], mspd_sym[n] i32 the lowest s that attains the
 * minimum; add_sum[n] i64 = sum_x rint((double)sqrtf(d2 at s = 0) * inv_unit * 2^30), a term above 2^42 (4096 units; a NaN too)
 * counted as 2^42: ADD = add_sum / 2^30 / inv_unit / V.  Integer atomic maxima and adds only: a function of the inputs alone.
 * V 1 .. 2^20, N 1 .. 1024, S 1 .. 1024; workspace and add_sum 8-byte aligned, the workspace at least
 * sam6d_pose_point_errors_workspace_bytes(N, S) = 8 N S (0 for sizes outside the limits); anything else, a null pointer or a
 * non-finite inv_unit returns non-zero without a launch or a write, the argument named in sam6d_last_error(). */
size_t sam6d_pose_point_errors_workspace_bytes(int N, int S);
int sam6d_pose_point_errors(const float* points, int V, const float* est, const float* gt, int N, const float* syms, int S, float fx,
                            float fy, float cx, float cy, float inv_unit, float* mssd, float* mspd, int* mssd_sym, int* mspd_sym,
                            int* n_skipped, long long* add_sum, void* workspace, size_t workspace_bytes, void* stream);
/* The counts of BOP's Visible Surface Discrepancy for N pose pairs.  Beside PEM/run_inference_custom_pytorch.py:460-471, as above; the
 * renderer is the package's own (Render/render_custom_templates.py:55-106 as sam6d_render_views restates it), so the figure is BOP's
 * in kind and not pixel for pixel.  Mesh, camera, near, wave_area as in sam6d_pose_verify.  view (2N,3,4) f32: views 0 .. N-1 the
 * estimates, N .. 2N-1 the ground truths; box (2N,4) i32 and offset (2N+1) i64 on the device as in sam6d_pose_verify, both views of a
 * pair with the same box (the union of their sam6d_pose_windows boxes), so that the ground-truth word of word i is i + offset[N];
 * total: the host's copy of offset[2N].  depth_obs (H,W) f32; delta >= 0 finite, in the unit of camera z; taus: T numbers >= 0 ON THE
 * HOST, T 1 .. 16; inv_norm > 0 finite (1, or 1 / the model's diameter).
 * Per window pixel, with the rendered depths r_e, r_g (or absent), o = depth_obs[y][x] a reading when o > 0, and distances D = z * c,
 * c = sqrtf((ax ax + ay ay) + 1), ax = ((float)x - cx) / fx: visib_gt = has_g && (!reading || D_g - D_o <= delta),
 * visib_est = has_e && (!reading || D_e - D_o <= delta || visib_gt) (BOP's `bop19` visibility); cost_k counts the pixels visible in
 * both with fabsf(D_g - D_e) * inv_norm >= taus[k] (BOP's `step` cost).
 * counts (N, 4+T) i32 = n_union, n_inter, n_visib_est, n_visib_gt, cost_0 .. cost_{T-1}; VSD_k = (cost_k + n_union - n_inter) /
 * n_union, 1 where n_union is 0.  total == 0: all 0.  64-bit atomic minima and 32-bit atomic adds only: a function of the inputs
 * alone.  The kernels clamp every box to the image and address no word at or beyond `total`, whatever box and offset hold.
 * Limits of sam6d_pose_windows with N 1 .. 512, wave_area >= 0, fx and fy not 0, total 0 .. 2 N H W, workspace 8-byte aligned and at
 * least sam6d_pose_vsd_workspace_bytes(total, N) = 8 total + 64 N (the z-buffer words, and the raster pass's counter words; 0 for
 * sizes outside the limits); anything else or a null pointer returns non-zero without a launch or a write. */
size_t sam6d_pose_vsd_workspace_bytes(long total, int N);
int sam6d_pose_vsd(const float* vertices, int V, const int* faces, int F, const float* view, int N, float fx, float fy, float cx,
                   float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset, long total,
                   const float* depth_obs, float delta, const float* taus, int T, float inv_norm, int* counts, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ADD-S / ADI and the model diameter: exact pruned searches over all pairs of vertices (csrc/nearest.hip, restated in
 * tests/nearest_ref.py).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* ADI (ADD-S: Hinterstoisser et al. 2012; Hodan et al. 2016) of N estimated poses against their ground truths, over the model's
 * vertices.  Beside PEM/run_inference_custom_pytorch.py:460-471, which writes its poses: the reference has no evaluation code.  The
 * definition is the published one, restated by the package and pinned against its numpy restatement, not against bop_toolkit.
 * points (V,3) f32 model vertices in CAD units; est, gt (N,3,4) f32 row-major object -> camera; inv_unit > 0, finite; no symmetries.
 * Per pose n and point i: e_i = est[n] x_i, g_j = gt[n] x_j, m_i = the least d2_ij = |e_i - g_j|^2 over all j (fp32 in the order of
 * the recipe at the top of csrc/nearest.hip; a NaN never wins, m_i = +inf where no d2 is a number), and
 * adi_sum[n] i64 = sum_i rint((double)sqrtf(m_i) * inv_unit * 2^30), a term above 2^42 (4096 units; a NaN too) counted as 2^42:
 * ADI = adi_sum / 2^30 / inv_unit / V.  Tiles of 256 points whose box cannot hold a nearer point are skipped; the bound holds in fp32
 * without a margin, so the sum has the bits of the full search.  flags: bit 0 = skip nothing (the full V x V walk), other bits 0.
 * The order of the points does not change the sum; tiles of neighbouring points (a sort along a space-filling curve) skip more.
 * Integer atomic adds only: a function of the inputs alone.
 * V 1 .. 2^20, N 1 .. 1024; workspace and adi_sum 8-byte aligned, the workspace at least sam6d_pose_adi_workspace_bytes(V, N) =
 * 24 N ceil(V / 256) (the boxes; 0 for sizes outside the limits); anything else, a null pointer or a non-finite inv_unit returns
 * non-zero without a launch or a write, the argument named in sam6d_last_error(). */
size_t sam6d_pose_adi_workspace_bytes(int V, int N);
int sam6d_pose_adi(const float* points, int V, const float* est, const float* gt, int N, float inv_unit, int flags, long long* adi_sum,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The diameter of a point set as bop_toolkit defines a model's: the largest distance between two of its points.  Beside
 * PEM/run_inference_custom_pytorch.py:460-471, as above: the reference has no evaluation code and reads no diameter.
 * points (V,3) f32; seeds (n_seeds) i32 ON THE DEVICE, point indices whose distances to all points give the first lower bound (the
 * extreme point of each axis is a good choice); a seed outside [0, V) is ignored, never dereferenced.  diameter: one f32 =
 * sqrtf(max_ij d2_ij), d2_ij = |x_i - x_j|^2 in fp32 in the order of the recipe at the top of csrc/nearest.hip, the maximum taken as
 * sam6d_pose_point_errors takes its maxima (a NaN is above every number: a coordinate that is not finite gives NaN).  V = 1 gives 0.
 * Tile pairs whose boxes cannot hold a pair farther apart than the seeds' bound are skipped; the bound holds in fp32 without a margin,
 * so the result has the bits of the full search.  flags: bit 0 = skip nothing, other bits 0.  Integer atomic maxima only.
 * V 1 .. 2^20, n_seeds 1 .. 8; workspace 8-byte aligned and at least sam6d_points_diameter_workspace_bytes(V) = 8 + 24 ceil(V / 256)
 * (0 for a V outside the limits); anything else or a null pointer returns non-zero without a launch or a write. */
size_t sam6d_points_diameter_workspace_bytes(int V);
int sam6d_points_diameter(const float* points, int V, const int* seeds, int n_seeds, int flags, float* diameter, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * All-pairs pose errors, the matching of estimates to ground-truth instances and the removal of duplicate poses
 * (csrc/posematch.hip, restated in tests/posematch_ref.py).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* The point errors of every pose a[i] against every pose b[j] of one object.  Beside PEM/run_inference_custom_pytorch.py:460-471,
 * which writes all its poses out unmatched and has no evaluation.  For every (i, j) the outputs are, bit for bit, what
 * sam6d_pose_point_errors gives for est = a[i], gt = b[j] (the recipe at the top of csrc/poseerr.hip, one copy of its per-point step
 * in csrc/poseerr_point.h): G = fl32(b[j] o syms[s]), mssd = sqrtf(min_s max_x d2), mspd the same in pixels, the lowest s on a tie,
 * n_skipped the points behind the camera under either pose for s = 0, add_sum the 2^30-scaled integer ADD sum capped at 2^42 a term.
 * points (V,3) f32; a (A,3,4), b (B,3,4), syms (S,3,4) f32 row-major; inv_unit > 0, finite.  flags: bit 0 = no MSPD: fx fy cx cy
 * are ignored, the projections are not computed, and mspd, mspd_sym, n_skipped are not written (they may be null); other bits 0.
 * mssd, mspd (A,B) f32; mssd_sym, mspd_sym, n_skipped (A,B) i32; add_sum (A,B) i64, 8-byte aligned.
 * The B S matrices are split over the launch grid by the sizes alone (runs of 8 .. 256 matrices, at least about 2048 workgroups where there are that many runs); the
 * partial results meet as integer atomic maxima and adds, so the outputs are a function of the inputs alone and not of the split.
 * V 1 .. 2^20; A, B, S 1 .. 1024 each and A B S <= 2^22; workspace 8-byte aligned and at least
 * sam6d_pose_pair_errors_workspace_bytes(A, B, S) = 8 A B S (0 for sizes outside the limits); anything else, a null pointer or a
 * non-finite inv_unit returns non-zero without a launch or a write, the argument named in sam6d_last_error(). */
size_t sam6d_pose_pair_errors_workspace_bytes(int A, int B, int S);
int sam6d_pose_pair_errors(const float* points, int V, const float* a, int A, const float* b, int B, const float* syms, int S, float fx,
                           float fy, float cx, float cy, float inv_unit, int flags, float* mssd, float* mspd, int* mssd_sym,
                           int* mspd_sym, int* n_skipped, long long* add_sum, void* workspace, size_t workspace_bytes, void* stream);
/* Greedy matching of A estimates to B targets from an error matrix, for each of T thresholds on its own.  Beside
 * PEM/run_inference_custom_pytorch.py:460-471, which writes its poses out unmatched.  BOP's match_poses in kind; the recipe is the
 * package's own (csrc/posematch.hip RECIPE b) and is pinned against its numpy restatement, not against bop_toolkit.
 * err (A,B) f32; scores (A) f32; thr (T) f32 ON THE DEVICE; valid (B) bytes, non-zero = a target that may be taken, null = all.
 * The estimates go by descending score, equal scores the lower index first, a NaN score last; with max_ests > 0 only the first
 * max_ests of that order take part.  Per threshold k, in that order, estimate i takes the target j with the smallest err[i][j] among
 * those valid, not yet taken and with err[i][j] < thr[k] (strict; false for a NaN), the lowest j among equal errors.
 * est_match (T,A) i32 = j or -1; gt_match (T,B) i32 = i or -1; n_matched (T) i32.  One wave per threshold, no atomics.
 * A, B 1 .. 1024, T 1 .. 64, max_ests >= 0; workspace 4-byte aligned and at least sam6d_pose_match_workspace_bytes(A) = 4 A rounded
 * up to 16 (0 for an A outside the limits); anything else or a null pointer returns non-zero without a launch or a write. */
size_t sam6d_pose_match_workspace_bytes(int A);
int sam6d_pose_match(const float* err, int A, int B, const float* scores, const float* thr, int T, const unsigned char* valid,
                     int max_ests, int* est_match, int* gt_match, int* n_matched, void* workspace, size_t workspace_bytes, void* stream);
/* Greedy removal of duplicate poses from an (N,N) error matrix.  Beside PEM/run_inference_custom_pytorch.py:460-471, which writes
 * every pose with its score.  The recipe is the package's own (csrc/posematch.hip RECIPE c), pinned against its numpy restatement.
 * err (N,N) f32, need not be symmetric, the diagonal is never read; scores (N) f32, the order as in sam6d_pose_match.  Walking the
 * order, pose i is kept unless a pose r kept before it has err[r][i] < thresh (strict; false for a NaN).
 * keep_idx (N) i64, 8-byte aligned: the kept poses in order, then -1; count (1) i32; suppressed_by (N) i32: the first kept pose in
 * order that suppresses i, i itself when it is kept.  No atomics.
 * N 1 .. 1024; workspace 8-byte aligned and at least sam6d_pose_nms_workspace_bytes(N) = 4 N rounded up to 16, + 8 N ceil(N / 64)
 * (0 for an N outside the limits); anything else or a null pointer returns non-zero without a launch or a write. */
size_t sam6d_pose_nms_workspace_bytes(int N);
int sam6d_pose_nms(const float* err, const float* scores, int N, float thresh, long long* keep_idx, int* count, int* suppressed_by,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * All-pairs VSD: one render per pose, the pairs by the overlap of their windows (csrc/vsdpairs.hip, restated in
 * tests/vsdpairs_ref.py).  (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* The counts of BOP's Visible Surface Discrepancy of every estimate a[i] against every ground truth b[j] of one object.  Beside
 * PEM/run_inference_custom_pytorch.py:460-471, where the reference writes its poses and leaves scoring to bop_toolkit.  For every
 * (i, j) the row of counts is, bit for bit, what sam6d_pose_vsd gives for est = a[i], gt = b[j]; the roles are not symmetric.
 * Mesh, camera, near, wave_area, depth_obs, delta, taus (ON THE HOST), T and inv_norm as in sam6d_pose_vsd.  view (A+B,3,4) f32: views
 * 0 .. A-1 are a, A .. A+B-1 are b; box (A+B,4) i32 and offset (A+B+1) i64 on the device as in sam6d_pose_verify, EVERY VIEW WITH ITS
 * OWN box (sam6d_pose_windows', not a pair's union); total: the host's copy of offset[A+B].
 * Each view is rastered once.  Per view and window pixel, with D = r * c as in sam6d_pose_vsd: has (a key is there) and own = has &&
 * (!reading || D - D_o <= delta); view_counts (A+B,2) i32 = n_render (#has), n_visible (#own).  Per pair, with E_i and G_j the
 * n_visible of a[i] and b[j] and X the intersection rectangle of their two windows: n_visib_gt = G_j, n_inter = #X{has_e && own_g},
 * n_visib_est = E_i + #X{has_e && !own_e && own_g}, n_union = n_visib_est + G_j - n_inter, cost_k = #X{has_e && own_g &&
 * fabsf(D_g - D_e) * inv_norm >= taus[k]}: integer identities of sam6d_pose_vsd's sets (the recipe at the top of csrc/vsdpairs.hip
 * says why).  counts (A, B, 4+T) i32 = n_union, n_inter, n_visib_est, n_visib_gt, cost_0 .. cost_{T-1}.  total == 0: every count and
 * view count is 0 and no pass runs.  A pair whose windows do not meet costs no pixel work.
 * 64-bit atomic minima (the raster) and 32-bit atomic adds (view_counts); a pair's row has one owner and is written by plain stores:
 * a function of the inputs alone.  The kernels clamp every box to the image and address no word at or beyond `total`, whatever box
 * and offset hold.
 * Limits of sam6d_pose_windows with A, B 1 .. 1024 each, T 1 .. 16, wave_area >= 0, fx and fy not 0, delta and taus finite and >= 0,
 * inv_norm finite and > 0, total 0 .. (A+B) H W, workspace 8-byte aligned and at least sam6d_pose_pair_vsd_workspace_bytes(total, A,
 * B) = 8 total + 8 ceil(total / 2) + 32 (A+B) (the z-buffer words, the 32-bit image of D and own, and the raster pass's counter
 * words; 0 for sizes outside the limits); anything else or a null pointer returns non-zero without a launch or a write. */
size_t sam6d_pose_pair_vsd_workspace_bytes(long total, int A, int B);
int sam6d_pose_pair_vsd(const float* vertices, int V, const int* faces, int F, const float* view, int A, int B, float fx, float fy,
                        float cx, float cy, int H, int W, float near, int wave_area, const int* box, const long long* offset,
                        long total, const float* depth_obs, float delta, const float* taus, int T, float inv_norm, int* counts,
                        int* view_counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * All-pairs ADI, capped by the tile bounds (csrc/pairadi.hip over csrc/nearest_walk.h, restated in tests/pair_adi_ref.py).
 * (New entries only, so SAM6D_ABI_VERSION stays.)
 * ------------------------------------------------------------------------------------------------------------ */
/* ADD-S / ADI of every pose a[i] against every pose b[j] of one object, over the model's vertices.  Beside
 * PEM/run_inference_custom_pytorch.py:460-471, which writes all its poses out unmatched and has no evaluation; beside sam6d_pose_adi,
 * which scores listed pairs, and sam6d_pose_pair_errors, which gives the other point errors as matrices.  The definition is the
 * published one, restated by the package and pinned against its numpy restatement, not against bop_toolkit.
 * points (V,3) f32; a (A,3,4), b (B,3,4) f32 row-major object -> camera; inv_unit > 0, finite; flags as in sam6d_pose_adi.
 * For a pair that is computed, adi_sum[i][j] i64 is bit for bit what sam6d_pose_adi gives for est = a[i], gt = b[j] (the recipe at the
 * top of csrc/nearest.hip, one copy of its steps in csrc/nearest_walk.h).  The boxes are built once per pose b[j].
 * cap_sum >= 0 (the caller's cap as an integer sum: floor(cap * inv_unit * 2^30 * V)): per pair and point e_i = a[i] x_i, lb_i = the
 * minimum over ALL tiles of b[j] of the tile bound of the skip rule (from +inf, fminf), and lower_sum[i][j] i64 = sum_i of
 * sam6d_pose_adi's term of lb_i, with the same cap at 2^42 and the same 64-bit integer adds.  lower_sum <= adi_sum holds as integers
 * (the proof is at the top of csrc/pairadi.hip), and a pair with lower_sum > cap_sum is SKIPPED: skipped[i][j] = 1, adi_sum[i][j] = -1,
 * its V x V search is never started.  Every other pair has skipped = 0.  cap_sum < 0: no cap; lower_sum is neither read nor written
 * and may be null.  skipped (A,B) bytes.  64-bit integer atomic adds only: every output is a function of the inputs alone.
 * V 1 .. 2^20; A, B 1 .. 1024 each and A B ceil(V / 1024) <= 2^22 (the workgroups of a launch); workspace, adi_sum and lower_sum
 * 8-byte aligned, the workspace at least sam6d_pose_pair_adi_workspace_bytes(V, A, B) = 24 B ceil(V / 256) (the boxes; 0 for sizes
 * outside the limits); anything else, a null pointer or a non-finite inv_unit returns non-zero without a launch or a write, the
 * argument named in sam6d_last_error(). */
size_t sam6d_pose_pair_adi_workspace_bytes(int V, int A, int B);
int sam6d_pose_pair_adi(const float* points, int V, const float* a, int A, const float* b, int B, float inv_unit, int flags, long cap_sum,
                        long long* adi_sum, long long* lower_sum, unsigned char* skipped, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAM6D_HIP_H */
