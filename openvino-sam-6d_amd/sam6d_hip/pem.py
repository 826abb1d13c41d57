"""Host orchestration of the PEM geometric-matching path on one MI355X.

The reference's Python modules call torch ops; this module issues the equivalent sequence of libsam6d_hip.so launches
on torch's current HIP stream.  torch is used for device buffers only (torch.empty) -- no torch arithmetic on the
path.  Everything that shares weights between the scene cloud and the template cloud (geo embedding, in_proj, PE, the
RPE self layers, the dense linear-attention layers, out_proj) runs ONCE on a stacked (2B, ...) batch; only the
sequential cross-attention halves (PEM/model/transformer.py:520-521) are issued per cloud.

What is here: the PEM weight set and its packed images, the pipeline's own primitives (`linear` with the panel route, `gemm` =
runtime.gemm behind bench.py's PROFILE hook), the layers, the pose solvers, and pem_match / PemGraph on top of them.  The plumbing
underneath (Options, on_tensor_device, Linear, the GEMM launch) is runtime.py's; the model's input tensors are built in inputs.py.

Citations: PEM = SAM-6D/Pose_Estimation_Model in the reference.
"""
import math
import types

import numpy as np
import torch

from . import _lib, runtime
from .ops import _chk
from .runtime import (C, Linear, Options, _empty, _flags, _getter, _p, _pow2_scale, _s, on_tensor_device, split_w16,
                      gemm_route)  # noqa: F401  (gemm_route: the route `gemm` and gemm_b2 below take, without the launch)

H = 4


# --------------------------------------------------------------------------------------------- weight packing
TB_P256, TB_P128, TB_P64 = 32768, 16384, 8192  # panel bytes of csrc/block.hip (32 rows x K = 256 / 128 / 64, fp16 hi + lo)
TB_CHUNK = 4 * TB_P256 + 8 * TB_P128
TB_Q_OFF = 8 * TB_P256 + 4 * TB_CHUNK


def pack_token_block(L, q=None, scale=None):
    """The LDS panel image + constant vector of csrc/block.hip for one layer tail L = {lin, n1, exp, sq, n2} (mode 0) or, with the
    dense layer's proj_q `q` and focusing `scale`, for a whole LinearTransformerLayer (mode 1).  Pure data movement plus the
    power-of-two operand scales (max / norms taken once, at weight-load time)."""
    dev = L["lin"].w.device
    mode = 1 if q is not None else 0
    nbytes = int(_lib.load().sam6d_token_block_image_bytes(mode))
    assert nbytes == TB_Q_OFF + (8 * TB_P256 if mode else 0)
    img = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def pk(Wt, row0, rows, k0, ksteps, sc, off):
        ld = Wt.shape[1]
        _lib.call("sam6d_pack_panels", _p(Wt, row0 * ld), ld, rows, k0, ksteps, float(sc), img.data_ptr() + off, _s())

    s_lin = _pow2_scale(L["lin"].w.abs().max())
    s_exp = _pow2_scale(L["exp"].w.abs().max())
    s_sq = _pow2_scale(L["sq"].w.abs().max())
    pk(L["lin"].w, 0, C, 0, 8, s_lin, 0)
    for c in range(4):
        base = 8 * TB_P256 + c * TB_CHUNK
        pk(L["exp"].w, 128 * c, 128, 0, 8, s_exp, base)
        pk(L["sq"].w, 0, C, 128 * c, 4, s_sq, base + 4 * TB_P256)
    s_q = 1.0
    if mode:
        s_q = _pow2_scale(q.w.abs().max())
        pk(q.w, 0, C, 0, 8, s_q, TB_Q_OFF)
    # bound of the FFN hidden row (Cauchy-Schwarz; |LayerNorm output|_2 <= 16 max|gamma| + |beta|_2): its scale must be known
    # before the chunks accumulate
    g1, b1 = L["n1"]
    ymax = 16.0 * float(g1.abs().max()) + float(b1.norm())
    hmax = float(L["exp"].w.norm(dim=1).max()) * ymax + float(L["exp"].b.abs().max())
    s_h = _pow2_scale(hmax)
    cst = torch.zeros(2568, dtype=torch.float32, device=dev)
    if mode:
        cst[0:256] = q.b
        cst[256:512] = 1.0 / torch.nn.functional.softplus(scale.reshape(-1))
    cst[512:768] = L["lin"].b
    cst[768:1024], cst[1024:1280] = g1, b1
    cst[1280:1792] = L["exp"].b
    cst[1792:2048] = L["sq"].b
    cst[2048:2304], cst[2304:2560] = L["n2"]
    cst[2560:2565] = torch.tensor([1.0 / s_q, 1.0 / s_lin, 1.0 / s_exp, 1.0 / (s_sq * s_h), s_h], device=dev)
    return dict(img=img, cst=cst, mode=mode)


def pack_cross_query(q):
    """proj_q of a cross-attention layer as the panel image of csrc/xattn.hip (head h = rows 64h .. 64h+64 = panels 2h, 2h+1)."""
    s_q = _pow2_scale(q.w.abs().max())
    img = torch.zeros(8 * TB_P256, dtype=torch.uint8, device=q.w.device)
    _lib.call("sam6d_pack_panels", _p(q.w), q.w.shape[1], C, 0, 8, float(s_q), img.data_ptr(), _s())
    return dict(img=img, inv=1.0 / s_q)


def pack_cross_kv(kv):
    """[proj_k; proj_v] of a cross-attention layer (kv.w (512,256): rows 0..255 proj_k, 256..511 proj_v) as the per-head panel images of
    csrc/xattn.hip's in-kernel key / value projection: head h -> Wk rows 64h..64h+64 (2 panels) | Wv rows 64h..64h+64 (2 panels)."""
    s_kv = _pow2_scale(kv.w.abs().max())
    nbytes = int(_lib.load().sam6d_cross_attention_kv_image_bytes())
    assert nbytes == 16 * TB_P256
    img = torch.zeros(nbytes, dtype=torch.uint8, device=kv.w.device)
    for h in range(H):
        for part in range(2):  # 0: proj_k, 1: proj_v
            _lib.call("sam6d_pack_panels", _p(kv.w, (part * C + 64 * h) * C), C, 64, 0, 8, float(s_kv),
                      img.data_ptr() + (4 * h + 2 * part) * TB_P256, _s())
    return dict(img=img, inv=1.0 / s_kv)


class PemWeights:
    """Device-resident weights in the layouts the kernels want, built from a reference-keyed state_dict
    (SURVEY 8b B2).  Packing is pure data movement: concatenating q/k/v projection weights, transposing proj_p, folding
    eval-mode BatchNorm into a per-channel scale/shift."""

    def __init__(self, sd, device, nblock=3, options=None):
        """options: the Options every launch sequence on this weight set runs with (None: the environment's, per call)."""
        g = _getter(sd, device)
        self.dev = device
        self.options = options
        self.nblock = nblock
        self.div_term = g("geo_embedding.embedding.div_term")
        self.geo_d = Linear(g("geo_embedding.proj_d.weight"), g("geo_embedding.proj_d.bias"))
        self.geo_a = Linear(g("geo_embedding.proj_a.weight"), g("geo_embedding.proj_a.bias"))
        self.coarse = self._matching(g, "coarse_point_matching")
        self.fine = self._matching(g, "fine_point_matching")
        self.coarse["blocks"] = [self._geo_transformer(g, "coarse_point_matching.transformers.%d" % i) for i in range(nblock)]
        self.fine["blocks"] = [self._sparse_to_dense(g, "fine_point_matching.transformers.%d" % i) for i in range(nblock)]
        self.pe = self._pe(g, "fine_point_matching.PE")

    @staticmethod
    def _matching(g, p):
        return dict(bg=g(p + ".bg_token").reshape(1, C), in_proj=Linear(g(p + ".in_proj.weight"), g(p + ".in_proj.bias")),
                    out_proj=Linear(g(p + ".out_proj.weight"), g(p + ".out_proj.bias")))

    @staticmethod
    def _post(g, p):
        L = dict(lin=Linear(g(p + ".attention.linear.weight"), g(p + ".attention.linear.bias")),
                 n1=(g(p + ".attention.norm.weight"), g(p + ".attention.norm.bias")),
                 exp=Linear(g(p + ".output.expand.weight"), g(p + ".output.expand.bias")),
                 sq=Linear(g(p + ".output.squeeze.weight"), g(p + ".output.squeeze.bias")),
                 n2=(g(p + ".output.norm.weight"), g(p + ".output.norm.bias")))
        L["tb"] = pack_token_block(L)  # the fused layer tail's weight image (csrc/block.hip)
        return L

    @staticmethod
    def _geo_transformer(g, p):
        s, c = p + ".layers.0", p + ".layers.1"
        sa, ca = s + ".attention.attention", c + ".attention.attention"
        self_l = dict(
            qkv=Linear(torch.cat([g(sa + ".proj_q.weight"), g(sa + ".proj_k.weight"), g(sa + ".proj_v.weight")], 0),
                       torch.cat([g(sa + ".proj_q.bias"), g(sa + ".proj_k.bias"), g(sa + ".proj_v.bias")], 0)),
            # proj_p folded into the query (attention.hip header): WpT[j, k] = Wp[k, j]; its bias cancels in softmax
            wpT=g(sa + ".proj_p.weight").t().contiguous(),
            **PemWeights._post(g, s))
        self_l["wpT16"] = split_w16(self_l["wpT"])
        cross_l = dict(
            q=Linear(g(ca + ".proj_q.weight"), g(ca + ".proj_q.bias")),
            kv=Linear(torch.cat([g(ca + ".proj_k.weight"), g(ca + ".proj_v.weight")], 0),
                      torch.cat([g(ca + ".proj_k.bias"), g(ca + ".proj_v.bias")], 0)),
            **PemWeights._post(g, c))
        cross_l["xq"] = pack_cross_query(cross_l["q"])
        cross_l["xkv"] = pack_cross_kv(cross_l["kv"])
        return dict(self=self_l, cross=cross_l)

    @staticmethod
    def _sparse_to_dense(g, p):
        """A SparseToDenseTransformer block: the geometric transformer of its sparse layer + the dense linear-attention layer (q, [k; v],
        the focusing scale, the layer tail and the whole layer's fused image)."""
        blk = PemWeights._geo_transformer(g, p + ".sparse_layer")
        d = p + ".dense_layer"
        a = d + ".attention.attention"
        L = dict(scale=g(a + ".scale").reshape(-1), q=Linear(g(a + ".proj_q.weight"), g(a + ".proj_q.bias")),
                 kv=Linear(torch.cat([g(a + ".proj_k.weight"), g(a + ".proj_v.weight")], 0),
                           torch.cat([g(a + ".proj_k.bias"), g(a + ".proj_v.bias")], 0)), **PemWeights._post(g, d))
        L["tbd"] = pack_token_block(L, L["q"], L["scale"])
        blk["dense"] = L
        return blk

    @staticmethod
    def _pe(g, pe):
        """PositionalEncoding's MLPs: the 1x1 convolutions of mlp1 / mlp2 with their eval-mode BatchNorm folded into a per-channel
        scale / shift, and mlp3."""
        mlp = []
        for k in (1, 2):
            layers = []
            for l in range(3):
                q = "%s.mlp%d.layer%d" % (pe, k, l)
                w = g(q + ".conv.weight")
                w = w.reshape(w.shape[0], w.shape[1]).contiguous()
                bn = q + ".normlayer.bn"
                scale = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + 1e-5)
                shift = g(bn + ".bias") - g(bn + ".running_mean") * scale
                layers.append(dict(w=w, scale=scale.contiguous(), shift=shift.contiguous()))
            mlp.append(layers)
        return dict(mlp=mlp, mlp3=Linear(g(pe + ".mlp3.conv.weight").reshape(C, C), g(pe + ".mlp3.conv.bias")))


# The drop-in sub-modules pack only their own part of the weights, into a plain namespace holding the PemWeights attributes their
# launches read (pem/transformer.py, pem/coarse_point_matching.py, pem/fine_point_matching.py).
def pack_geo(sd, device, p="geo_embedding"):
    g = _getter(sd, device)
    return types.SimpleNamespace(dev=device, div_term=g(p + ".embedding.div_term"),
                                 geo_d=Linear(g(p + ".proj_d.weight"), g(p + ".proj_d.bias")),
                                 geo_a=Linear(g(p + ".proj_a.weight"), g(p + ".proj_a.bias")))


def pack_geo_transformer(sd, device, p):
    return PemWeights._geo_transformer(_getter(sd, device), p)


def pack_sparse_to_dense(sd, device, p):
    return PemWeights._sparse_to_dense(_getter(sd, device), p)


def pack_pe(sd, device, pe):
    return types.SimpleNamespace(dev=device, pe=PemWeights._pe(_getter(sd, device), pe))


# ------------------------------------------------------------------------------------------------- primitives
def gemm(A, W, bias, out, M, N, K, lda, ldw, ldc, *, residual=None, batch=1, **kw):
    """runtime.gemm, timed for bench.py where it is one of the dense-token projections."""
    if PROFILE is not None and batch == 1 and N == C and K == C and M >= 65536:
        # bench.py's second roofline: the dense-token projections (M = 2B x 2049 rows, 256 -> 256) are HBM streams
        PROFILE.setdefault("gemm_dense_256_bytes", []).append(4 * M * (K + N + (N if residual is not None else 0)) + 4 * N * K)
        with _Timed("gemm_dense_256"):
            runtime.gemm(A, W, bias, out, M, N, K, lda, ldw, ldc, residual=residual, batch=batch, **kw)
    else:
        runtime.gemm(A, W, bias, out, M, N, K, lda, ldw, ldc, residual=residual, batch=batch, **kw)


def linear(x2d, lin, *, act=0, residual=None, out=None, cloud_rows=0):
    """x2d (M,K) contiguous -> (M,N) = act(x W^T + b) (+ residual).  cloud_rows: tokens per cloud when the rows are the sparse tokens of
    whole clouds (<= 512 each): the projection then runs on the panel kernel."""
    M, K = x2d.shape
    N = lin.w.shape[0]
    if out is None:
        out = _empty((M, N), x2d)
    if cloud_rows and act == 0 and residual is None and K == C and M % cloud_rows == 0 and \
            rows_linear(x2d, lin, out, M, cloud_rows, cloud_rows, 0, cloud_rows, 0):
        return out
    gemm(x2d, lin.w, lin.b, out, M, N, K, K, K, N, residual=residual, ldr=N, act=act, w16=lin.w16())
    return out


def rows_linear(x, lin, out, M, rpb, x_bs, x_r0, o_bs, o_r0):
    """out rows = x rows @ lin.w^T + lin.b for M = clouds * rpb token rows of 256 channels; row R = (cloud R // rpb, token R % rpb) sits at
    row cloud * x_bs + x_r0 + token of x and cloud * o_bs + o_r0 + token of out (rows of 256 / lin.w.shape[0] floats).  False when the
    panel kernel does not serve this Linear / size (the caller then launches the GEMM)."""
    if not _flags().rows_linear or M <= 0 or rpb > 512:  # (by tokens per cloud, never by batch size: a shard must take the same path as the whole batch)
        return False
    pi = lin.pimg()
    if pi is None:
        return False
    _lib.call("sam6d_rows_linear", _p(x), pi[0].data_ptr(), pi[2], _p(lin.b), float(pi[1]), _p(out), M, rpb, x_bs, x_r0, o_bs, o_r0, _s())
    return True


def layernorm(x2d, gb, out=None):
    rows = x2d.shape[0]
    if out is None:
        out = torch.empty_like(x2d)
    _lib.call("sam6d_layernorm256", _p(x2d), _p(gb[0]), _p(gb[1]), _p(out), rows, C, C, 1e-5, _s())
    return out


def _post_attention(hidden, x2d, L, out=None):
    """linear -> +residual -> LayerNorm -> AttentionOutput (expand, ReLU, squeeze, +residual, LayerNorm)
    (PEM/model/transformer.py:152-199).  out: optional contiguous destination holding M x 256 floats."""
    M = hidden.shape[0]
    if out is not None:
        assert out.is_contiguous() and out.numel() == M * C
        out = out.view(M, C)
    if _fused_block() and "tb" in L:
        # linear + residual + LayerNorm + FFN + residual + LayerNorm in ONE launch: the 128-token tile never leaves the chip
        if out is None:
            out = _empty((M, C), hidden)
        tb = L["tb"]
        with _Timed("token_block"):
            _lib.call("sam6d_token_block", _p(hidden), _p(x2d), tb["img"].data_ptr(), _p(tb["cst"]), _p(out), M, 1e-5, _s())
        return out
    y = layernorm(linear(hidden, L["lin"], residual=x2d), L["n1"])
    h = linear(y, L["exp"], act=1)
    return layernorm(linear(h, L["sq"], residual=y), L["n2"], out=out)


def _fused_block():
    """The fused transformer-block kernels (csrc/block.hip) serve the split-precision mode; SAM6D_FUSED_BLOCK=0 keeps the
    launch-per-op path (also what matmul mode 0, the exact fp32 MFMA reference arithmetic, uses)."""
    return _flags().fused_block


# optional profiling hook: bench.py sets PROFILE = {} and reads back lists of (start, end) torch.cuda.Event pairs per
# kernel name.  Events are recorded on the launch stream and cost nothing when PROFILE is None.  An event pair is not free on
# the GPU (each record is a barrier packet: ~150 pairs per step cost 1.6 ms of a 9.4 ms step), so PROFILE_NAMES limits the
# recording to the kernels asked for (None = every instrumented site).
PROFILE = None
PROFILE_NAMES = None


class _Timed:
    """Profiling events around a launch site (PROFILE); nothing is recorded when PROFILE is None."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = PROFILE is not None and (PROFILE_NAMES is None or self.name in PROFILE_NAMES)
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.on:
            self.b.record()
            PROFILE.setdefault(self.name, []).append((self.a, self.b))


@on_tensor_device
def geo_embedding(points_bg, W, sigma_d=0.2, sigma_a=15, angle_k=3):
    """points_bg (B,n,3) with the bg point prepended -> (B,n,n,256)   (PEM/model/transformer.py:343-363)."""
    B, n, _ = points_bg.shape
    out = _empty((B, n, n, C), points_bg)
    knn = _empty((B * n * angle_k + 1,), points_bg, torch.int32)  # + the range flag
    idx = _empty((B, n, n, 4), points_bg)
    flag = knn.data_ptr() + 4 * B * n * angle_k
    factor_a = 180.0 / (sigma_a * math.pi)
    _lib.call("sam6d_geo_indices", _p(points_bg), B, n, float(sigma_d), float(factor_a), angle_k, _p(knn), _p(idx), _s())
    exact = lambda redo: _lib.call("sam6d_geo_embed", _p(idx), B * n * n, _p(W.div_term), _p(W.geo_d.w), _p(W.geo_d.b), _p(W.geo_a.w),
                                   _p(W.geo_a.b), C, flag, redo, _p(out), _s())
    if _flags().mode == 0 or not geo_images_in_range(W):
        # the exact fp32 kernel: mode 0's arithmetic, and the split-precision modes' when proj_d / proj_a (or their Chebyshev
        # coefficients) x 1024 leave the fp16 range -- the split-precision images of this weight set would hold inf; slower, never wrong
        with _Timed("geo_embed_kernel"):
            exact(0)
        return out
    lst = _empty((B * n * n + 1,), points_bg, torch.int32)  # [count | pair ids outside the Chebyshev range]
    pos = _empty((B * n * n,), points_bg, torch.int32)  # pair -> list slot or -1
    with _Timed("geo_embed_kernel"):
        _lib.call("sam6d_geo_embed_cheb", _p(idx), B * n * n, geo_cheb_packed(W).data_ptr(), float(GEO_XMAX), _p(W.div_term),
                  geo_packed(W).data_ptr(), _p(W.geo_d.b), _p(W.geo_a.b), C, flag, _p(pos), _p(lst), _p(out), _s())
    # indices beyond the fast sincos range (flag set on the device): this launch redoes the call exactly; otherwise it returns immediately
    exact(1)
    return out


GEO_XMAX = 24.0  # Chebyshev range of the embedding indices (d_idx = dist / 0.2, a_idx <= 12); beyond it: the sin/cos kernel
GEO_CHEB_K = 32


def cheb_coefficients(weight, div_term, xmax=GEO_XMAX, K=GEO_CHEB_K):
    """Chebyshev interpolant (degree K-1, float64) of x -> weight @ sinusoid(x) on [0, xmax], one row per output column:
    returns c (cols, K) with  weight @ [sin(w0 x), cos(w0 x), sin(w1 x), ...] ~= sum_p c[:, p] T_p(2x/xmax - 1)
    (SinusoidalPositionalEmbedding: PEM/model/transformer.py:259-285; error ~4e-12 for xmax = 24, K = 32)."""
    Wm = weight.detach().double().cpu().numpy()  # (cols, 256) over interleaved [sin, cos]
    om = div_term.detach().double().cpu().numpy()  # (128,)
    k = np.arange(K)
    u = np.cos(np.pi * (k + 0.5) / K)
    ph = ((u + 1.0) * (xmax / 2.0))[:, None] * om[None, :]
    emb = np.stack([np.sin(ph), np.cos(ph)], -1).reshape(K, -1)  # (K nodes, 256)
    F = emb @ Wm.T  # (K nodes, cols)
    T = np.cos(np.outer(np.arange(K), np.arccos(u)))  # T[p, node]
    c = (2.0 / K) * (T @ F)
    c[0] *= 0.5
    return c.T.copy()  # (cols, K)


def geo_cheb_packed(W):
    """Chebyshev coefficient matrices of proj_d / proj_a as geo_cheb_kernel's LDS image: [mat][col][32 hi | 32 lo | 8 pad]
    fp16 halves of (c * 1024); built once per weight set on the host in float64."""
    pk = getattr(W, "_geo_cheb", None)
    if pk is None:
        c = np.stack([cheb_coefficients(W.geo_d.w, W.div_term), cheb_coefficients(W.geo_a.w, W.div_term)], 0) * 1024.0
        # the images hold (coefficient x 1024) and (weight x 1024) as fp16 hi / lo halves: both matrices of both must stay finite there
        wmax = max(float(W.geo_d.w.abs().max()), float(W.geo_a.w.abs().max())) * 1024.0
        W._geo_img_fits = bool(np.abs(c).max() < 60000.0 and wmax < 60000.0)
        c32 = np.clip(c, -65000.0, 65000.0).astype(np.float32)  # (an out-of-range image is never used: geo_images_in_range)
        hi = c32.astype(np.float16)
        lo = (c32 - hi.astype(np.float32)).astype(np.float16)
        img = np.concatenate([hi, lo, np.zeros((2, C, 8), np.float16)], axis=2)  # (2, 256, 72 halves = 144 B)
        pk = torch.from_numpy(np.ascontiguousarray(img)).to(W.geo_d.w.device)
        W._geo_cheb = pk
        # rpe_score_kernel converts the projected angular embedding (x 1024) to fp16 hi / lo for its second contraction: |T_p| <= 1, so
        # sum_p |1024 c[ch][p]| bounds every value it can meet.  Weights beyond the fp16 range take the materialised-embedding path.
        W._geo_cheb_fits = bool(W._geo_img_fits and np.abs(c[1]).sum(axis=1).max() < 60000.0)
    return pk


def geo_cheb_a_packed(W, sigma_a=15):
    """proj_a's Chebyshev image for the fused score kernel (rpe.hip), on the range the angular indices actually live on: the angle of
    get_embedding_indices (PEM/model/transformer.py:326-341) is at most pi, so a_idx = angle * 180 / (sigma_a pi) <= 180 / sigma_a
    (12 for the reference's sigma_a = 15) against GEO_XMAX = 24 for the distance index.  On the shorter range the coefficients fall
    off twice as fast (|c_p| ~ J_p(xmax_a / 2)), which is what lets the kernel drop the cross terms of the orders >= 16.
    Returns (image (256, 72) fp16 = [32 hi | 32 lo | pad] of c * 1024, xmax_a, products, fits):
      products = 2 when, for every channel, 2^-10 sum_{p >= 16} |c[ch][p]| <= 3e-8 of that channel's bound sum_p |c[ch][p]| (never
                 below 1e-3 of the largest channel's) -- half an fp32 ulp of the values the reference computes -- else 3;
      fits     = sum_p |1024 c[ch][p]| < 60 000 (the kernel's fp16 split of the projected embedding cannot overflow)."""
    cache = getattr(W, "_geo_cheb_a", None)
    if cache is None:
        cache = W._geo_cheb_a = {}
    key = float(sigma_a)
    hit = cache.get(key)
    if hit is None:
        xmax_a = min(float(GEO_XMAX), (180.0 / float(sigma_a)) * (1.0 + 2.0 ** -6))
        c = cheb_coefficients(W.geo_a.w, W.div_term, xmax=xmax_a)  # (256, 32) float64
        bound = np.abs(c).sum(axis=1)
        tail = np.abs(c[:, 16:]).sum(axis=1) * 2.0 ** -10
        floor = max(float(bound.max()) * 1e-3, 1e-30)
        products = 2 if bool(np.all(tail <= 3e-8 * np.maximum(bound, floor))) else 3
        fits = bool(geo_images_in_range(W) and (bound * 1024.0).max() < 60000.0)
        c32 = np.clip(c * 1024.0, -65000.0, 65000.0).astype(np.float32)
        hi = c32.astype(np.float16)
        lo = (c32 - hi.astype(np.float32)).astype(np.float16)
        img = np.concatenate([hi, lo, np.zeros((C, 8), np.float16)], axis=1)  # (256, 72 halves = 144 B)
        hit = cache[key] = (torch.from_numpy(np.ascontiguousarray(img)).to(W.geo_d.w.device), xmax_a, products, fits)
    return hit


def geo_images_in_range(W):
    """True when proj_d / proj_a x 1024 and their Chebyshev coefficients x 1024 are all finite in fp16, i.e. the split-precision
    embedding kernels (sam6d_geo_embed_cheb / _h3 and the outlier rows) can serve this weight set; otherwise geo_embedding uses the
    exact fp32 kernel."""
    geo_cheb_packed(W)
    return W._geo_img_fits


def fused_rpe_in_range(W, sigma_a=15):
    """True when the fused RPE score kernel's fp16 split of the projected embedding cannot overflow for this weight set."""
    return geo_cheb_a_packed(W, sigma_a)[3]


def geo_packed(W):
    """proj_d / proj_a split into fp16 hi/lo (scaled by 1024) and tiled [kc][mat][col][16 hi | 16 lo | 8 pad] for
    geo_embed_h3_kernel; built once per weight set.  The split is a HIP kernel, the re-tiling pure data movement."""
    pk = getattr(W, "_geo_pack", None)
    if pk is None:
        both = torch.stack([W.geo_d.w, W.geo_a.w], 0).contiguous()  # (2, 256 cols, 256 k)
        hi = torch.empty(both.shape, dtype=torch.float16, device=both.device)
        lo = torch.empty_like(hi)
        _lib.call("sam6d_split_f16", _p(both), both.numel(), 1024.0, hi.data_ptr(), lo.data_ptr(), _s())
        t = lambda x: x.view(2, C, 16, 16).permute(2, 0, 1, 3)  # (kc, mat, col, 16)
        pad = torch.zeros(16, 2, C, 8, dtype=torch.float16, device=both.device)
        pk = torch.cat([t(hi), t(lo), pad], dim=3).contiguous()  # (16, 2, 256, 40): the kernel's LDS row image (80 B)
        W._geo_pack = pk
    return pk


class GeoContext:
    """What the fused RPE attention needs instead of the (B,n,n,256) embedding tensor: the per-pair embedding indices, the
    map pair -> stored row for the pairs outside the Chebyshev range, those rows, and the packed coefficient matrices."""
    __slots__ = ("B", "n", "idx", "pos", "rows", "wa_cheb", "xmax_a", "products", "dcT", "dcT16", "keep")


def geo_context(points_bg, W, sigma_d=0.2, sigma_a=15, angle_k=3):
    """points_bg (B,n,3) with the bg point prepended -> GeoContext (GeometricStructureEmbedding without its output tensor:
    PEM/model/transformer.py:306-363; the projections are applied inside sam6d_rpe_scores)."""
    B, n, _ = points_bg.shape
    pairs = B * n * n
    img, xmax_a, products, fits = geo_cheb_a_packed(W, sigma_a)
    if not fits:
        raise ValueError("geo_context: proj_a of this weight set exceeds the fp16 range of the fused RPE score kernel "
                         "(sum |Chebyshev coefficients| >= 58.6 per channel); use geo_embedding (SAM6D_FUSED_RPE=0)")
    knn = _empty((B * n * angle_k + 1,), points_bg, torch.int32)  # + the range flag
    idx = _empty((B, n, n, 4), points_bg)
    flag = knn.data_ptr() + 4 * B * n * angle_k
    _lib.call("sam6d_geo_indices", _p(points_bg), B, n, float(sigma_d), float(180.0 / (sigma_a * math.pi)), angle_k, _p(knn),
              _p(idx), _s())
    G = GeoContext()
    G.B, G.n, G.idx = B, n, idx
    G.pos = _empty((pairs,), points_bg, torch.int32)
    lst = _empty((pairs + 1,), points_bg, torch.int32)
    G.rows = _empty((pairs, C), points_bg)  # capacity for the worst case; only the listed rows are ever touched
    _lib.call("sam6d_geo_outliers2", _p(idx), pairs, float(GEO_XMAX), float(xmax_a), _p(W.div_term), geo_packed(W).data_ptr(),
              _p(W.geo_d.w), _p(W.geo_a.w), flag, _p(G.pos), _p(lst), _p(G.rows), _s())
    G.wa_cheb = img.data_ptr()  # proj_a's expansion on [0, xmax_a]
    G.xmax_a = xmax_a
    G.products = 3 if _flags().rpe_products == 3 else products
    G.dcT = geo_dcT(W)
    G.dcT16 = geo_dcT16(W)
    G.keep = (knn, lst, img)
    return G


def geo_dcT(W):
    """(32, 256) fp32: Chebyshev coefficients of proj_d, transposed -- the W operand of qd = qp @ D_c."""
    d = getattr(W, "_geo_dcT", None)
    if d is None:
        c = cheb_coefficients(W.geo_d.w, W.div_term)  # (256, 32) float64
        d = torch.from_numpy(c.T.copy()).to(device=W.geo_d.w.device, dtype=torch.float32).contiguous()
        W._geo_dcT = d
    return d


def geo_dcT16(W):
    d = getattr(W, "_geo_dcT16", None)
    if d is None:
        d = W._geo_dcT16 = split_w16(geo_dcT(W))
    return d


def gemm_b2(A, Wt, out, M, N, K, lda, ldw, ldc, batch, sA, sW, sC, batch2, sA2, sW2, sC2, a_off=0, w_off=0, c_off=0):
    _lib.call("sam6d_gemm_nt_b2", _p(A, a_off), _p(Wt, w_off), _p(out, c_off), M, N, K, lda, ldw, ldc, batch, sA, sW, sC, batch2,
              sA2, sW2, sC2, _s())


def pack_rpe_front(L, dcT):
    """Panel image of csrc/block.hip's rpe_front_kernel for one self layer: [Wq;Wk;Wv] | per head proj_p^T columns 64h.. | D_c^T."""
    dev = L["qkv"].w.device
    nbytes = int(_lib.load().sam6d_rpe_front_image_bytes())
    assert nbytes == 24 * TB_P256 + 32 * TB_P64 + TB_P256
    img = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    s_qkv, s_wp, s_dc = _pow2_scale(L["qkv"].w.abs().max()), _pow2_scale(L["wpT"].abs().max()), _pow2_scale(dcT.abs().max())
    _lib.call("sam6d_pack_panels", _p(L["qkv"].w), C, 3 * C, 0, 8, float(s_qkv), img.data_ptr(), _s())
    for h in range(H):
        _lib.call("sam6d_pack_panels", _p(L["wpT"]), C, C, 64 * h, 2, float(s_wp), img.data_ptr() + 24 * TB_P256 + h * 8 * TB_P64, _s())
    _lib.call("sam6d_pack_panels", _p(dcT), C, 32, 0, 8, float(s_dc), img.data_ptr() + 24 * TB_P256 + 32 * TB_P64, _s())
    return dict(img=img, inv=(1.0 / s_qkv, 1.0 / s_wp, 1.0 / s_dc))


# the longest cloud the one-launch self attention (xattn.hip sattn_kernel) takes; longer clouds run q.k^T and P.v as batched GEMMs
SATTN_MAX_N = 208


def rpe_self_layer_fused(x, G, L):
    """rpe_self_layer without the embedding tensor (rpe.hip): the geometric term rebuilt from the Chebyshev basis inside the score
    kernel."""
    return _rpe_self_tail(x, G, L, *_rpe_self_front(x, G, L))


def _rpe_self_front(x, G, L):
    """(qkv, qp, qd, vT) of rpe_self_layer_fused: the q | k | v rows, the query folded into proj_p per head and qp folded into D_c;
    vT = the values transposed per cloud where the GEMM tail takes them (else None)."""
    Bp, n, _ = x.shape
    M = Bp * n
    x2 = x.reshape(M, C)
    if _flags().fused_front:
        # qkv projection, proj_p fold and D_c fold of the query in one launch (block.hip rpe_front_kernel)
        fr = L.get("front")
        if fr is None:
            fr = L["front"] = pack_rpe_front(L, G.dcT)
        qkv = _empty((M, 3 * C), x)
        qp = _empty((M, H * C), x)
        qd = _empty((M * H, 32), x)
        ldp = (n + 3) // 4 * 4
        if n <= SATTN_MAX_N:  # the attention kernel cuts k and v into its LDS images itself: plain q | k | v rows
            with _Timed("rpe_front"):
                _lib.call("sam6d_rpe_front", _p(x2), fr["img"].data_ptr(), _p(L["qkv"].b), fr["inv"][0], fr["inv"][1], fr["inv"][2],
                          _p(qkv), _p(qp), _p(qd), M, _s())
            return qkv, qp, qd, None
        vT = _empty((Bp, C, ldp), x)  # the values land transposed per cloud (the P.v operand): no transpose pass
        with _Timed("rpe_front"):
            _lib.call("sam6d_rpe_front_vt", _p(x2), fr["img"].data_ptr(), _p(L["qkv"].b), fr["inv"][0], fr["inv"][1], fr["inv"][2], _p(qkv),
                      _p(qp), _p(qd), M, _p(vT), n, ldp, _s())
        return qkv, qp, qd, vT
    qkv = linear(x2, L["qkv"])  # (M, 768): q | k | v
    qp = _empty((M, H * C), x)
    # (act 16: the two folds of the geometric embedding into the query stay at fp16 x3 in matmul mode 2 -- "fp32 geometry")
    gemm(qkv, L["wpT"], None, qp, M, C, 64, 3 * C, C, H * C, batch=H, sA=64, sW=64, sC=C, act=16, w16=L.get("wpT16"))
    qd = _empty((M * H, 32), x)
    gemm(qp, G.dcT, None, qd, M * H, 32, C, C, C, 32, act=16, w16=G.dcT16)
    return qkv, qp, qd, None


def _rpe_self_tail(x, G, L, qkv, qp, qd, vT=None):
    """q.k^T, geometric scores + softmax, P.v and the layer tail of rpe_self_layer_fused."""
    if x.shape[1] <= SATTN_MAX_N:
        return _rpe_self_tail_attention(x, G, L, qkv, qp, qd)
    return _rpe_self_tail_gemm(x, G, L, qkv, qp, qd, vT)


def _rpe_self_tail_attention(x, G, L, qkv, qp, qd):
    """The geometric score term alone, then q.k^T + softmax + P.v per (cloud, head) in one launch (xattn.hip sattn_kernel)."""
    Bp, n, _ = x.shape
    M = Bp * n
    ldp = (n + 3) // 4 * 4
    Gs = _empty((M, H, ldp), x)
    with _Timed("rpe_score_kernel"):
        _lib.call("sam6d_rpe_geo_scores", _p(G.idx), _p(G.pos), _p(G.keep[1]), _p(G.rows), G.wa_cheb, float(GEO_XMAX),
                  float(G.xmax_a), int(G.products), _p(qp), _p(qd), _p(Gs), M, n, ldp, _s())
    hid = _empty((M, C), x)
    _lib.call("sam6d_rpe_self_attention", _p(qkv), _p(Gs), _p(hid), Bp, n, ldp, _s())
    return _post_attention(hid, x.reshape(M, C), L).reshape(Bp, n, C)


def _rpe_self_tail_gemm(x, G, L, qkv, qp, qd, vT=None):
    """q.k^T and P.v as batched GEMMs, the softmax inside the score kernel; vT None: the values are transposed out of qkv."""
    Bp, n, _ = x.shape
    M = Bp * n
    ldp = (n + 3) // 4 * 4
    qk = _empty((M, H, ldp), x)
    P = _empty((M, H, ldp), x)
    gemm_b2(qkv, qkv, qk, n, n, 64, 3 * C, 3 * C, H * ldp, Bp, n * 3 * C, n * 3 * C, n * H * ldp, H, 64, 64, ldp, w_off=C)
    with _Timed("rpe_score_kernel"):
        _lib.call("sam6d_rpe_scores2", _p(G.idx), _p(G.pos), _p(G.keep[1]), _p(G.rows), G.wa_cheb, float(GEO_XMAX), float(G.xmax_a),
                  int(G.products), _p(qp), _p(qd), _p(qk), _p(P), M, n, ldp, _s())
    if vT is None:
        vT = _empty((Bp, C, ldp), x)
        _lib.call("sam6d_transpose", _p(qkv, 2 * C), 3 * C, n * 3 * C, Bp, n, C, _p(vT), ldp, C * ldp, _s())
    hid = _empty((M, C), x)
    gemm_b2(P, vT, hid, n, 64, n, H * ldp, ldp, C, Bp, n * H * ldp, C * ldp, n * C, H, ldp, 64 * ldp, 64)
    return _post_attention(hid, x.reshape(M, C), L).reshape(Bp, n, C)


def rpe_self_layer(x, E, L):
    """x (B',n,256), E (B',n,n,256) -> (B',n,256)   RPETransformerLayer (PEM/model/transformer.py:366-479)."""
    if isinstance(E, GeoContext):
        return rpe_self_layer_fused(x, E, L)
    Bp, n, _ = x.shape
    M = Bp * n
    x2 = x.reshape(M, C)
    qkv = linear(x2, L["qkv"])  # (M, 768): q | k | v
    qp = _empty((M, H * C), x)
    # qp[:, h, :] = q_h @ Wp[h*64:(h+1)*64, :]  -- 4 head problems as one batched launch
    gemm(qkv, L["wpT"], None, qp, M, C, 64, 3 * C, C, H * C, batch=H, sA=64, sW=64, sC=C, w16=L.get("wpT16"))
    hid = _empty((M, C), x)
    _lib.call("sam6d_attention", _p(qkv), _p(qkv, C), _p(qkv, 2 * C), _p(qp), _p(E), _p(hid), Bp, n, n, 3 * C, 3 * C, 3 * C,
              C, n * 3 * C, n * 3 * C, n * 3 * C, n * C, _s())
    return _post_attention(hid, x2, L).reshape(Bp, n, C)


def cross_layer(x, mem, L, out=None):
    """x (B,n,256) attends to mem (B,m,256)   TransformerLayer (PEM/model/transformer.py:95-226).  out: optional (B,n,256) view to write
    the layer's output into (a slice of the caller's stacked token buffer)."""
    B, n, _ = x.shape
    m = mem.shape[1]
    x2 = x.reshape(B * n, C)
    hid = _empty((B * n, C), x)
    if _fused_block() and "xq" in L and n <= 256 and m <= 208:
        # proj_q, proj_k, proj_v + softmax attention of all four heads in one launch on the matrix cores (xattn.hip)
        with _Timed("cross_attention"):
            if "xkv" in L:
                _lib.call("sam6d_cross_attention_kv", _p(x2), _p(mem), L["xq"]["img"].data_ptr(), _p(L["q"].b), float(L["xq"]["inv"]),
                          L["xkv"]["img"].data_ptr(), _p(L["kv"].b), float(L["xkv"]["inv"]), _p(hid), B, n, m, _s())
            else:
                kv = linear(mem.reshape(B * m, C), L["kv"])  # (B*m, 512): k | v
                _lib.call("sam6d_cross_attention", _p(x2), _p(kv), L["xq"]["img"].data_ptr(), _p(L["q"].b), float(L["xq"]["inv"]), _p(hid),
                          B, n, m, _s())
        return _post_attention(hid, x2, L, out=out).reshape(B, n, C)
    kv = linear(mem.reshape(B * m, C), L["kv"])  # (B*m, 512): k | v
    q = linear(x2, L["q"])
    _lib.call("sam6d_attention", _p(q), _p(kv), _p(kv, C), None, None, _p(hid), B, n, m, C, 2 * C, 2 * C, C, n * C, m * 2 * C,
              m * 2 * C, n * C, _s())
    return _post_attention(hid, x2, L, out=out).reshape(B, n, C)


# ------------------------------------------------------------------------------ stand-alone sub-module forwards (drop-in API)
@on_tensor_device
def sinusoid_embedding(x, div_term, d_model):
    """x (n) -> (n, d_model)   SinusoidalPositionalEmbedding.forward (PEM/model/transformer.py:269-285)."""
    n = x.numel()
    out = _empty((n, d_model), x)
    dt = div_term.detach().float().contiguous()
    _lib.call("sam6d_sinusoid_embed", _p(x), n, _p(dt), int(d_model), _p(out), _s())
    return out


@on_tensor_device
def mha_forward(xq, xk, xv, lq, lk, lv, heads=H, embed_qk=None, proj_p=None):
    """MultiHeadAttention.forward / RPEMultiHeadAttention.forward (PEM/model/transformer.py:111-150, 383-420) as separate launches,
    WITH the attention probabilities as an output: xq (B,N,C), xk / xv (B,M,C) [, embed_qk (B,N,M,C)] -> hidden (B,N,C),
    probabilities (B,heads,N,M).  The fused kernels (sam6d_cross_attention_kv, sam6d_rpe_scores) are what the pipeline uses."""
    B, N, Cm = xq.shape
    M = xk.shape[1]
    if Cm != C or heads != H:
        raise ValueError("kernels are specialised for d_model=256, num_heads=4 (PEM/config/base.yaml)")
    q = linear(xq.reshape(B * N, C), lq)
    k = linear(xk.reshape(B * M, C), lk)
    v = linear(xv.reshape(B * M, C), lv)
    ldp = (M + 3) // 4 * 4
    qk = torch.zeros((B * N, H, ldp), dtype=torch.float32, device=xq.device)  # rows = query tokens, [head][key]
    gemm_b2(q, k, qk, N, M, 64, C, C, H * ldp, B, N * C, M * C, N * H * ldp, H, 64, 64, ldp)
    sp = None
    if embed_qk is not None:
        # q . proj_p(E) = (Wp_h^T q_h) . E + q_h . b_p;  the bias term is constant over the keys and cancels in the softmax
        wpT = proj_p.w.t().contiguous()
        qp = _empty((B * N, H * C), xq)
        gemm(q, wpT, None, qp, B * N, C, 64, C, C, H * C, batch=H, sA=64, sW=64, sC=C, act=16)
        sp = torch.zeros((B * N, H, ldp), dtype=torch.float32, device=xq.device)
        gemm(qp, embed_qk, None, sp, H, M, C, C, C, ldp, batch=B * N, sA=H * C, sW=M * C, sC=H * ldp, act=16)
    P = torch.zeros((B * N, H, ldp), dtype=torch.float32, device=xq.device)
    _lib.call("sam6d_scaled_softmax", _p(qk), _p(sp), 0.125, B * N * H, M, ldp, ldp, _p(P), ldp, _s())
    vT = torch.zeros((B, C, ldp), dtype=torch.float32, device=xq.device)
    _lib.call("sam6d_transpose", _p(v), C, M * C, B, M, C, _p(vT), ldp, C * ldp, _s())
    hid = _empty((B * N, C), xq)
    gemm_b2(P, vT, hid, N, 64, M, H * ldp, ldp, C, B, N * H * ldp, C * ldp, N * C, H, ldp, 64 * ldp, 64)
    probs = P.reshape(B, N, H, ldp)[..., :M].permute(0, 2, 1, 3).contiguous()
    return hid.reshape(B, N, C), probs


@on_tensor_device
def linear_attention_forward(xq, xk, xv, lq, lk, lv, scale, heads=H):
    """LinearAttention.forward (PEM/model/transformer.py:548-578): xq (B,I,C), xk / xv (B,J,C) -> (B,I,C); the kv contraction order."""
    B, I, Cm = xq.shape
    J = xk.shape[1]
    if Cm != C or heads != H:
        raise ValueError("kernels are specialised for d_model=256, num_heads=4 (PEM/config/base.yaml)")
    if not (I * J * 128 > 64 * 64 * (I + J)):
        raise NotImplementedError("linear attention: only the kv contraction order is implemented (transformer.py:569-572)")
    q = linear(xq.reshape(B * I, C), lq)
    kv = _empty((B * J, 2 * C), xq)
    gemm(xk.reshape(B * J, C), lk.w, lk.b, kv, B * J, C, C, C, C, 2 * C)
    gemm(xv.reshape(B * J, C), lv.w, lv.b, kv, B * J, C, C, C, C, 2 * C, c_off=C)
    _lib.call("sam6d_linattn_focus_k", _p(kv), _p(scale), B * J, 2 * C, _s())
    kvT = _empty((B, H, 64, 64), xq)
    ksum = _empty((B, H, 64), xq)
    _lib.call("sam6d_linattn_kv", _p(kv), _p(kv, C), B, J, 2 * C, 2 * C, J * 2 * C, J * 2 * C, _p(kvT), _p(ksum), _s())
    _lib.call("sam6d_linattn_focus_q", _p(q), _p(scale), _p(ksum), B, I, C, _s())
    hid = _empty((B * I, C), xq)
    _linattn_contract(q, kvT, hid, B, I)
    return hid.reshape(B, I, C)


def _linattn_contract(q, kvT, hid, Bn, I):
    """hid[:, h] = (phi(q)_h z_h) @ kv_h for the four heads, batched over the Bn clouds: the last step of the launch-per-op linear
    attention.  In matmul mode 1 these four GEMMs run on the exact fp32 loop of mode 0.  Cubing spreads a row of phi(q) z over twenty
    orders of magnitude under a maximum near 2^-6, the lower end of the range in which sam6d_gemm_nt keeps the fp16 split: the lo halves
    are fp16 subnormals there, every element carries 2^-25 absolute, and kv^T holds entries of a few hundred -- the split product was
    off by 1.4e-5 of the largest output at (B, I, J) = (2, 300, 197), the exact loop by 1e-6.  (The fused layer scales every row by a
    power of two instead.)  64 x 64 weights: the loop's rate does not matter."""
    exact = _flags().mode == 1
    if exact:
        prev = int(_lib.load().sam6d_get_thread_matmul_mode())
        _lib.call("sam6d_set_thread_matmul_mode", 0)
    try:
        for h in range(H):  # x_h = (phi(q)_h z) @ kv_h
            gemm(q, kvT, None, hid, I, 64, 64, C, 64, C, a_off=h * 64, w_off=h * 4096, c_off=h * 64, batch=Bn, sA=I * C, sW=H * 4096,
                 sC=I * C)
    finally:
        if exact:
            _lib.call("sam6d_set_thread_matmul_mode", prev)


def geometric_transformer(S, E, T):
    """S (2B,n,256) stacked [scene; template], E (2B,n,n,256) -> same shape
    (GeometricTransformer blocks ['self','cross'], sequential cross: PEM/model/transformer.py:483-527)."""
    B = S.shape[0] // 2
    S = rpe_self_layer(S, E, T["self"])
    out = torch.empty_like(S)  # the two cross layers write their halves of the stacked result directly (no copy pass)
    f0 = cross_layer(S[:B], S[B:], T["cross"], out=out[:B])
    cross_layer(S[B:], f0, T["cross"], out=out[B:])
    return out


def _stack(a, b):
    out = _empty((a.shape[0] * 2,) + tuple(a.shape[1:]), a)
    rows = a.shape[1]
    _lib.call("sam6d_put_rows", _p(a), rows * C, C, _p(out), rows * C, C, a.shape[0], rows, C, _s())
    _lib.call("sam6d_put_rows", _p(b), rows * C, C, _p(out, a.shape[0] * rows * C), rows * C, C, b.shape[0], rows, C, _s())
    return out


def linear_transformer_layer(D, S, L):
    """D (B',I,256) dense tokens (row 0 = bg slot, recomputed by the caller), S (B',J+1,256) sparse tokens (row 0 = bg).
    LinearTransformerLayer on D[:,1:] with memory S[:,1:] (PEM/model/transformer.py:581-622, 707-719); the bg rows of
    D ride along through the row kernels and are overwritten afterwards."""
    Bp, I, _ = D.shape
    J = S.shape[1] - 1
    rows = Bp * I
    D2 = D.reshape(rows, C)
    if not (I * J * 128 > 64 * 64 * (I + J)):
        raise RuntimeError("linear attention: only the kv contraction order is implemented (transformer.py:569-572)")
    kv = _empty((Bp, J, 2 * C), D)
    if not rows_linear(S, L["kv"], kv, Bp * J, J, J + 1, 1, J, 0):
        gemm(S, L["kv"].w, L["kv"].b, kv, J, 2 * C, C, C, C, 2 * C, a_off=C, batch=Bp, sA=(J + 1) * C, sC=J * 2 * C, w16=L["kv"].w16())
    ksum = _empty((Bp, H, 64), D)
    if _fused_block() and "tbd" in L:
        # the whole layer on the dense tokens (rows 1 .. I-1 of every cloud) in one launch; row 0 (the bg slot) is written by the caller
        tb = L["tbd"]
        kvimg = torch.empty(Bp * TB_P64 * 8, dtype=torch.uint8, device=D.device)
        kvinv = _empty((Bp, 4), D)  # one image scale per head
        # phi(k), kv^T, the key sums and the packed fp16 image of kv^T in one launch (was focus_k + kv + kv_pack)
        _lib.call("sam6d_linattn_kv_image", _p(kv), _p(L["scale"]), Bp, J, 2 * C, J * 2 * C, kvimg.data_ptr(), _p(kvinv), _p(ksum), _s())
        Dn = _empty((Bp, I, C), D)
        with _Timed("linattn_layer"):
            _lib.call("sam6d_linattn_layer", _p(D), tb["img"].data_ptr(), _p(tb["cst"]), kvimg.data_ptr(), _p(kvinv), _p(ksum), _p(Dn),
                      Bp, I, 1, 1e-5, _s())
        return Dn
    _lib.call("sam6d_linattn_focus_k", _p(kv), _p(L["scale"]), Bp * J, 2 * C, _s())
    kvT = _empty((Bp, H, 64, 64), D)
    _lib.call("sam6d_linattn_kv", _p(kv), _p(kv, C), Bp, J, 2 * C, 2 * C, J * 2 * C, J * 2 * C, _p(kvT), _p(ksum), _s())
    q = linear(D2, L["q"])
    _lib.call("sam6d_linattn_focus_q", _p(q), _p(L["scale"]), _p(ksum), Bp, I, C, _s())
    hid = _empty((rows, C), D)
    _linattn_contract(q, kvT, hid, Bp, I)
    return _post_attention(hid, D2, L).reshape(Bp, I, C)


@on_tensor_device
def sparse_to_dense_transformer(D, E, fps_idx, T, lead=None, write_bg=True, return_sparse=False):
    """D (2B,N+1,256) dense tokens incl. bg row, E (2B,n,n,256), fps_idx (2B,n-1) i32 -> new D
    (SparseToDenseTransformer, PEM/model/transformer.py:627-720, incl. the index-into-the-cat quirk :667-705).
    lead: (2B, >=1, 256) tensor whose row 0 per cloud is the bg token of D (default: D itself).  Between the blocks of the fine stage
    nothing reads row 0 of D but the next block's gather, so fine_point_matching hands the previous block's sparse tokens on as `lead`
    and writes the bg row of D (write_bg) after the last block only: one small launch per block instead of three."""
    Bp, I, _ = D.shape
    n1 = fps_idx.shape[1]
    S = _empty((Bp, n1 + 1, C), D)
    ld = D if lead is None else lead
    _lib.call("sam6d_gather_rows_lead", _p(D), _p(fps_idx), Bp, I, n1, C, I * C, (n1 + 1) * C, 0, _p(ld), ld.shape[1] * C, _p(S), _s())
    S = geometric_transformer(S, E, T)
    Dn = linear_transformer_layer(D, S, T["dense"])
    if write_bg:
        _lib.call("sam6d_put_rows", _p(S), (n1 + 1) * C, C, _p(Dn), I * C, C, Bp, 1, C, _s())
    return (Dn, S) if return_sparse else Dn


def pe_group(pts, r1=0.1, r2=0.2, ns1=32, ns2=64):
    """The two ball queries of PositionalEncoding (fine_point_matching.py:108-131; new_xyz = pts + 1e-8, :117) in one pass:
    ((idx1, idx2), (cnt1, cnt2)), cnt = the slots of a point that hold hits (the rest repeat slot 0)."""
    Bp, N, _ = pts.shape
    q = _empty((Bp, N, 3), pts)
    _lib.call("sam6d_add_scalar", _p(pts), 0.00000001, Bp * N * 3, _p(q), _s())
    idx12 = (_empty((Bp, N, ns1), pts, torch.int32), _empty((Bp, N, ns2), pts, torch.int32))
    nbytes = int(_lib.load().sam6d_ball_query2_grid_workspace_bytes(Bp, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    cnt12 = (_empty((Bp, N), pts, torch.int32), _empty((Bp, N), pts, torch.int32))
    with _Timed("ball_query"):
        _lib.call("sam6d_ball_query2_grid_counts", _p(q), _p(pts), Bp, N, N, float(r1), ns1, _p(idx12[0]), float(r2), ns2, _p(idx12[1]),
                  ws.data_ptr(), nbytes, _p(cnt12[0]), _p(cnt12[1]), _s())
    return idx12, cnt12


def pe_apply(pts, grp, W, dst, dst_off, dst_sb, max_wg=0):
    """dst rows += mlp3(cat(max_s mlp1(group_r1), max_s mlp2(group_r2))) for the groups (indices, counts) of pe_group.  max_wg: bound on
    the persistent workgroups of the MLP kernels (0 = fill the chip) for launches that share the chip with another stream."""
    Bp, N, _ = pts.shape
    idx12, cnt12 = grp
    feat = _empty((Bp * N, 2 * 128), pts)
    for k in range(2):
        idx = idx12[k]
        L = W.pe["mlp"][k]
        with _Timed("pe_mlp"):
            _lib.call("sam6d_pe_mlp_max_counted", _p(pts), _p(idx), Bp, N, idx.shape[2], _p(L[0]["w"]), _p(L[0]["scale"]), _p(L[0]["shift"]),
                      _p(L[1]["w"]), _p(L[1]["scale"]), _p(L[1]["shift"]), _p(L[2]["w"]), _p(L[2]["scale"]), _p(L[2]["shift"]),
                      _p(feat), 2 * 128, k * 128, int(max_wg), _p(cnt12[k]), _s())
    m3 = W.pe["mlp3"]
    gemm(feat, m3.w, m3.b, dst, N, C, C, C, C, C, c_off=dst_off, residual=dst, r_off=dst_off, ldr=C, batch=Bp, sA=N * C,
         sC=dst_sb, sR=dst_sb, w16=m3.w16())


@on_tensor_device
def positional_encoding_add(pts, W, dst, dst_off, dst_sb, r1=0.1, r2=0.2, ns1=32, ns2=64):
    """dst[b, 1 + i, :] += mlp3(cat(max_s mlp1(group_r1), max_s mlp2(group_r2)))   (PositionalEncoding,
    PEM/model/fine_point_matching.py:102-144).  pts (B',N,3); dst rows addressed by (dst_off, batch stride dst_sb)."""
    pe_apply(pts, pe_group(pts, r1, r2, ns1, ns2), W, dst, dst_off, dst_sb)


def feature_similarity(F, B, n, out_proj, temp):
    """F (2B,n,256) -> atten (B,n,n) = normalize(out_proj(F0)) @ normalize(out_proj(F1))^T / temp
    (PEM/utils/model_utils.py:131-153)."""
    f = linear(F.reshape(2 * B * n, C), out_proj, cloud_rows=n)
    _lib.call("sam6d_l2norm256", _p(f), _p(f), 2 * B * n, C, C, _s())
    att = _empty((B, n, n), F)
    gemm(f, f, None, att, n, n, C, C, C, n, w_off=B * n * C, batch=B, sA=n * C, sW=n * C, sC=n * n, divisor=temp)
    return att


def _assign_buffers(att):
    """the statistics and labels of a soft assignment of att (B,R,C): rmax / rsum (B,R), cmax / csum (B,C), l1 (B,R-1), l2 (B,C-1)"""
    B, R, Cn = att.shape
    return dict(rmax=_empty((B, R), att), rsum=_empty((B, R), att), cmax=_empty((B, Cn), att), csum=_empty((B, Cn), att),
                l1=_empty((B, R - 1), att, torch.int32), l2=_empty((B, Cn - 1), att, torch.int32))


def soft_assign(att):
    B, R, Cn = att.shape
    st = _assign_buffers(att)
    ws = _empty((32 * B * Cn,), att)
    _lib.call("sam6d_soft_assign", _p(att), B, R, Cn, _p(st["rmax"]), _p(st["rsum"]), _p(st["cmax"]), _p(st["csum"]),
              _p(st["l1"]), _p(st["l2"]), _p(ws), ws.numel(), _s())
    return st


@on_tensor_device
def compute_coarse_Rt(att, pts1, pts2, model, radius, rand, n_proposal1=6000, n_proposal2=300, return_aux=False):
    """PEM/utils/model_utils.py:204-275.  model (B,P,3) RAW CAD points and radius (B,): the division
    model / (radius + 1e-6) of coarse_point_matching.py:60 happens inside the scoring kernel.
    rand (B, 3*n_proposal1): the uniforms the reference draws with torch.rand (model_utils.py:292)."""
    B, R, Cn = att.shape
    N1, N2 = R - 1, Cn - 1
    L = N1 * N2
    w = _empty((B, L), att)
    w1 = _empty((B, N1), att)
    if (R * Cn + 3 * R + 3 * Cn) * 4 <= 160 * 1024:
        # the whole soft assignment of a proposal from LDS, one launch (bit-identical to the two calls below)
        st = _assign_buffers(att)
        _lib.call("sam6d_coarse_soft_assign", _p(att), B, R, Cn, _p(st["rmax"]), _p(st["rsum"]), _p(st["cmax"]), _p(st["csum"]),
                  _p(st["l1"]), _p(st["l2"]), _p(w), _p(w1), _s())
    else:
        st = soft_assign(att)
        _lib.call("sam6d_coarse_weights", _p(att), B, R, Cn, _p(st["rmax"]), _p(st["rsum"]), _p(st["cmax"]), _p(st["csum"]),
                  _p(st["l1"]), _p(st["l2"]), _p(w), _p(w1), _s())
    ns = 3 * n_proposal1
    cum = _empty((B, L), att)
    idx = _empty((B, ns), att, torch.int32)
    _lib.call("sam6d_weighted_sample", _p(w), _p(rand), B, L, ns, _p(cum), _p(idx), _s())
    Rs = _empty((B, n_proposal1, 9), att)
    ts = _empty((B, n_proposal1, 3), att)
    dis = _empty((B, n_proposal1), att)
    _lib.call("sam6d_coarse_hypotheses", _p(idx), _p(pts1), _p(pts2), B, N1, N2, n_proposal1, _p(Rs), _p(ts), _p(dis), _s())
    sel = _empty((B, n_proposal2), att, torch.int32)
    _lib.call("sam6d_select_smallest", _p(dis), B, n_proposal1, n_proposal2, _p(sel), _s())
    scores = _empty((B, n_proposal2), att)
    Rb = _empty((B, 3, 3), att)
    tb = _empty((B, 3), att)
    best = _empty((B,), att, torch.int32)
    if model.shape[1] <= 4096:
        # the K = 3 distance contraction on the fp32 matrix cores (same bits), weighted distances staged in a workspace
        ws = _empty((B * N1 * n_proposal2,), att)
        with _Timed("score_hyp"):
            _lib.call("sam6d_score_select_hypotheses_ws", _p(sel), _p(Rs), _p(ts), _p(pts1), _p(w1), _p(model), _p(radius), B, N1,
                      model.shape[1], n_proposal1, n_proposal2, _p(scores), _p(Rb), _p(tb), _p(best), _p(ws), ws.numel() * 4, _s())
    else:
        with _Timed("score_hyp"):
            _lib.call("sam6d_score_select_hypotheses", _p(sel), _p(Rs), _p(ts), _p(pts1), _p(w1), _p(model), _p(radius), B, N1,
                      model.shape[1], n_proposal1, n_proposal2, _p(scores), _p(Rb), _p(tb), _p(best), _s())
    if return_aux:
        return Rb, tb, dict(weights=w, w1=w1, idx=idx, dis=dis, top=sel, scores=scores, best=best, Rs=Rs, ts=ts, cum=cum)
    return Rb, tb


@on_tensor_device
def pairwise_distance(x, y):
    """PEM/utils/model_utils.py:101-128 on (B,N,3) x (B,M,3) -> (B,N,M) squared distances, torch-CPU bit recipe."""
    _chk(x, "x", torch.float32, 3)
    _chk(y, "y", torch.float32, 3)
    B, N, _ = x.shape
    M = y.shape[1]
    if y.shape[0] != B or x.shape[2] != 3 or y.shape[2] != 3:
        raise RuntimeError("pairwise_distance: need x (B,N,3) and y (B,M,3)")
    out = _empty((B, N, M), x)
    _lib.call("sam6d_pairwise_distance", _p(x), _p(y), B, N, M, _p(out), _s())
    return out


@on_tensor_device
def weighted_procrustes(src, ref, weights=None, weight_thresh=0.0, eps=1e-5):
    """PEM/utils/model_utils.py:343-436: (B,N,3) x2 [+ (B,N)] -> R (B,3,3), t (B,3)."""
    B, N, _ = src.shape
    R = _empty((B, 3, 3), src)
    t = _empty((B, 3), src)
    _lib.call("sam6d_weighted_procrustes", _p(src), _p(ref), _p(weights), B, N, float(weight_thresh), float(eps), _p(R),
              _p(t), _s())
    return R, t


def _fine_pose_tail(pred, wgt, l1, pts1, model, radius, dis_thres):
    """The tail of both fine-pose forms (PEM/utils/model_utils.py:331-341): the weighted Procrustes pred -> pts1, then the share of the
    labelled scene points within dis_thres of the CAD cloud.  -> R (B,3,3), t (B,3) times (radius + 1e-6), score (B,)"""
    B, N = wgt.shape
    R, t = weighted_procrustes(pred, pts1, wgt, 0.0)
    cnt = _empty((B, 2), pred)
    score = _empty((B,), pred)
    _lib.call("sam6d_fine_score", _p(pts1), _p(R), _p(t), _p(model), _p(radius), _p(l1), B, N, model.shape[1], float(dis_thres),
              _p(cnt), _p(score), _s())
    return R, t, score


@on_tensor_device
def compute_fine_Rt(att, pts1, pts2, model, radius, dis_thres=0.15):
    """PEM/utils/model_utils.py:308-341 + the translation rescale of fine_point_matching.py:78.
    Returns R (B,3,3), t (B,3) already multiplied by (radius + 1e-6), score (B,)."""
    B, R_, Cn = att.shape
    st = soft_assign(att)
    pred = _empty((B, R_ - 1, 3), att)
    wgt = _empty((B, R_ - 1), att)
    _lib.call("sam6d_fine_assign", _p(att), B, R_, Cn, _p(st["rmax"]), _p(st["rsum"]), _p(st["cmax"]), _p(st["csum"]),
              _p(st["l1"]), _p(st["l2"]), _p(pts2), _p(pred), _p(wgt), _s())
    return _fine_pose_tail(pred, wgt, st["l1"], pts1, model, radius, dis_thres)


def fine_match_min_temp():
    """the smallest temperature the fused fine-match pipeline serves (its fixed softmax shift 1 / temp: csrc/finematch.hip FM_MIN_TEMP)"""
    return float(_lib.load().sam6d_fine_match_min_temp())


@on_tensor_device
def fine_match(f, B, n, temp, pts2):
    """f (2B*n, 256) out_proj outputs [scene clouds; template clouds] -- or the pair (fh, fl) of sam6d_linear_norm_split -- -> label1,
    label2 (B,n-1) i32, pred (B,n-1,3), weight (B,n-1)
    (compute_feature_similarity + the soft-assignment head of compute_fine_Rt, PEM/utils/model_utils.py:131-153, 308-331).
    temp >= fine_match_min_temp(); smaller temperatures take feature_similarity + compute_fine_Rt."""
    if not float(temp) >= fine_match_min_temp():
        raise ValueError("fine_match: temp = %g is below fine_match_min_temp() = %g" % (temp, fine_match_min_temp()))
    l1 = _empty((B, n - 1), pts2, torch.int32)
    l2 = _empty((B, n - 1), pts2, torch.int32)
    pred = _empty((B, n - 1, 3), pts2)
    wgt = _empty((B, n - 1), pts2)
    nbytes = int(_lib.load().sam6d_fine_match_workspace_bytes_n(B, n))
    if nbytes == 0:
        raise ValueError("fine_match: n = %d tokens per cloud (2049 or 4097 are built)" % n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pts2.device)
    with _Timed("fine_match"):
        if isinstance(f, tuple):
            _lib.call("sam6d_fine_match_split", f[0].data_ptr(), f[1].data_ptr(), B, n, float(temp), _p(pts2), _p(l1), _p(l2), _p(pred),
                      _p(wgt), ws.data_ptr(), nbytes, _s())
        else:
            _lib.call("sam6d_fine_match", _p(f), B, n, float(temp), _p(pts2), _p(l1), _p(l2), _p(pred), _p(wgt), ws.data_ptr(), nbytes, _s())
    return l1, l2, pred, wgt


def linear_norm_split(x, L, img=None):
    """x (M,256), L a 256 -> 256 Linear (img: its panel image, pack_cross_query(L)): (fh, fl) fp16 halves of normalize(L(x)) * 2^10 --
    out_proj, F.normalize and the operand split of the fine similarity in one pass (block.hip out_split_kernel)."""
    M = x.shape[0]
    if img is None:
        img = pack_cross_query(L)
    fh = torch.empty(M * C, dtype=torch.float16, device=x.device)
    fl = torch.empty(M * C, dtype=torch.float16, device=x.device)
    with _Timed("linear_norm_split"):
        _lib.call("sam6d_linear_norm_split", _p(x), img["img"].data_ptr(), _p(L.b), float(img["inv"]), fh.data_ptr(), fl.data_ptr(), M, _s())
    return fh, fl


def compute_fine_Rt_fused(f, B, n, temp, pts1, pts2, model, radius, dis_thres=0.15, return_aux=False):
    """compute_feature_similarity + compute_fine_Rt (PEM/utils/model_utils.py:131-153, 308-341) from the out_proj features."""
    pts2 = pts2.contiguous()
    l1, l2, pred, wgt = fine_match(f, B, n, temp, pts2)
    R, t, score = _fine_pose_tail(pred, wgt, l1, pts1, model, radius, dis_thres)
    if return_aux:
        return R, t, score, dict(l1=l1, l2=l2, pred=pred, weights=wgt)
    return R, t, score


# --------------------------------------------------------------------------------------------------- modules
def sample_pts_feats(pts, feats, npoint):
    """PEM/utils/model_utils.py:70-84 on (B',N,3) / (B',N,C): FPS + two row gathers."""
    Bp, N, _ = pts.shape
    idx = _empty((Bp, npoint), pts, torch.int32)
    temp = _empty((Bp, N), pts) if N > 4096 else None
    _lib.call("sam6d_furthest_point_sampling", _p(pts), Bp, N, npoint, _p(temp), _p(idx), _s())
    sp = _empty((Bp, npoint, 3), pts)
    _lib.call("sam6d_gather_rows", _p(pts), _p(idx), Bp, N, npoint, 3, N * 3, npoint * 3, 0, _p(sp), _s())
    if isinstance(feats, tuple):  # (scene, template) halves left where the caller holds them: no stacked copy of the features
        fa, fb = feats
        Cf, Bh = fa.shape[2], fa.shape[0]
        sf = _empty((Bp, npoint, Cf), pts)
        _lib.call("sam6d_gather_rows", _p(fa), _p(idx), Bh, N, npoint, Cf, N * Cf, npoint * Cf, 0, _p(sf), _s())
        _lib.call("sam6d_gather_rows", _p(fb), _p(idx, Bh * npoint), Bp - Bh, N, npoint, Cf, N * Cf, npoint * Cf, 0,
                  _p(sf, Bh * npoint * Cf), _s())
        return sp, sf, idx
    Cf = feats.shape[2]
    sf = _empty((Bp, npoint, Cf), pts)
    _lib.call("sam6d_gather_rows", _p(feats), _p(idx), Bp, N, npoint, Cf, N * Cf, npoint * Cf, 0, _p(sf), _s())
    return sp, sf, idx


def _tokens_with_bg(x, lin, bg, extra=None):
    """cat([bg_token, in_proj(x)], dim=1) for stacked x (B',N,256) -> (B',N+1,256)
    (PEM/model/coarse_point_matching.py:35-38, fine_point_matching.py:47-51)."""
    if isinstance(x, tuple):  # (scene, template) halves: two batched launches into the one token buffer
        xa, xb = x
        Ba, N, K = xa.shape
        Bp = Ba + xb.shape[0]
        T = _empty((Bp, N + 1, C), xa)
        gemm(xa, lin.w, lin.b, T, N, C, K, K, K, C, c_off=C, batch=Ba, sA=N * K, sC=(N + 1) * C, w16=lin.w16())
        gemm(xb, lin.w, lin.b, T, N, C, K, K, K, C, c_off=C + Ba * (N + 1) * C, batch=Bp - Ba, sA=N * K, sC=(N + 1) * C, w16=lin.w16())
        _lib.call("sam6d_put_rows", _p(bg), 0, C, _p(T), (N + 1) * C, C, Bp, 1, C, _s())
        return T
    Bp, N, K = x.shape
    T = _empty((Bp, N + 1, C), x)
    if not (K == C and rows_linear(x, lin, T, Bp * N, N, N, 0, N + 1, 1)):
        gemm(x, lin.w, lin.b, T, N, C, K, K, K, C, c_off=C, batch=Bp, sA=N * K, sC=(N + 1) * C, w16=lin.w16())
    _lib.call("sam6d_put_rows", _p(bg), 0, C, _p(T), (N + 1) * C, C, Bp, 1, C, _s())
    return T


def _expand_blocks(src, gidx):
    """src (U, ...) -> (len(gidx), ...) with out[j] = src[gidx[j]] (whole leading blocks, any dtype): how per-template results are handed
    to the proposals that share the template (a device copy, no arithmetic; sam6d_take_rows)."""
    src = src.contiguous()
    M = gidx.shape[0]
    out = torch.empty((M,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    row_bytes = src.element_size()
    for d in src.shape[1:]:
        row_bytes *= d
    _lib.call("sam6d_take_rows", src.data_ptr(), gidx.data_ptr(), src.shape[0], M, row_bytes, out.data_ptr(), _s())
    return out


def coarse_point_matching(sp, sf, E, radius, model, W, rand, cfg, return_aux=False, before_pose=None):
    """sp (2B,n,3), sf (2B,n,256) stacked [scene; template]  (PEM/model/coarse_point_matching.py:32-63, eval).
    before_pose: optional callable run between the transformer and the pose solver (pem_match queues side-stream work there)."""
    B = sp.shape[0] // 2
    n = sp.shape[1]
    S = _tokens_with_bg(sf, W.coarse["in_proj"], W.coarse["bg"])
    for blk in W.coarse["blocks"]:
        S = geometric_transformer(S, E, blk)
    att = feature_similarity(S, B, n + 1, W.coarse["out_proj"], cfg["temp"])
    if before_pose is not None:
        before_pose()
    out = compute_coarse_Rt(att, sp[:B], sp[B:], model, radius, rand, cfg["nproposal1"], cfg["nproposal2"], return_aux)
    if return_aux:
        out[2]["atten"] = att
    return out


def fine_static_a(dp, df, W, cfg, templates=None):
    """First half of fine_static: token buffer D with in_proj of both clouds + the template cloud's ball queries (ordinary
    grids that share the chip well).  df: stacked (2B,N,256) or the (scene, template) pair.
    templates = (B, T, gidx, ids) (pem_match's unique-template form): dp = [B scene clouds; T UNIQUE template clouds], df = (scene
    (B,N,256), template (T,N,256)).  The scene tokens go to slots 0 .. B-1 of D (2B slots); the T template token blocks are finished in
    their own buffer Dt (in_proj here, the PE MLPs in fine_static_b), which fine_static_b then hands to the template slot of every
    proposal.  Returns (D, grp), with D = (D, Dt) in that form."""
    if templates is None:
        D = _tokens_with_bg(df, W.fine["in_proj"], W.fine["bg"])
        grp = pe_group(dp[dp.shape[0] // 2:], cfg["pe_radius1"], cfg["pe_radius2"], cfg["pe_nsample1"], cfg["pe_nsample2"])
        return D, grp
    B, T = templates[:2]
    N, K = df[0].shape[1], df[0].shape[2]
    lin = W.fine["in_proj"]
    D = _empty((2 * B, N + 1, C), df[0])
    Dt = _empty((T, N + 1, C), df[0])
    gemm(df[0], lin.w, lin.b, D, N, C, K, K, K, C, c_off=C, batch=B, sA=N * K, sC=(N + 1) * C, w16=lin.w16())
    gemm(df[1], lin.w, lin.b, Dt, N, C, K, K, K, C, c_off=C, batch=T, sA=N * K, sC=(N + 1) * C, w16=lin.w16())
    _lib.call("sam6d_put_rows", _p(W.fine["bg"]), 0, C, _p(D), (N + 1) * C, C, B, 1, C, _s())
    _lib.call("sam6d_put_rows", _p(W.fine["bg"]), 0, C, _p(Dt), (N + 1) * C, C, T, 1, C, _s())
    grp = pe_group(dp[B:], cfg["pe_radius1"], cfg["pe_radius2"], cfg["pe_nsample1"], cfg["pe_nsample2"])
    return (D, Dt), grp


def fine_static_b(dp, D, grp, W, templates=None, max_wg=0):
    """Second half: the PE MLPs of the template clouds (persistent workgroups that hold most of every CU's LDS while they run).
    templates: once per unique template, into Dt; its finished token blocks are then copied to the template slot of every proposal."""
    if templates is None:
        Bp, N, _ = dp.shape
        B = Bp // 2
        pe_apply(dp[B:], grp, W, D, B * (N + 1) * C + C, (N + 1) * C, max_wg)
        return D
    B, T, _, ids = templates
    D, Dt = D
    N = dp.shape[1]
    pe_apply(dp[B:], grp, W, Dt, C, (N + 1) * C, max_wg)
    _lib.call("sam6d_take_rows", Dt.data_ptr(), ids.data_ptr(), T, B, (N + 1) * C * 4, _p(D, B * (N + 1) * C), _s())
    return D


def fine_static(dp, df, W, cfg, templates=None):
    """The part of FinePointMatching.forward that does not depend on the coarse pose: in_proj of both clouds' dense
    features into the token buffer D (2B,N+1,256) with the bg token, and the positional encoding of the TEMPLATE cloud
    (PEM/model/fine_point_matching.py:47-51).  pem_match issues it on a side stream, under the latency-bound coarse stage.
    templates: as in fine_static_a."""
    D, grp = fine_static_a(dp, df, W, cfg, templates)
    return fine_static_b(dp, D, grp, W, templates)


def fine_point_matching(dp, df, E, fps_idx, radius, model, init_R, init_t, W, cfg, return_aux=False, D=None, fused_fine=True):
    """dp (2B,N,3) stacked [scene; template], df the dense features: (2B,N,256) stacked the same way, or the pair (scene (B,N,256),
    template (B,N,256)) left where the caller holds them  (PEM/model/fine_point_matching.py:42-79, eval).
    D: the result of fine_static() when the caller has already produced it.  fused_fine=False: the (B,N+1,N+1) attention matrix is
    materialised (launch-per-op path; aux then carries it as `atten`), otherwise aux carries the pipeline's labels / weights.  The
    launch-per-op path, which keeps a running maximum, also serves cfg["temp"] below fine_match_min_temp()."""
    Bp, N, _ = dp.shape
    B = Bp // 2
    if D is None:
        D = fine_static(dp, df, W, cfg)
    p1 = _empty((B, N, 3), dp)
    _lib.call("sam6d_rigid_inverse", _p(dp), _p(init_R), _p(init_t), B, N, _p(p1), _s())  # p1_ = (p1 - t) @ R
    positional_encoding_add(p1, W, D, C, (N + 1) * C, cfg["pe_radius1"], cfg["pe_radius2"], cfg["pe_nsample1"],
                            cfg["pe_nsample2"])
    blocks = W.fine["blocks"]
    lead = None
    for k, blk in enumerate(blocks):
        D, lead = sparse_to_dense_transformer(D, E, fps_idx, blk, lead=lead, write_bg=(k == len(blocks) - 1), return_sparse=True)
    if fused_fine and N in (2048, 4096) and _fused_block() and cfg["temp"] >= fine_match_min_temp():
        # similarity + soft assignment as one pipeline: the (B, 2049, 2049) matrix is written once and read twice (finematch.hip)
        if "out_img" not in W.fine:
            W.fine["out_img"] = pack_cross_query(W.fine["out_proj"])
        f = linear_norm_split(D.reshape(2 * B * (N + 1), C), W.fine["out_proj"], W.fine["out_img"])
        return compute_fine_Rt_fused(f, B, N + 1, cfg["temp"], dp[:B], dp[B:], model, radius, cfg["dis_thres"], return_aux)
    att = feature_similarity(D, B, N + 1, W.fine["out_proj"], cfg["temp"])
    R, t, score = compute_fine_Rt(att, dp[:B], dp[B:], model, radius, cfg["dis_thres"])
    if return_aux:
        return R, t, score, dict(atten=att)
    return R, t, score


def _ensure_w16(W):
    """Cut every Linear of the weight set into its fp16 halves now (first call only), on the caller's stream: the lazily built
    halves must exist before the pipeline forks its side stream."""
    if getattr(W, "_w16_done", False):
        return

    def walk(o):
        if isinstance(o, Linear):
            o.w16()
            o.pimg()
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
    for part in (getattr(W, "coarse", None), getattr(W, "fine", None), getattr(W, "pe", None)):
        walk(part)
    # the RPE-front weight images of every self layer too (rpe_self_layer_fused would build them on first use -- with micro-batching
    # on whichever slice's stream got there first, while another slice's stream could already launch with the cached image)
    if getattr(W, "fine", None) and "out_proj" in W.fine and "out_img" not in W.fine:
        W.fine["out_img"] = pack_cross_query(W.fine["out_proj"])
    dcT = geo_dcT(W)
    for part in (getattr(W, "coarse", None), getattr(W, "fine", None)):
        for blk in (part or {}).get("blocks", []):
            L = blk["self"]
            if "front" not in L:
                L["front"] = pack_rpe_front(L, dcT)
    W._w16_done = True


_SIDE_STREAMS = {}
# bound on the persistent PE-MLP workgroups of the side stream (they run beside the coarse pose solver)
PE_SIDE_WGS = 512


def _side_stream(dev, key=0):
    """A per-device pool of auxiliary HIP streams (key 0: the side stream of the single-slice pipeline; ("mb", i) the micro-batch
    streams)."""
    s = _SIDE_STREAMS.get((dev, key))
    if s is None:
        s = _SIDE_STREAMS[(dev, key)] = torch.cuda.Stream(device=dev)
    return s


DEFAULT_CFG = dict(coarse_npoint=196, sigma_d=0.2, sigma_a=15, angle_k=3, temp=0.1, nproposal1=6000, nproposal2=300,
                   pe_radius1=0.1, pe_radius2=0.2, pe_nsample1=32, pe_nsample2=64, dis_thres=0.15)


def resolve_routes(W, cfg, options):
    """The pipeline shape pem_match takes for this weight set, cfg and Options (a cfg key wins over the Options field of its name):
      fused_rpe        RPE attention without the embedding tensor: asked for, a split-precision mode, and the weight set's guard passed
      fused_rpe_guard  that guard (fused_rpe_in_range at cfg's sigma_a, which sets the range of the angular indices); None in mode 0
      fused_fine       the fine similarity + soft-assignment pipeline of finematch.hip (it runs on the fused block kernels, and its fixed
                       softmax shift serves cfg["temp"] >= fine_match_min_temp())
      overlap          the pose-independent fine work on a side stream
      microbatch       slices of the batch on concurrent streams"""
    split = options.mode >= 1
    guard = bool(fused_rpe_in_range(W, cfg.get("sigma_a", 15))) if split else None
    return dict(fused_rpe=bool(cfg.get("fused_rpe", options.fused_rpe)) and split and guard,
                fused_rpe_guard=guard,
                fused_fine=(bool(cfg.get("fused_fine", options.fused_fine)) and options.fused_block
                            and cfg.get("temp", DEFAULT_CFG["temp"]) >= fine_match_min_temp()),
                overlap=bool(cfg.get("overlap", options.overlap)),
                microbatch=int(cfg.get("microbatch", options.microbatch)))


@on_tensor_device
def pem_match(dense_pm, dense_fm, dense_po, dense_fo, radius, model, W, rand, cfg=DEFAULT_CFG, return_aux=False,
              shared_template=False, init_pose=None, template_ids=None):
    """Net.forward after feature extraction (PEM/model/pose_estimation_model.py:29-55):
    FPS x2 -> geo-embedding x2 -> CoarsePointMatching -> FinePointMatching -> (pred_R, pred_t, pred_pose_score).
    rand (B, 3*nproposal1) uniforms for the hypothesis sampling (the reference draws them inside, model_utils.py:292).

    cfg["microbatch"] = k (env SAM6D_MICROBATCH, default 1 = off): the batch is cut into k slices whose coarse / fine stages run
    on k HIP streams (one slice's latency-bound chains beside another's dense kernels, +2 % at k = 2, twice the host launch work).
    Each slice runs its own FPS, gathers and geometric indices on its own stream and forks no further stream.

    return_aux=True adds a dict of intermediates (coarse attention, sampled indices, hypotheses, scores, the coarse pose, FPS indices,
    fine labels / weights) WITHOUT changing which kernels run.  Kernel choice is cfg's (resolve_routes): cfg["fused_rpe"] (env
    SAM6D_FUSED_RPE, default on) = RPE attention without the embedding tensor, cfg["fused_fine"] (env SAM6D_FUSED_FINE, default on) = the
    similarity + soft-assignment pipeline of finematch.hip; off = the materialised launch-per-op forms.
    template_ids (B,) integer tensor: a MULTI-OBJECT batch (a BOP scene mixes objects per batch: PEM/provider/bop_test_dataset.py:107,156
    returns an `obj` index per instance).  dense_po (T,N,3) / dense_fo (T,N,256) then hold the T UNIQUE templates and proposal b uses
    template template_ids[b] -- the form the reference's caller would have BEFORE it `.repeat`s / indexes the template tensors per
    instance (run_inference_custom_pytorch.py:445-446).  Template-side work that does not depend on the proposal -- FPS and the row
    gathers of the sparse points / features, in_proj of the dense tokens, both ball queries, both PE MLPs, mlp3 -- runs once per
    template and its result is handed to every proposal of that template (device copies); every kernel treats a cloud independently of
    its batch neighbours, so the result is bit-identical to the repeated form (tests/test_configs_gpu.py).  The batch runs as one slice.
    shared_template=True: the case T = 1 of template_ids -- the caller guarantees dense_po[b] == dense_po[0] and dense_fo[b] ==
    dense_fo[0] for every proposal (the reference's caller repeats one object's template tensors per instance,
    run_inference_custom_pytorch.py:445-446), and the call runs on dense_po[:1] / dense_fo[:1] with every id 0.
    init_pose = (R0 (B,3,3), t0 (B,3)): the fine stage starts from this pose instead of the coarse stage's own result (which is still
    computed and returned in aux) -- the seam FinePointMatching.forward takes its init_R / init_t through
    (PEM/model/fine_point_matching.py:42-46); used by the staged parity tests."""
    B = dense_pm.shape[0]
    opts = _flags()
    routes = resolve_routes(W, cfg, opts)
    mb, fused, overlap = routes["microbatch"], routes["fused_rpe"], routes["overlap"]
    if shared_template and template_ids is not None:
        raise ValueError("pem_match: template_ids and shared_template are alternatives")
    tmpl = None  # the unique-template form: (B, T, gidx, ids)
    if shared_template or template_ids is not None:
        if shared_template:
            dense_po, dense_fo = dense_po[:1], dense_fo[:1]
            ids = torch.zeros(B, dtype=torch.int64, device=dense_pm.device)
        else:
            T = dense_po.shape[0]
            if dense_fo.shape[0] != T or template_ids.numel() != B:
                raise ValueError("pem_match: template_ids (B,) indexes dense_po / dense_fo (T, ...)")
            ids = template_ids.to(device=dense_pm.device, dtype=torch.int64).reshape(B)
            # one host read-back per call (an out-of-range id would otherwise read a zero block); not while a hipGraph is being
            # captured -- PemGraph validates the ids it is built with on the host
            if not torch.cuda.is_current_stream_capturing() and bool(((ids < 0) | (ids >= T)).any()):
                raise ValueError("pem_match: template_ids out of range [0, %d)" % T)
        # block b of a stacked (2B, ...) tensor comes from block gidx[b] of the unique (B + T, ...) one
        gidx = torch.cat([torch.arange(B, device=ids.device, dtype=torch.int64), ids + B]).contiguous()
        tmpl = (B, dense_po.shape[0], gidx, ids.contiguous())
        mb = 1

    def prepare(lo, hi, fork):
        """FPS, gathers and the geometric indices of proposals [lo, hi) on the caller's stream.  fork (the single-slice pipeline with
        overlap on): the first half of the fine stage's static part (in_proj GEMM, ball queries) is forked onto the side stream BEFORE
        these kernels and fills the chip while FPS (one workgroup per cloud, 196 sequential rounds) runs; its second half (the
        persistent PE-MLP workgroups, which would keep the LDS-heavy outlier-embedding kernels of this phase waiting) is queued by
        rest() beside the coarse pose solver.  A micro-batch slice forks no second stream: inside a slice the pipeline of slices
        provides the overlap, and a second level of forked streams is also what hipStreamEndCapture crashed on when the slices were
        captured into a graph (scratch/graph_probe2.py)."""
        b = hi - lo
        if tmpl is not None:
            dp = _cat0(dense_pm, dense_po)  # (B + T, N, 3): the unique clouds
            df = (dense_fm, dense_fo)
        else:
            dp = _cat0(dense_pm[lo:hi], dense_po[lo:hi])
            # the features (2 x 67 MB at B = 32) stay where they are: their consumers -- the FPS row gather and the fine in_proj -- read the
            # two halves with one launch each (a stacked copy cost 0.27 GB of traffic at the head of every step)
            df = (dense_fm[lo:hi], dense_fo[lo:hi])
        early = None
        if fork:
            cur = torch.cuda.current_stream()
            side = _side_stream(dp.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                D, grp = fine_static_a(dp, df, W, cfg, tmpl)
        n = cfg["coarse_npoint"]
        sp, sf, idx = sample_pts_feats(dp, df, n)
        dpu = dp
        if tmpl is not None:
            # FPS + gathers ran once per unique cloud; every proposal now gets its template's sparse points / features / indices and the
            # stacked (2B, N, 3) point tensor the rest of the pipeline addresses
            sp, sf, idx, dp = (_expand_blocks(x, tmpl[2]) for x in (sp, sf, idx, dp))
        pb = _empty((2 * b, n + 1, 3), dp)
        _lib.call("sam6d_prepend_bg_point", _p(sp), 2 * b, n, _p(pb), _s())
        if fused:
            E = geo_context(pb, W, cfg["sigma_d"], cfg["sigma_a"], cfg["angle_k"])
        else:
            E = geo_embedding(pb, W, cfg["sigma_d"], cfg["sigma_a"], cfg["angle_k"])
        if fork:
            for x in (D if isinstance(D, tuple) else (D,)):
                x.record_stream(cur)
            early = (D, side, grp)
        return dp, df, sp, sf, idx, E, early, dpu

    def rest(prep, lo, hi):
        dp, df, sp, sf, idx, E, early, dpu = prep
        rad, mod, rnd = radius[lo:hi].contiguous(), model[lo:hi].contiguous(), rand[lo:hi].contiguous()
        # The coarse stage is a chain of small launches (197-token layers, 6000 hypotheses) that leaves most of the chip
        # idle; the static part of the fine stage runs beside it when prepare forked it.  Without the fork the unique-template form
        # finishes it here and the per-proposal form inside fine_point_matching.
        D = side = hook = None
        if early is not None:
            D, side, grp = early

            def hook():
                # second half of the static fine work: the PE MLPs are matrix-pipe work, the pose solver that starts here
                # (soft assignment, sampling, 6000 SVDs, hypothesis scoring) is VALU / latency work -- they share the chip well,
                # and the RPE score kernels of the transformer above keep the matrix pipe to themselves
                cur = torch.cuda.current_stream()
                ev = torch.cuda.Event()
                ev.record(cur)
                with torch.cuda.stream(side):
                    side.wait_event(ev)
                    fine_static_b(dpu, D, grp, W, tmpl, max_wg=PE_SIDE_WGS)
        elif tmpl is not None:
            D = fine_static(dpu, df, W, cfg, tmpl)
        c = coarse_point_matching(sp, sf, E, rad, mod, W, rnd, cfg, return_aux, before_pose=hook)
        R0, t0 = c[0], c[1]
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        if isinstance(D, tuple):
            D = D[0]  # (fine_static_b has filled the template slots from the per-template buffer)
        Ri, ti = (R0, t0) if init_pose is None else (init_pose[0][lo:hi].contiguous(), init_pose[1][lo:hi].contiguous())
        f = fine_point_matching(dp, df, E, idx, rad, mod, Ri, ti, W, cfg, return_aux, D=D, fused_fine=routes["fused_fine"])
        if return_aux:
            b = hi - lo
            return f[0], f[1], f[2], dict(coarse=c[2], fine=f[3], init_R=R0, init_t=t0, fps_idx_m=idx[:b], fps_idx_o=idx[b:],
                                          geo=E)
        return f

    dense_pm, dense_fm, dense_po, dense_fo = [x.contiguous() for x in (dense_pm, dense_fm, dense_po, dense_fo)]
    if opts.mode >= 1:
        geo_packed(W), geo_cheb_packed(W), geo_dcT(W), geo_dcT16(W)  # lazily built weight images: finish them before a stream forks
        _ensure_w16(W)
    if mb <= 1 or B < 8 * mb or return_aux:
        return rest(prepare(0, B, overlap), 0, B)
    main = torch.cuda.current_stream()
    per = (B + mb - 1) // mb
    spans = [(i * per, min(B, (i + 1) * per)) for i in range(mb)]
    # (until round 4 the slices' FPS / gathers / geometric indices ran serially on the caller's stream first -- defence in depth for the
    #  packed-fp32 hazard, which the build flags have removed since; FPS is latency-bound, 0.17 ms whatever the batch, so k serial
    #  prologues cost k times that: each slice now runs its own prologue on its own stream)
    outs = []
    for i, (lo, hi) in enumerate(spans):
        st = _side_stream(dense_pm.device, ("mb", i))
        st.wait_stream(main)
        with torch.cuda.stream(st):
            outs.append(rest(prepare(lo, hi, False), lo, hi))
    R = _empty((B, 3, 3), dense_pm)
    t = _empty((B, 3), dense_pm)
    sc = _empty((B,), dense_pm)
    for i, o in enumerate(outs):
        lo = spans[i][0]
        main.wait_stream(_side_stream(dense_pm.device, ("mb", i)))
        for dst, src, w in ((R, o[0], 9), (t, o[1], 3), (sc, o[2], 1)):
            src.record_stream(main)
            _lib.call("sam6d_copy_f32", _p(src), _p(dst, lo * w), src.numel(), _s())
    return R, t, sc


def describe_paths(W, cfg=DEFAULT_CFG, options=None):
    """Which kernel routes pem_match takes for THIS weight set: several fast paths are guarded per weight set on the host (the fused RPE
    score kernel needs proj_a's Chebyshev coefficients inside the fp16 range; its two-product stage 1 needs their tail below 3e-8; the
    split-precision embedding images need proj_d / proj_a x 1024 finite in fp16) -- with the released checkpoint any of them may route
    to the slower three-product or materialised kernels.  Returned as a plain dict (bench.py prints it as `paths`)."""
    o = options if options is not None else (getattr(W, "options", None) or Options.from_env())
    routes = resolve_routes(W, cfg, o)
    split = o.mode >= 1
    img_ok = bool(geo_images_in_range(W)) if split else None
    fused = routes["fused_rpe"]
    products = None
    if fused:
        products = 3 if o.rpe_products == 3 else int(geo_cheb_a_packed(W, cfg.get("sigma_a", 15))[2])
    return {
        "matmul_mode": {0: "exact fp32 MFMA", 1: "fp16x3 split", 2: "fp16 single product (experimental)"}[o.mode],
        "rpe_attention": ("fused score kernel (Chebyshev basis, no embedding tensor), stage 1 = rpe_score_kernel<%d>" % products) if fused
                         else "materialised embedding + attention_kernel<RPE>",
        "rpe_stage1_products": products,
        "fused_rpe_guard_passed": routes["fused_rpe_guard"],
        "embedding_rows": ("geo_cheb_kernel + geo_embed_h3_kernel (split-precision images in range)" if img_ok else
                           "geo_embed_kernel (exact fp32: weight images leave the fp16 range)") if split else "geo_embed_kernel (exact fp32)",
        "gemm_route": "gemm_nt_h3_kernel, pre-split fp16 weight halves" if split else "gemm_nt_kernel (v_mfma_f32_32x32x2_f32)",
        "layer_tails": "token_block_kernel (one launch per tail)" if o.fused_block else "GEMM + LayerNorm launches",
        "cross_layers": "xattn_kernel<kv inside> + token_block kernel" if o.fused_block else "GEMM / attention_kernel launches",
        "self_attention": "sattn_kernel (q.k^T + softmax + P.v per (cloud, head))" if fused else "batched GEMMs",
        "fine_match": "finematch.hip pipeline (E written once, read twice)" if routes["fused_fine"]
                      else "materialised (B,N+1,N+1) attention + soft-assignment passes",
        "fine_out_proj": "out_split_kernel (out_proj + normalize + fp16 split)" if o.fused_out else "GEMM + fm_prep_kernel",
        "hypothesis_scoring": "score_hyp_mfma_kernel (fp32 matrix cores)",
        "ball_query": "cell grid",
        "overlap_side_stream": routes["overlap"],
        "microbatch": routes["microbatch"],
    }


class PemGraph:
    """pem_match captured ONCE into a hipGraph and replayed per step: the ~250 launches of a step (x the number of micro-batch slices)
    then cost the host one graph launch instead of one ctypes call each.  Two things follow.  Small batches (config 1's single
    proposal, a strong-scaled shard of 25) stop being bound by the host's launch rate; and the batch can be cut into `microbatch`
    independent slices whose latency-bound chains (197-token layers, FPS, the pose solver) run BESIDE each other's dense kernels on
    separate streams of the same graph without any extra host work -- eagerly, the second slice's launches were still being issued
    while the first slice ran (+2 % only).  Slices are independent proposals: results are bit-identical to the eager call.

    g = PemGraph(W, dense_pm, dense_fm, dense_po, dense_fo, radius, model, rand, microbatch=2)   # example inputs fix the shapes
    R, t, score = g(dense_pm, dense_fm, dense_po, dense_fo, radius, model, rand)                   # copies into the static inputs, replays
    R, t, score = g.replay()                                                                      # inputs already written to g.inputs

    The outputs are the graph's static tensors (overwritten by the next replay).  template_ids (fixed at capture) and shared_template
    (its case T = 1) as in pem_match; either runs the batch as one slice.  The reference has no counterpart (eager PyTorch: PEM/run_inference_custom_pytorch.py:447-454 calls the model
    once per batch)."""

    KEYS = ("dense_pm", "dense_fm", "dense_po", "dense_fo", "radius", "model", "rand")

    def __init__(self, W, dense_pm, dense_fm, dense_po, dense_fo, radius, model, rand, cfg=DEFAULT_CFG, microbatch=None,
                 shared_template=False, template_ids=None, options=None, warmup=2):
        dev = dense_pm.device
        if dev.type != "cuda":
            raise RuntimeError("PemGraph: needs HIP device tensors (this build has no CPU path)")
        self.W = W
        self.options = options if options is not None else getattr(W, "options", None)
        self.cfg = dict(cfg)
        if microbatch is not None:
            self.cfg["microbatch"] = int(microbatch)
        self.kw = dict(shared_template=shared_template)
        if template_ids is not None:
            T = dense_po.shape[0]
            ids = template_ids.detach().to("cpu", torch.int64).reshape(-1)
            if ids.numel() != dense_pm.shape[0] or bool(((ids < 0) | (ids >= T)).any()):
                raise ValueError("PemGraph: template_ids (B,) must index dense_po / dense_fo (T, ...)")
            self.kw["template_ids"] = ids.to(dev)
        if self.options is not None:
            self.kw["options"] = self.options
        with torch.cuda.device(dev):
            self.inputs = {k: v.detach().clone().contiguous() for k, v in zip(self.KEYS, (dense_pm, dense_fm, dense_po, dense_fo, radius,
                                                                                          model, rand))}
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # eager warm-up on the capture-side stream: weight images, LDS attributes, first-use setup
                for _ in range(max(1, int(warmup))):
                    self._call()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.outputs = self._call()
        self.device = dev

    def _call(self):
        i = self.inputs
        return pem_match(i["dense_pm"], i["dense_fm"], i["dense_po"], i["dense_fo"], i["radius"], i["model"], self.W, i["rand"],
                         cfg=self.cfg, **self.kw)

    def replay(self):
        self.graph.replay()
        return self.outputs

    def __call__(self, dense_pm, dense_fm, dense_po, dense_fo, radius, model, rand):
        for k, v in zip(self.KEYS, (dense_pm, dense_fm, dense_po, dense_fo, radius, model, rand)):
            dst = self.inputs[k]
            if v.shape != dst.shape:
                raise ValueError("PemGraph: %s has shape %s, the graph was captured for %s" % (k, tuple(v.shape), tuple(dst.shape)))
            if v.data_ptr() != dst.data_ptr():
                dst.copy_(v, non_blocking=True)
        return self.replay()


def template_is_shared(dense_po, dense_fo):
    """True when every proposal carries the same template cloud (bitwise), i.e. the caller `.repeat`ed one object's tensors
    (PEM/run_inference_custom_pytorch.py:445-446).  One host read-back."""
    B = dense_po.shape[0]
    if B < 2:
        return False
    flags = torch.empty(2, dtype=torch.int32, device=dense_po.device)
    _lib.call("sam6d_batch_rows_equal", _p(dense_po.contiguous()), B, dense_po[0].numel(), flags.data_ptr(), _s())
    _lib.call("sam6d_batch_rows_equal", _p(dense_fo.contiguous()), B, dense_fo[0].numel(), flags.data_ptr() + 4, _s())
    f = flags.cpu()
    return bool(f[0]) and bool(f[1])


def _cat0(a, b):
    """stack two (B,N,K) tensors along the batch -- a device copy, no arithmetic"""
    a = a.contiguous()
    b = b.contiguous()
    out = _empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a)
    n = a.numel()
    _lib.call("sam6d_copy_f32", _p(a), _p(out), n, _s())
    _lib.call("sam6d_copy_f32", _p(b), _p(out, n), b.numel(), _s())
    return out
