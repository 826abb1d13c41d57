"""Float64 restatements of the launch-per-op layer under the fused kernels -- sam6d_attention (csrc/attention.hip), sam6d_scaled_softmax,
sam6d_sinusoid_embed, the three kernels of csrc/linattn.hip, sam6d_transpose, the row kernels sam6d_layernorm256 / sam6d_l2norm256 and
the small helpers at the end of csrc/pe.hip -- and of the unfused routes pem.mha_forward / cross_layer / rpe_self_layer /
linear_attention_forward composed of them; the seeded builders and case lists of tests/test_attn_shapes_gpu.py /
tests/test_attn_shapes_host.py; an fp32 CPU evaluation of the same formulas (the `*32` functions: plain torch float32, the "oracle"
side); and the table of bounds.  Plain numpy / torch on the CPU, nothing of the product is imported.

Where TOL's numbers come from:
  project   attn / softmax 3e-6 x max(1, max |want|) (tests/test_block_gpu.py::test_rpe_self_attention_vs_fp64, the same operation on the
            matrix cores), layernorm 2e-5 (tests/test_pem_gpu.py::test_layernorm), mha_hidden 2e-5 / mha_probs 2e-6 / layer 5e-5
            (tests/test_submodules_gpu.py), the cap 2e-5 of the three LinearAttention entries (test_submodules_gpu.py)
  stated    rowsum_ulp 4 and sinusoid_ulp 1: the requirements these tests were written to
  derived   kv_bounds (sequential fp32 accumulation, gamma_k), rigid_bound (five roundings), l2norm (three roundings + the sum)
  measured  focus_k / focus_q / linattn: 8 x the worst error of the fp32 CPU evaluation against float64 over the case lists (the factor
            covers the wave-butterfly norm against a sequential sum), each relative to max |want| of its case
Measured maxima when written (fp32 CPU evaluation against float64, tests/test_attn_shapes_host.py prints them again):
  attention 7.5e-7 relative at unit scale (a quarter of the bound), 1.3e-7 with equal keys, below 1e-15 on the dominant-key and
  large-logit inputs (every other probability underflows); softmax 2.2e-7, row sums 2.3 ulp; sinusoid 1 ulp (torch's fp32 sin / cos);
  kvT 0.99 of its bound (J = 1: the one rounding the bound allows), ksum 0.11; rigid inverse 0.38 of its bound; layernorm 4.3e-7
  (3.6e-7 on 1e4 + N(0,1)); l2norm 1.3e-8; mha hidden 1.6e-6, probabilities 3.8e-7; whole layers 1.2e-6.
Measured maxima of the kernels on an MI355X over all cases of tests/test_attn_shapes_gpu.py, against the same float64:
  attention plain 0.15 of its bound (4.5e-7 relative), RPE 0.08; equal keys 0.03; dominant and large-logit inputs below 1e-9 of it;
  softmax 1.8e-7, row sums 1.75 ulp; sinusoid 0 ulp (every entry bit-equal); focus_k 1.7e-7, focus_q 1.4e-7 of max |want|; kvT 0.99 of
  its bound (J = 1), ksum 0.23; linear_attention_forward 1.0e-6 (mode 0) / 8.9e-7 (mode 1) of max |want|; layernorm256 3.8e-7 (3.0e-7 on
  1e4 + N(0,1)); l2norm256 1.4e-8; rigid inverse 0.38 of its bound; mha_forward hidden 1.5e-6, probabilities 3.8e-7; cross_layer
  1.6e-6, rpe_self_layer 1.4e-6.
Two of these figures were reached by changing the product, not the bound: layernorm256 summed the row as it stood and was off by 1.9e-3
on the 1e4 + N(0,1) row (it now takes the row's first element off first), and in matmul mode 1 the last contraction of the unfused
linear attention lost 1.35e-5 at (2, 300, 197) to fp16 subnormals of the split (pem._linattn_contract now runs it on the exact loop)."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

H, C, D = 4, 256, 64
ULP1 = 2.0 ** -23   # one fp32 ulp of 1.0
U = 2.0 ** -24      # the fp32 unit roundoff

TOL = dict(
    attn=3e-6,          # project: x max(1, max |want|)
    softmax=3e-6,       # the same bound for the stand-alone softmax (probabilities: max |want| <= 1)
    rowsum_ulp=4,       # stated: |sum_m p - 1| <= 4 ulp of 1.0
    sinusoid_ulp=1,     # stated: against float64 sin / cos of the fp32 product, rounded once
    focus_k=1.6e-6,     # 8 x 2.0e-7   (measured fp32: 2.02e-7 of max |want|)
    focus_q=1.4e-6,     # 8 x 1.8e-7   (measured fp32: 1.78e-7)
    linattn=8.2e-6,     # 8 x 1.02e-6  (measured fp32: 1.02e-6); all three <= the project's 2e-5 for LinearAttention
    layernorm=2e-5,     # project: max abs
    l2norm=2e-6,        # derived in l2norm_bound's docstring; x max |want| (<= 1 for a normalised row)
    mha_hidden=2e-5, mha_probs=2e-6, layer=5e-5,  # project: tests/test_submodules_gpu.py
)
LINATTN_CAP = 2e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_bound(want, tol):
    """tol x max(1, max |want|)"""
    return tol * max(1.0, float(torch.as_tensor(want).abs().max()))


def gamma(k):
    """gamma_k = k u / (1 - k u): the relative bound of k sequential fp32 roundings"""
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------- 1. attention
PLAIN_SHAPES = [(1, 1, 1), (2, 5, 3), (3, 4, 17), (2, 7, 64), (2, 6, 65), (1, 9, 255), (1, 3, 256), (2, 197, 197), (1, 257, 197)]
RPE_SHAPES = PLAIN_SHAPES[:7] + [(2, 50, 50)]
INDEPENDENCE_SHAPES = [(3, 5, 17), (3, 4, 65)]
ATTN_KINDS = ("random", "dominant", "equal", "large")
DOMINANT_SCALE = 70.0   # the leading key's logit; every other key's is scale x the cosine between two keys of a head
LARGE_SCALE = 400.0     # logits of a few hundred: exp overflows fp32 above 88.7 without the max subtraction
# (layout, shape) pairs of tests/test_attn_shapes_gpu.py; "sep" = four contiguous buffers, run at every shape
LAYOUT_SHAPES = dict(qkv768={False: [(1, 1, 1), (2, 197, 197)], True: [(1, 1, 1), (2, 50, 50)]},
                     kv512={False: [(3, 4, 17), (2, 6, 65)], True: [(3, 4, 17), (2, 6, 65)]},
                     wide={False: [(2, 5, 3), (1, 9, 255)], True: [(2, 5, 3), (1, 9, 255)]})


def lead_key(B, n, m):
    """(B,n) int64: the key that leads query (b, i) of the dominant / large kinds"""
    b, i = torch.meshgrid(torch.arange(B), torch.arange(n), indexing="ij")
    return (7 * i + 3 * b + 1) % m


@functools.lru_cache(maxsize=None)
def attn_inputs(kind, B, n, m, rpe, scale=None, seed=0):
    """q (B,n,256), k / v (B,m,256) [, qp (B,n,4,256), E (B,n,m,256)] fp32, seeded.
    random:   unit scale: q, k, v, qp ~ N(0,1), E ~ N(0, 1/4): both score terms / 8 have unit variance
    dominant: every head of every key scaled to norm 8, q_h = (scale / 8) k_h[lead]: the lead's logit is `scale`, another key's is
              scale x cos(k_h[lead], k_h[m]) (+ the unit-scale RPE term); scale defaults to DOMINANT_SCALE
    large:    the same with LARGE_SCALE
    equal:    all keys of a cloud bitwise equal (and all E rows of a query): every probability is 1 / m"""
    g = gen(100 + 1000 * ATTN_KINDS.index(kind) + 31 * B + 7 * n + m + (500 if rpe else 0) + seed)
    q, k, v = torch.randn(B, n, C, generator=g), torch.randn(B, m, C, generator=g), torch.randn(B, m, C, generator=g)
    qp = E = None
    if rpe:
        qp, E = torch.randn(B, n, H, C, generator=g), 0.5 * torch.randn(B, n, m, C, generator=g)
    if kind in ("dominant", "large"):
        s = float(scale if scale is not None else (DOMINANT_SCALE if kind == "dominant" else LARGE_SCALE))
        kh = k.view(B, m, H, D)
        k = (kh / kh.norm(dim=3, keepdim=True) * 8.0).reshape(B, m, C)
        q = torch.gather(k, 1, lead_key(B, n, m)[:, :, None].expand(B, n, C)) * (s / 8.0)
    elif kind == "equal":
        k = k[:, :1].expand(B, m, C)
        if rpe:
            E = E[:, :, :1].expand(B, n, m, C)
    f = lambda t: None if t is None else t.contiguous()
    return types.SimpleNamespace(q=f(q), k=f(k), v=f(v), qp=f(qp), E=f(E))


def _attention(q, k, v, qp, E, dt):
    B, n, _ = q.shape
    m = k.shape[1]
    qh, kh, vh = q.to(dt).view(B, n, H, D), k.to(dt).view(B, m, H, D), v.to(dt).view(B, m, H, D)
    s = torch.einsum("bnhc,bmhc->bhnm", qh, kh)
    if E is not None:
        s = s + torch.einsum("bnhc,bnmc->bhnm", qp.to(dt).view(B, n, H, C), E.to(dt))
    s = s / 8.0
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhnm,bmhc->bnhc", p, vh).reshape(B, n, C), p, s


def attention64(q, k, v, qp=None, E=None):
    """s[h,n,m] = (q_h[n].k_h[m] (+ qp[n,h,:].E[n,m,:])) / 8, out = softmax_m(s) v -> (out (B,n,256), p (B,4,n,m), s) in float64"""
    return _attention(q, k, v, qp, E, torch.float64)


def attention32(q, k, v, qp=None, E=None):
    return _attention(q, k, v, qp, E, torch.float32)


def logit_lead(s, lead):
    """min over (b, h, n) of s[lead] - max_{m != lead} s[m]; inf for a single key"""
    B, _, n, m = s.shape
    if m == 1:
        return math.inf
    idx = lead[:, None, :, None].expand(B, H, n, 1)
    top = torch.gather(s, 3, idx)
    rest = s.scatter(3, idx, -math.inf).amax(3, keepdim=True)
    return float((top - rest).min())


# ------------------------------------------------------------------------------------------------------- 2. softmax, sinusoid
SOFTMAX_ROWS = (1, 3, 4, 5, 1001)
SOFTMAX_N = (1, 63, 64, 65, 197, 300)
SOFTMAX_SCALES = (0.125, 1.0)
SINUSOID_CASES = [(1, 2), (2, 6), (129, 256), (1000, 256)]


@functools.lru_cache(maxsize=None)
def softmax_inputs(rows, n):
    g = gen(2000 + 13 * rows + n)
    return (2.0 * torch.randn(rows, n, generator=g)).contiguous(), torch.randn(rows, n, generator=g).contiguous()


def _softmax(a, b, scale, dt):
    s = a.to(dt) if b is None else a.to(dt) + b.to(dt)
    return torch.softmax(s * scale, dim=-1)


def softmax64(a, b, scale):
    return _softmax(a, b, scale, torch.float64)


def softmax32(a, b, scale):
    return _softmax(a, b, scale, torch.float32)


def div_term(d_model):
    """SinusoidalPositionalEmbedding's buffer (PEM/model/transformer.py:264-266), the same torch operations"""
    return torch.exp(torch.arange(0, d_model, 2).float() * (-np.log(10000.0) / d_model))


@functools.lru_cache(maxsize=None)
def sinusoid_x(n):
    """(n,) fp32 arguments: zero, -0.0, negative ones, 866.0254 (the bg point's distance index), +-1e4, the rest spread over
    [0, 24), [-24, 0), [0, 1e3) and [0, 1e4)"""
    g = gen(3000 + n)
    r = torch.rand(n, generator=g)
    k = torch.arange(n) % 4
    x = torch.where(k == 0, r * 24.0, torch.where(k == 1, -r * 24.0, torch.where(k == 2, r * 1e3, r * 1e4)))
    special = torch.tensor([866.0254, 0.0, -0.0, 1e4, -1e4, -57.3, 23.9, 9999.5])
    if n == 2:
        special = torch.tensor([0.0, -3.7])
    x[:min(n, special.numel())] = special[:n]
    return x.contiguous()


def sinusoid_ref(x, div):
    """(n, 2 half) fp32: float64 sin / cos of the fp32 product x[i] div[j], interleaved, rounded once -- what the kernel is written to do"""
    w = (x.float()[:, None] * div.float()[None, :]).numpy().astype(np.float64)
    return torch.from_numpy(np.stack([np.sin(w), np.cos(w)], -1).reshape(x.numel(), -1).astype(np.float32))


def sinusoid32(x, div):
    w = x.float()[:, None] * div.float()[None, :]
    return torch.stack([torch.sin(w), torch.cos(w)], -1).reshape(x.numel(), -1)


def ulp_distance(got, want32):
    """max over the entries of |got - want| / ulp(want) (the spacing of fp32 at |want|), and the count of entries not bit-equal"""
    g, w = np.asarray(got, np.float32), np.asarray(want32, np.float32)
    d = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
    return float(d.max()), int((g.view(np.int32) != w.view(np.int32)).sum())


# ------------------------------------------------------------------------------------------------------- 3. linear attention
FOCUS_K_ROWS = (1, 3, 4, 5, 394)
FOCUS_LD = (256, 260, 512)
KV_J = (1, 31, 32, 33, 196, 197)
KV_B = (1, 3)
FOCUS_Q_CASES = [(1, 1), (3, 5), (2, 2049), (1, 16389)]
FOCUS_Q_LD = (256, 260)
LINATTN_CASES = [(2, 300, 197), (1, 130, 43)]  # (B, I, J) with I J 128 > 64 64 (I + J): the kv contraction order
SOFTPLUS_MAX = 1.4  # stated condition of the all-non-positive rows: (1e-6 / softplus)^6 stays a normal fp32 number


def focus_scale(uniform=None):
    """(256,) fp32 focusing scale: U(-1, 1) (softplus in [0.31, 1.32]), or one value for every channel"""
    if uniform is not None:
        return torch.full((C,), float(uniform))
    return (torch.rand(C, generator=gen(3100)) * 2.0 - 1.0).contiguous()


@functools.lru_cache(maxsize=None)
def focus_rows(rows, seed=0):
    """(rows,256) fp32: row r is random (r % 3 = 0), has a single positive channel (r % 3 = 1) or none (r % 3 = 2)"""
    g = gen(3200 + rows + seed)
    x = torch.randn(rows, C, generator=g)
    r = torch.arange(rows)
    neg = -x.abs()
    one = neg.clone()
    ch = (37 * r + 5) % C
    one[r, ch] = x.abs()[r, ch] + 0.1
    x = torch.where((r % 3 == 1)[:, None], one, torch.where((r % 3 == 2)[:, None], neg, x))
    if rows >= 3:
        x[2, ::2] = 0.0  # zeros and -0.0 among the non-positive channels
        x[2, 1::4] = -0.0
    return x.contiguous()


def _phi(x, scale, dt):
    sp = F.softplus(scale.to(dt))
    x1 = (torch.relu(x.to(dt)) + 1e-6) / sp
    x3 = x1 ** 3
    return x3 / x3.norm(dim=-1, keepdim=True) * x1.norm(dim=-1, keepdim=True)


def phi64(x, scale):
    """phi(x) = x3 / |x3| |x1|, x1 = (relu(x) + 1e-6) / softplus(scale), x3 = x1^3 (PEM/model/transformer.py:553-563)"""
    return _phi(x, scale, torch.float64)


def phi32(x, scale):
    return _phi(x, scale, torch.float32)


def _focus_q(q, scale, ksum, dt):
    """q (B,I,256), ksum (B,256) = [head][64] -> phi(q) scaled per head by z = 1 / (phi(q)_h . ksum_h + 1e-6)"""
    B, I, _ = q.shape
    p = _phi(q, scale, dt).view(B, I, H, D)
    z = 1.0 / (torch.einsum("bihc,bhc->bih", p, ksum.to(dt).view(B, H, D)) + 1e-6)
    return (p * z[..., None]).reshape(B, I, C)


def focus_q64(q, scale, ksum):
    return _focus_q(q, scale, ksum, torch.float64)


def focus_q32(q, scale, ksum):
    return _focus_q(q, scale, ksum, torch.float32)


@functools.lru_cache(maxsize=None)
def kv_inputs(B, J):
    """k >= 0 as phi leaves it (|N(0,1)|, a tenth of the entries 1e-6), v ~ N(0,1): (B,J,256) each"""
    g = gen(3300 + 17 * B + J)
    k = torch.randn(B, J, C, generator=g).abs()
    k[torch.rand(B, J, C, generator=g) < 0.1] = 1e-6
    return k.contiguous(), torch.randn(B, J, C, generator=g).contiguous()


def _kv(k, v, dt):
    B, J, _ = k.shape
    kh, vh = k.to(dt).view(B, J, H, D), v.to(dt).view(B, J, H, D)
    return torch.einsum("bjhc,bjhd->bhdc", kh, vh), kh.sum(1)


def kv64(k, v):
    """kvT[b,h,d,c] = sum_j k[b,j,64h+c] v[b,j,64h+d] (B,4,64,64), ksum[b,h,c] = sum_j k[b,j,64h+c] (B,4,64)"""
    return _kv(k, v, torch.float64)


def kv32(k, v):
    return _kv(k, v, torch.float32)


def kv_bounds(k, v):
    """Element-wise bounds of |kvT - kvT64| and |ksum - ksum64| for a sequential fp32 accumulation over the J keys: each of the J fused
    multiply-adds rounds once -> gamma_J sum_j |k v|; the J - 1 additions of ksum (the first term enters exactly) -> gamma_{J-1} sum_j |k|.
    Any other summation order of the same terms rounds no more often per term."""
    J = k.shape[1]
    a, s = kv64(k.abs(), v.abs())
    return gamma(J) * a, gamma(J - 1) * s


def _linattn(xq, xk, xv, W, scale, dt):
    B, I, _ = xq.shape
    lin = lambda x, wb: x.to(dt) @ wb[0].to(dt).t() + wb[1].to(dt)
    q, k, v = lin(xq, W["q"]), lin(xk, W["k"]), lin(xv, W["v"])
    kvT, ksum = _kv(_phi(k, scale, dt), v, dt)
    qz = _focus_q(q, scale, ksum.reshape(B, C), dt).view(B, I, H, D)
    return torch.einsum("bihc,bhdc->bihd", qz, kvT).reshape(B, I, C)


def linattn64(xq, xk, xv, W, scale):
    """LinearAttention.forward (PEM/model/transformer.py:548-578), the kv contraction order; W = dict(q=(w, b), k=, v=)"""
    return _linattn(xq, xk, xv, W, scale, torch.float64)


def linattn32(xq, xk, xv, W, scale):
    return _linattn(xq, xk, xv, W, scale, torch.float32)


# ------------------------------------------------------------------------------------------------------- 4. bit-exact helpers
TRANSPOSE_SHAPES = [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 33, 31)]


def prepend_bg(pts):
    """(B,n,3) -> (B,n+1,3) numpy: the bg point (100,100,100) in front of every cloud"""
    p = np.asarray(pts, np.float32)
    return np.concatenate([np.full((p.shape[0], 1, 3), 100.0, np.float32), p], 1)


def rows_equal(x):
    """1 when every x[b] equals x[0] bit for bit (so +0.0 != -0.0, and a NaN equals the same NaN), else 0"""
    b = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)
    return int((b == b[:1]).all())


# ------------------------------------------------------------------------------------------------------- 5. row kernels
ROW_COUNTS = (1, 3, 4, 5)
RIGID_CASES = [(1, 1), (3, 257), (2, 2048)]


def layernorm64(x, g, b, eps=1e-5):
    """nn.LayerNorm over the last axis (biased variance)"""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def layernorm32(x, g, b, eps=1e-5):
    """The same two passes in fp32, on the row minus its first element (LayerNorm is invariant under the shift, and the differences of
    nearby fp32 values are exact): the form csrc/gemm.hip's layernorm256_kernel has.  On a row of 1e4 + N(0,1) F.layer_norm in fp32 is
    off by 1.8e-3 and the two passes without the shift by 1.9e-3 -- the mean of 256 values near 1e4 carries the rounding of sums of 1e6
    -- against 6e-7 with it (measured when written; the host test holds the shifted form to TOL.layernorm)."""
    x = x.float()
    return _ln(x - x[..., :1], (g.float(), b.float()), eps)


def l2norm64(x):
    """F.normalize(x, p=2, dim=-1): x / max(|x|, 1e-12)"""
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def l2norm32(x):
    return F.normalize(x.float(), p=2, dim=-1)


def l2norm_bound(want):
    """Relative to max |want|: the squared norm of 256 fp32 terms in any order is off by at most gamma_{256+1} relative (all terms
    positive), its root halves that and rounds once, the division rounds once: (257 / 2 + 2) 2^-24 = 7.8e-6 worst case; the tree sum
    of the kernel rounds 2 + 8 times per term -> (10 / 2 + 2) 2^-24 = 4.2e-7.  TOL.l2norm = 2e-6 lies between the two."""
    return TOL["l2norm"] * float(torch.as_tensor(want).abs().max())


@functools.lru_cache(maxsize=None)
def rigid_inputs(B, N):
    """x (B,N,3) around t (B,3) (a cloud in camera coordinates: offsets up to 2, translations up to 1000), R (B,3,3) random rotations"""
    g = gen(5000 + 3 * B + N)
    Rm = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))[0].float().contiguous()
    t = ((torch.rand(B, 3, generator=g) - 0.5) * 2000.0).contiguous()
    x = (t[:, None, :] + (torch.rand(B, N, 3, generator=g) - 0.5) * 4.0).contiguous()
    return x, Rm, t


def rigid_inverse64(x, Rm, t):
    """y[b,i,:] = (x[b,i,:] - t[b]) @ R[b] in float64"""
    return (x.double() - t.double()[:, None, :]) @ Rm.double()


def rigid_inverse32(x, Rm, t):
    return (x - t[:, None, :]) @ Rm


def rigid_bound(x, Rm, t):
    """|y_j - y64_j| <= 5 x 2^-24 sum_k |d_k| |R_kj| with d = x - t in float64.  Derivation, u = 2^-24: the kernel forms d_k = fl(x_k -
    t_k) = (x_k - t_k)(1 + e1), |e1| <= u, then y_j = fma(d_2, R_2j, fma(d_1, R_1j, fl(d_0 R_0j))): the product rounds once, each of the
    two fused multiply-adds once.  The term k = 0 so carries (1 + u)^4 - 1, k = 1 (1 + u)^3 - 1 and k = 2 (1 + u)^2 - 1, every one at
    most 4 u + O(u^2) <= 5 u of |d_k R_kj|.  A matmul that does not fuse (the fp32 CPU evaluation) rounds three products and two sums:
    the same count."""
    d = (x.double() - t.double()[:, None, :]).abs()
    return 5.0 * U * (d @ Rm.double().abs())


# ------------------------------------------------------------------------------------------------------- 6. composed routes
MHA_CASES = [(2, 50, 37), (1, 5, 1)]
MHA_RPE_CASE = (2, 6, 9)
CROSS_M = (209, 256)
RPE_LAYER_CASES = [(2, 50), (1, 5)]


def _wb(sd, p):
    return sd[p + ".weight"].detach().float().cpu(), sd[p + ".bias"].detach().float().cpu()


def attention_weights(sd, p, rpe):
    """proj_q / proj_k / proj_v (/ proj_p) of the MultiHeadAttention at reference-keyed prefix p (".attention.attention" included)"""
    W = dict(q=_wb(sd, p + ".proj_q"), k=_wb(sd, p + ".proj_k"), v=_wb(sd, p + ".proj_v"))
    if rpe:
        W["p"] = _wb(sd, p + ".proj_p")
    return W


def layer_weights(sd, p, rpe):
    """a whole TransformerLayer / RPETransformerLayer / LinearTransformerLayer at prefix p: the attention's projections and the tail"""
    W = attention_weights(sd, p + ".attention.attention", rpe)
    W.update(lin=_wb(sd, p + ".attention.linear"), n1=_wb(sd, p + ".attention.norm"), exp=_wb(sd, p + ".output.expand"),
             sq=_wb(sd, p + ".output.squeeze"), n2=_wb(sd, p + ".output.norm"))
    return W


def _lin(x, wb):
    return x @ wb[0].to(x.dtype).t() + wb[1].to(x.dtype)


def _ln(x, gb, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gb[0].to(x.dtype) + gb[1].to(x.dtype)


def _mha(xq, xk, xv, W, E, dt):
    """MultiHeadAttention.forward / RPEMultiHeadAttention.forward -> (hidden (B,N,256), probabilities (B,4,N,M)).  The bias of proj_p
    adds q_h . b_p,h to every key of a row and cancels in the softmax; it is kept here as the reference model has it."""
    q, k, v = _lin(xq.to(dt), W["q"]), _lin(xk.to(dt), W["k"]), _lin(xv.to(dt), W["v"])
    qp = None
    B, N, _ = q.shape
    if E is not None:
        Wp = W["p"][0].to(dt).view(H, D, C)  # proj_p(E)_h = Wp[64h:64h+64] E + b_p: q_h . proj_p(E)_h = (Wp_h^T q_h) . E + q_h . b_p,h
        qp = torch.einsum("bnhd,hdc->bnhc", q.view(B, N, H, D), Wp)
    out, p, s = _attention(q, k, v, qp, E, dt)
    return out, p


def mha64(xq, xk, xv, W, E=None):
    return _mha(xq, xk, xv, W, E, torch.float64)


def mha32(xq, xk, xv, W, E=None):
    return _mha(xq, xk, xv, W, E, torch.float32)


def _attn_layer(hidden, x, W):
    """AttentionLayer's tail: LayerNorm(linear(hidden) + x) (PEM/model/transformer.py:152-181)"""
    return _ln(_lin(hidden, W["lin"]) + x, W["n1"])


def _output(y, W):
    """AttentionOutput: LayerNorm(y + squeeze(relu(expand(y)))) (PEM/model/transformer.py:184-199)"""
    return _ln(y + _lin(torch.relu(_lin(y, W["exp"])), W["sq"]), W["n2"])


def attention_layer64(x, mem, W, E=None):
    """AttentionLayer / RPEAttentionLayer output_states"""
    return _attn_layer(mha64(x, mem, mem, W, E)[0], x.double(), W)


def output64(x, W):
    return _output(x.double(), W)


def layer64(x, mem, W, E=None):
    """TransformerLayer (cross: E None) / RPETransformerLayer (mem = x) output_states in float64"""
    return _output(attention_layer64(x, mem, W, E), W)


def layer32(x, mem, W, E=None):
    x = x.float()
    return _output(_attn_layer(mha32(x, mem, mem, W, E)[0], x, W), W)


def linattn_layer64(x, mem, W, scale, upto="layer"):
    """LinearAttention ("attn"), LinearAttentionLayer ("attn_layer") or LinearTransformerLayer ("layer") output in float64"""
    hid = linattn64(x, mem, mem, W, scale)
    if upto == "attn":
        return hid
    y = _attn_layer(hid, x.double(), W)
    return y if upto == "attn_layer" else _output(y, W)


def layer_inputs(seed, B=1, n=197):
    """the generator of oracle/gen_golden.py: x, y (B,n,256), e0, e1 (B,n,n,256)"""
    g = gen(seed)
    x = torch.randn(B, n, C, generator=g)
    y = torch.randn(B, n, C, generator=g)
    e0 = 0.5 * torch.randn(B, n, n, C, generator=g)
    e1 = 0.5 * torch.randn(B, n, n, C, generator=g)
    return x, y, e0, e1


@functools.lru_cache(maxsize=None)
def tokens(B, n, seed):
    return torch.randn(B, n, C, generator=gen(6000 + 100 * seed + 7 * B + n)).contiguous()


@functools.lru_cache(maxsize=None)
def embedding(B, n, m, seed):
    return (0.5 * torch.randn(B, n, m, C, generator=gen(6500 + 100 * seed + 7 * B + n + m))).contiguous()
