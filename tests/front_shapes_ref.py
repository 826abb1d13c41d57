"""Float64 restatements of the fused "front" kernels of csrc/block.hip -- rpe_front_kernel (sam6d_rpe_front, sam6d_rpe_front_vt:
qkv projection, proj_p fold and D_c fold of every RPE self layer) and the dense linear-attention layer (sam6d_linattn_kv_image +
sam6d_linattn_layer) -- with the seeded builders and case lists of tests/test_front_shapes_gpu.py / tests/test_front_shapes_host.py,
the per-element bound of the chained split products, and a CPU emulation of the kernel's arithmetic.  Plain numpy / torch on the CPU,
nothing of the product is imported.

The bounds and where each number comes from
  arithmetic  tests/test_gemm_routes_gpu.py "mode 1": both operands multiplied by a power of two, cut into fp16 hi + lo, the products
              lo.hi + hi.lo + hi.hi accumulated in fp32.  With x' = x s: x' = hi + lo + d, |d| <= 2^-22 |x'| + 2^-25 (lo is rounded to
              fp16, whose subnormal spacing is 2^-24), so one product is off by <= 3 * 2^-22 |a||w| + 2^-25 (|a| / s_w + |w| / s_a) in
              true units, and the 3 * K32 fp16 products (exact in fp32) are summed with at most one rounding each.
  tau(K)      TIGHTEN[K] * (3 * 2^-22 + 3 * K32 * u), u = 2^-24, K32 = K rounded up to 32       (derived, that docstring)
  TIGHTEN     K = 64: 1/8, the GEMM test's figure for this arithmetic (it observed 0.14 of the tightened bound on an MI355X; the
              proj_p fold sits at 0.12 here).  K = 256: 1/16 -- at 1/8 the first MI355X run gave 0.031 (qkv, product-dominated kinds)
              and 0.032 (D_c fold, flat rows), far below 0.14: the 768 roundings of the derived sum behave like a random walk.
              Tightened once by 2, which keeps 4 x headroom at every case (table below); only ever tightened.
  abs         2^-25 * (sum_k |a_k| / s_w + sum_k |w_k| / s_a): the subnormal floor of the lo halves, NOT tightened   (derived)
  scales      s_a per token = pow2_scale(max |row|) (csrc/common.h: the power of two that puts the maximum into [2^13, 2^14), 1 for a
              zero row), s_w per matrix = runtime._pow2_scale(max |W|), the same rule.  The folds take their row scale from the q / qp
              the kernel itself computed, which may sit on the other side of a power of two: the abs term takes half the scale there.
  chain       e_q  = tau(256) |x| . |Wqkv|^T + abs + 4u (|acc| + |b|)                            (the last term: the bias add)
              e_qp = e_q_h . |Wp_h| + tau(64) (|q_h| + e_q_h) . |Wp_h| + abs
              e_qd = e_qp . |D_c| + tau(256) (|qp_h| + e_qp) . |D_c| + abs
              k, v and the values read back from vT: e_q of their columns.
  folds alone The chain adds worst cases through two |.| products, which leaves it ~100 x (qp) and ~1000 x (qd) above what the
              arithmetic does: an emulation that drops every activation lo half reaches only 3.9 (qp) and 0.27 (qd) of it.  So each
              fold is ALSO checked on its own, against float64 of the q / qp the kernel returned (its very operands):
              tau(64) |q_h| . |Wp_h| + abs and tau(256) |qp_h| . |D_c| + abs (fold_stages).  Tighter than the chain, never instead of it.
  dense      5e-5 absolute on the LayerNorm output: the project's bound, tests/test_block_gpu.py::test_linattn_layer_vs_oracle_math
Conditions on the inputs: every operand finite and its scaled maximum inside pow2_scale's exponent clamp (2^-86 < max |.| < 2^114); the
case lists stay eleven decades inside that.

Worst |err| / bound over all cases of the lists, per output (tests/test_front_shapes_host.py prints the first column again, the GPU
test the second):
                   CPU emulation   MI355X
  qkv              0.243           0.243   (the bias add's half ulp against its 4u where the bias dominates: x 1e-5, Wqkv 1e-4, the
                                            large bias; 0.06 where the product dominates)
  qp, chained      0.097           0.100
  qd, chained      0.0060          0.0099
  qp, fold alone   0.125           0.119
  qd, fold alone   0.107           0.107   (the decaying D_c rows, where the abs term leads; 0.06 on flat rows)
  vT               (= v of qkv)    0.055
  dense layer      --              3.4e-6 max |err| against 5e-5 (J = 33, memory x 1e3)
The emulation with the activation lo halves dropped, worst ratio per case: qkv 14.5 - 91, fold alone qp 78 - 118, qd 17 - 33 (each must
exceed 1, and does at every case); against the chained bounds alone qp 3.9 - 87 and qd 0.27 - 9.1 -- the chain would not see it."""
import functools
import math
import types

import torch
import torch.nn.functional as F

H, C, D = 4, 256, 64
U = 2.0 ** -24
TIGHTEN = {64: 1.0 / 8, 256: 1.0 / 16}   # scale of the derived tau per K (module docstring; only ever tightened)
DENSE_TOL = 5e-5
EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------- case lists
FRONT_M = [1, 15, 16, 17, 63, 64, 65, 127, 129, 1000]          # edges of the 16-row wave and the 64-row workgroup
FRONT_KINDS = ["unit", "mixed", "x1e4", "x1e-5", "wqkv300", "wqkv1e-4", "wp1e3", "dc1e-5", "dcdecay", "bigbias"]
FRONT_KIND_M = [129, 300]
FRONT_CASES = [("unit", M) for M in FRONT_M] + [(k, M) for k in FRONT_KINDS for M in FRONT_KIND_M]
INDEPENDENCE_ROWS = [0, 15, 16, 63, 64]                        # and M - 1
INDEPENDENCE_M = 129
# (Bp, n, ldp - 4 ceil(n / 4)): n > 208 is the range pem._rpe_self_front serves with this entry
VT_CASES = [(1, 1, 0), (3, 5, 0), (2, 50, 0), (2, 50, 8), (5, 64, 0), (2, 209, 0), (1, 260, 0), (3, 211, 0)]
VT_BITWISE = [(2, 209), (1, 260)]
KV_J = [1, 15, 16, 17, 31, 32, 33, 48, 196, 197]               # the 16-key step and the two-step register ring (32 keys per trip)
KV_B = [1, 3]
KV_LD = [512, 516, 768]
KV_GAP = [0, 2]                                                # cloud stride (J + gap) * ld
DENSE_J = [1, 17, 33, 196]
DENSE_ROWS = [1, 63, 64, 65, 130]                              # I - row0: the 64-token workgroup
DENSE_ROW0 = [0, 1, 3]
DENSE_B = [1, 3]
DENSE_MEM_SCALES = [1e3, 1e-3]


def ldp_of(n, extra=0):
    return (n + 3) // 4 * 4 + extra


# ---------------------------------------------------------------------------------------------------------- the front
def pow2_scale(amax, clamp=True):
    """csrc/common.h pow2_scale, elementwise on a float64 tensor: the power of two s with amax s in [2^13, 2^14); 1 for zero"""
    amax = torch.as_tensor(amax, dtype=torch.float64)
    e = 14 - torch.frexp(amax)[1]
    if clamp:
        e = e.clamp(-100, 100)
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    return torch.where((amax > 0) & torch.isfinite(amax), s, torch.ones_like(s))


@functools.lru_cache(maxsize=None)
def front_weights(kind, seed=0):
    """Wqkv (768,256), b (768), Wp (256,256) = proj_p.weight, dcT (32,256) fp32 for an input kind of FRONT_KINDS"""
    g = gen(4000 + seed)
    Wqkv = (torch.rand(3 * C, C, generator=g) * 2 - 1) / 16
    b = (torch.rand(3 * C, generator=g) * 2 - 1) / 16
    Wp = (torch.rand(C, C, generator=g) * 2 - 1) / 16
    dcT = 0.1 * torch.randn(32, C, generator=g)
    decay = torch.randn(32, C, generator=g) * torch.logspace(0, -6, 32).reshape(32, 1)
    big = (torch.rand(3 * C, generator=g) * 2 - 1) * 1e3
    if kind == "wqkv300":
        Wqkv = Wqkv * 300
    elif kind == "wqkv1e-4":
        Wqkv = Wqkv * 1e-4
    elif kind == "wp1e3":
        Wp = Wp * 1e3
    elif kind == "dc1e-5":
        dcT = dcT * 1e-5
    elif kind == "dcdecay":
        dcT = decay           # coefficient rows decaying over six decades, like D_c
    elif kind == "bigbias":
        b = big               # |b| ~ 500 against |x W^T| ~ 0.6
    return types.SimpleNamespace(Wqkv=Wqkv.contiguous(), b=b.contiguous(), Wp=Wp.contiguous(), dcT=dcT.contiguous())


def mixed_special_rows(M):
    """(the all-zero token, the token with a single non-zero channel) of the mixed kind"""
    return M // 3, (2 * M) // 3


@functools.lru_cache(maxsize=None)
def front_x(kind, M, seed=0):
    """x (M,256) fp32.  mixed: token r scaled by 10^(-4 + 8 r / M), one all-zero token, one token with a single non-zero channel."""
    g = gen(5000 + 7 * M + seed)
    x = torch.randn(M, C, generator=g)
    if kind == "mixed":
        x = x * (10.0 ** (-4 + 8 * torch.arange(M, dtype=torch.float64) / M)).float().reshape(M, 1)
        z, s = mixed_special_rows(M)
        x[z] = 0.0
        one = x[s, 77].clone()
        x[s] = 0.0
        x[s, 77] = one
    elif kind == "x1e4":
        x = x * 1e4
    elif kind == "x1e-5":
        x = x * 1e-5
    return x.contiguous()


def front64(x, w):
    """(qkv (M,768), qp (M,4,256), qd (M,4,32)) in float64, from the header comment of rpe_front_kernel
    (PEM/model/transformer.py:395-405): qkv = x Wqkv^T + b; qp[n,h,:] = Wp[64h:64h+64,:]^T q_h; qd[n,h,:] = D_c^T qp[n,h,:]"""
    d = lambda t: t.double()
    qkv = d(x) @ d(w.Wqkv).t() + d(w.b)
    q = qkv[:, :C]
    qp = torch.stack([q[:, D * h:D * h + D] @ d(w.Wp)[D * h:D * h + D, :] for h in range(H)], 1)
    qd = qp @ d(w.dcT).t()
    return qkv, qp, qd


def front64_composed(x, w):
    """the same layer a second way: F.linear for the projection, one einsum over (head, channel) per fold"""
    qkv = F.linear(x.double(), w.Wqkv.double(), w.b.double())
    qh = qkv[:, :C].reshape(-1, H, D)
    qp = torch.einsum("nhk,hkc->nhc", qh, w.Wp.double().reshape(H, D, C))
    qd = torch.einsum("nhc,jc->nhj", qp, w.dcT.double())
    return qkv, qp, qd


def vt64(qkv, Bp, n):
    """vT[cloud][c][tok] (Bp,256,n) from the v third of qkv (Bp n, 768)"""
    return qkv[:, 2 * C:].reshape(Bp, n, C).transpose(1, 2).contiguous()


def tau(K):
    return TIGHTEN[K] * (3 * 2.0 ** -22 + 3 * (32 * math.ceil(K / 32)) * U)


def _stage_bound(A, W, s_w, K, eA=None):
    """bound of one split product A (.., K) . W (N, K)^T: A's rows carry their own scale, W one scale; eA: the error A arrives with"""
    A, W = A.abs(), W.abs()
    s_a = pow2_scale(A.amax(-1, keepdim=True))
    prop = 0.0
    if eA is not None:
        prop = eA @ W.t()
        A = A + eA
        s_a = s_a / 2       # the kernel's own maximum may sit on the other side of a power of two
    ab = 2.0 ** -25 * (A.sum(-1, keepdim=True) / s_w + W.sum(-1) / s_a)
    return prop + tau(K) * (A @ W.t()) + ab


def front_bounds(x, w):
    """(e_qkv, e_qp, e_qd) per element, shapes as front64 (module docstring: chain)"""
    d = lambda t: t.double()
    qkv, qp, qd = front64(x, w)
    s_qkv, s_wp, s_dc = (float(pow2_scale(d(t).abs().max(), clamp=False)) for t in (w.Wqkv, w.Wp, w.dcT))
    acc = d(x) @ d(w.Wqkv).t()
    e_qkv = _stage_bound(d(x), d(w.Wqkv), s_qkv, C) + 4 * U * (acc.abs() + d(w.b).abs())
    e_qp = torch.stack([_stage_bound(qkv[:, D * h:D * h + D], d(w.Wp)[D * h:D * h + D, :].t(), s_wp, D, e_qkv[:, D * h:D * h + D])
                        for h in range(H)], 1)
    e_qd = _stage_bound(qp, d(w.dcT), s_dc, C, e_qp)
    return e_qkv, e_qp, e_qd


def fold_stages(qkv_got, qp_got, w):
    """The two folds one at a time, from the q and qp the implementation itself returned (fp32; they ARE its operands: q and qp pass
    from one product's accumulators to the next product's split): ((want_qp, e_qp), (want_qd, e_qd)) with want in float64 from those
    operands and e = tau(K) |a| . |W| + abs alone -- no inherited error, and the row scale is exactly the kernel's."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    s_wp, s_dc = (float(pow2_scale(d(t).abs().max(), clamp=False)) for t in (w.Wp, w.dcT))
    q, qp = d(qkv_got)[:, :C], d(qp_got).reshape(-1, H, C)
    Wp = d(w.Wp)
    want_qp = torch.stack([q[:, D * h:D * h + D] @ Wp[D * h:D * h + D, :] for h in range(H)], 1)
    e_qp = torch.stack([_stage_bound(q[:, D * h:D * h + D], Wp[D * h:D * h + D, :].t(), s_wp, D) for h in range(H)], 1)
    return (want_qp, e_qp), (qp @ d(w.dcT).t(), _stage_bound(qp, d(w.dcT), s_dc, C))


def front_ratios(got, x, w):
    """worst |err| / bound of (qkv, qp, qd) = got: [qkv, qp chained, qd chained, qp fold alone, qd fold alone]"""
    r = [worst_ratio(g, t, b) for g, t, b in zip(got, front64(x, w), front_bounds(x, w))]
    (want_qp, e_qp), (want_qd, e_qd) = fold_stages(got[0], got[1], w)
    return r + [worst_ratio(got[1], want_qp, e_qp), worst_ratio(got[2], want_qd, e_qd)]


# ------------------------------------------------------------------------------------- CPU emulation of the kernel's arithmetic
def _split(x32):
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi.float(), lo.float()


def _emul_product(A, W, s_w, drop_lo):
    """A (rows, K) fp32 activations, W (N, K) fp32 weights -> A W^T fp32: scale by the row's / the matrix's power of two, hi = fp16(x s),
    lo = fp16(x s - hi), the three products per k-step of 32 summed in fp32, the scales undone (exact)"""
    s_a = pow2_scale(A.double().abs().amax(-1, keepdim=True)).float()
    ah, al = _split(A * s_a)
    wh, wl = _split(W * float(s_w))
    if drop_lo:
        al = torch.zeros_like(al)
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
    for k in range(0, A.shape[1], 32):
        sl = slice(k, k + 32)
        acc = acc + ah[:, sl] @ wl[:, sl].t()
        acc = acc + al[:, sl] @ wh[:, sl].t()
        acc = acc + ah[:, sl] @ wh[:, sl].t()
    return acc * (1.0 / (s_a * float(s_w)))


def front_emulated(x, w, drop_lo=False):
    """the front in the kernel's arithmetic on the CPU, shapes as front64 (fp32); drop_lo: without the activation lo halves"""
    s_qkv, s_wp, s_dc = (float(pow2_scale(t.double().abs().max(), clamp=False)) for t in (w.Wqkv, w.Wp, w.dcT))
    qkv = _emul_product(x, w.Wqkv, s_qkv, drop_lo) + w.b
    wpT = w.Wp.t().contiguous()
    qp = torch.stack([_emul_product(qkv[:, D * h:D * h + D].contiguous(), wpT[:, D * h:D * h + D].contiguous(), s_wp, drop_lo)
                      for h in range(H)], 1)
    qd = _emul_product(qp.reshape(-1, C), w.dcT, s_dc, drop_lo).reshape(-1, H, 32)
    return qkv, qp, qd


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (float64)"""
    got = torch.as_tensor(got).detach().cpu().double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), "non-finite values"
    return float(((got - want).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------- the dense layer
def _linear(g, o, i):
    return (torch.rand(o, i, generator=g) * 2 - 1) / math.sqrt(i), (torch.rand(o, generator=g) * 2 - 1) / math.sqrt(i)


@functools.lru_cache(maxsize=None)
def dense_weights(seed=0):
    """one LinearTransformerLayer: (w, b) pairs lin / exp / sq / q / kv, (gamma, beta) pairs n1 / n2, the focusing `scale` (256)"""
    g = gen(6000 + seed)
    n = lambda: (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g))
    return dict(lin=_linear(g, C, C), n1=n(), exp=_linear(g, 2 * C, C), sq=_linear(g, C, 2 * C), n2=n(), q=_linear(g, C, C),
                kv=_linear(g, 2 * C, C), scale=0.3 * torch.randn(C, generator=g))


@functools.lru_cache(maxsize=None)
def dense_inputs(B, I, J, mem_scale=1.0, seed=0):
    """D (B,I,256) dense tokens and kv (B,J,512) = [proj_k | proj_v] of J memory tokens ~ mem_scale N(0,1), fp32: the projection is
    taken in float64 and rounded once, the rounded rows are the layer's input"""
    g = gen(7000 + 131 * B + 17 * I + J + seed)
    L = dense_weights()
    Dn = torch.randn(B, I, C, generator=g)
    mem = torch.randn(B, J, C, generator=g) * mem_scale
    kv = (mem.double() @ L["kv"][0].double().t() + L["kv"][1].double()).float()
    return Dn.contiguous(), kv.contiguous()


def tail64(hidden, x, L):
    """y = LayerNorm(hidden Wlin^T + b + x); out = LayerNorm(relu(y Wexp^T + b) Wsq^T + b + y)   (PEM/model/transformer.py:152-160, 184-199)"""
    d = lambda t: t.double()
    ln = lambda v, gb: F.layer_norm(v, (C,), d(gb[0]), d(gb[1]), EPS)
    y = ln(hidden @ d(L["lin"][0]).t() + d(L["lin"][1]) + x, L["n1"])
    h = torch.relu(y @ d(L["exp"][0]).t() + d(L["exp"][1]))
    return ln(h @ d(L["sq"][0]).t() + d(L["sq"][1]) + y, L["n2"])


def dense_layer64(Dn, kv, L, row0):
    """LinearTransformerLayer (PEM/model/transformer.py:532-622) on rows row0 .. I-1 of every cloud of Dn (B,I,256) with the projected
    memory rows kv (B,J,512) = k | v: float64, (B, I - row0, 256).  As tests/test_block_gpu.py::test_linattn_layer_vs_oracle_math states
    it, for any J, I, row0."""
    d = lambda t: t.double()
    Dt = d(Dn[:, row0:])
    q = Dt @ d(L["q"][0]).t() + d(L["q"][1])
    k, v = d(kv[..., :C]), d(kv[..., C:])
    sp = F.softplus(d(L["scale"]))

    def phi(z):
        z = (torch.relu(z) + 1e-6) / sp
        n = z.norm(dim=-1, keepdim=True)
        z3 = z ** 3
        return z3 / z3.norm(dim=-1, keepdim=True) * n
    q, k = phi(q), phi(k)
    hid = torch.zeros_like(q)
    for h in range(H):
        sl = slice(D * h, D * h + D)
        z = 1.0 / (torch.einsum("bic,bc->bi", q[..., sl], k[..., sl].sum(1)) + 1e-6)
        kvm = torch.einsum("bjc,bjd->bcd", k[..., sl], v[..., sl])
        hid[..., sl] = torch.einsum("bic,bcd,bi->bid", q[..., sl], kvm, z)
    return tail64(hid, Dt, L)
