"""Every dispatch route of sam6d_gemm_nt / _w16 / _b2 (csrc/gemm.hip gemm_pick) against a float64 host reference at the shapes that
select it: the exact fp32 kernel, the fp16-split kernel with the weight tile split per k-step and with pre-split (w16) weights, each
with 64 x 64 and 128 x 128 tiles, and the whole-tile FAST specialisation; the plain, column-group and batch-fold workgroup orders with
their padding; the wide and narrow epilogues; matmul modes 0, 1, 2 and mode 2 with the keep-split flag; the per-tile range fallback.

Each case first proves which route it runs (pem.gemm_route = the launch decision itself), then checks every element against a
condition-aware bound (below) and checks guard bands around the output for stray writes.

Error bound, per element (i, j), with P = |A| . |W|^T in float64, u = 2^-24, s = the pre-split weight scale (1 without w16):
    |got - ref| <= (tau * P + abs) * |colscale| / |divisor| + 4u * (|acc| * |colscale| / |divisor| + |bias| + |residual|)
  * mode 0 (v_mfma_f32_32x32x2_f32 = a k-ordered fmaf chain, one rounding per product): tau = K u (gamma_K), abs = 0.
  * mode 1: x = hi + lo + d with |x - hi| <= 2^-11 |x| and |d| <= 2^-22 |x| + 2^-25 (lo rounded to fp16, whose subnormal spacing is
    2^-24); a.b - (ah bh + ah bl + al bh) = a db + da b - da db + al bl, so each product is off by <= 3 * 2^-22 |a||b| plus
    2^-25 (|a| + |b| / s).  The fp16 products are exact in fp32; the 3 * K32 of them (K32 = K rounded up to 32, the zero-padded tail)
    are accumulated in fp32 with at most one rounding each: tau = 3 * 2^-22 + 3 * K32 * u, abs = 2^-24 (sum_k |a_k| + sum_k |w_k| / s).
  * mode 2 (hi . hi only): the dropped lo halves are <= 2^-11 |x| each: ceiling tau = 2 * 2^-11 + 2^-22 + K32 * u.  Floor: the median of
    |got - ref| / P must be >= 2^-20 -- a product of K random-sign terms of size ~2^-12 |a||b| sits near 2^-12 / sqrt(K) >> 2^-20, the
    full split stays near 1e-8 << 2^-20; so a mode-2 route that silently kept the lo halves fails.  With act | 16, mode 2 keeps the
    split and must meet the mode-1 bound.
  The derived tau are worst cases; TIGHTEN scales them down by what the MI355X runs showed (only ever tightened, never loosened).
  Observed maximum of |got - ref| / bound on the MI355X with the derived tau (TIGHTEN = 1): mode 0 0.24 (K = 20; 0.04 - 0.08 at
  K = 72 - 100), mode 1 0.020 (0.0035 - 0.020 over the routes), mode 2 0.26.  Tightened from that to mode 1 x 1/8, mode 2 x 1/2,
  mode 0 as derived; with those: mode 0 0.24, mode 1 0.14 (range-fallback tests 0.22), mode 2 0.52.  Mode-2 median |err| / P
  1.9e-5 - 3.2e-5, split routes <= 1.5e-8.

The whole-tile FAST kernel and the general pre-split 128 x 128 kernel share every arithmetic step (only the load ring differs), so
their outputs must be bit-identical; `colscale` = ones forces the general kernel (a multiply by 1.0f is exact)."""
import math
import os
import re

import pytest
import torch

from tests._util import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TIGHTEN = {0: 1.0, 1: 1.0 / 8, 2: 1.0 / 2}  # scale of the derived tau per arithmetic (from the first MI355X run; module docstring)


def _route_bits():
    txt = open(os.path.join(ROOT, "include", "sam6d_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+SAM6D_GEMM_ROUTE_([A-Z0-9_]+)\s+(\d+)", txt)}


R = _route_bits()
EXACT, H3, W16 = R["EXACT"], R["H3"], R["H3_W16"]
T128, FAST, WIDE, HALF = R["TILE128"], R["FAST"], R["WIDE"], R["HALF"]
PLAIN, CG, FOLD, NONE = R["PLAIN"], R["COLGROUP"], R["FOLD"], R["NONE"]


def _half_enabled():
    return bool(int(os.environ.get("SAM6D_HALF_MASK", "15")) & 1)


class _Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from sam6d_hip import _lib
        _lib.call("sam6d_set_thread_matmul_mode", self.mode)

    def __exit__(self, *exc):
        from sam6d_hip import _lib
        _lib.call("sam6d_set_thread_matmul_mode", -1)


def _case(name, mode, M, N, K, code, *, batch=1, batch2=1, lda=None, ldw=None, ldc=None, sA=None, sW=0, sC=None, sA2=0, sW2=0,
          sC2=0, a_off=0, w_off=0, c_off=None, c_shift=0, bias=False, colscale=False, divisor=1.0, act=0, res="none", w16=False,
          qk=False):
    """qk: A and W are the q and k column blocks of one (batch, M, 3 x 256) qkv buffer (pem.py's per-head q.k^T through gemm_b2)."""
    lda = K if lda is None else lda
    ldw = K if ldw is None else ldw
    ldc = (N + 4) if ldc is None else ldc  # guard columns right of every row
    sA = M * lda if sA is None else sA
    sC = (M + 1) * ldc if sC is None else sC  # one guard row between batch elements
    c_off = (2 * ldc if c_off is None else c_off) + c_shift  # two guard rows in front
    return dict(name=name, mode=mode, M=M, N=N, K=K, code=code, batch=batch, batch2=batch2, lda=lda, ldw=ldw, ldc=ldc, sA=sA, sW=sW,
                sC=sC, sA2=sA2, sW2=sW2, sC2=sC2, a_off=a_off, w_off=w_off, c_off=c_off, bias=bias, colscale=colscale, divisor=divisor,
                act=act, res=res, w16=w16, qk=qk)


BIG_M = 16384 + 3 * 128  # tm = 131: not a multiple of 8, the last column group is padded
EPI = dict(bias=True, colscale=True, divisor=0.75, act=1)
NB, NQ, H = 9, 197, 4  # q.k^T of pem.py's materialised RPE attention: 9 clouds x 4 heads = 36 problems of 197 x 197 x 64
LDP = 200

CASES = [
    # --- the exact fp32 kernel: mode 1 with K < 32, and mode 0
    _case("exact64_k_lt_32", 1, 300, 200, 24, EXACT | PLAIN, bias=True),
    _case("exact128_k_lt_32", 1, BIG_M, 1024, 20, EXACT | T128 | CG, res="sep"),
    _case("exact64_mode0", 0, 1000, 130, 100, EXACT | PLAIN, **EPI),
    _case("exact128_mode0_plain", 0, BIG_M, 1026, 72, EXACT | T128 | PLAIN, res="inplace", **EPI),
    # --- split kernel, weight split per k-step
    _case("h3_64", 1, 777, 260, 200, H3 | WIDE | PLAIN, res="sep", **EPI),
    _case("h3_64_mode2", 2, 777, 260, 200, H3 | WIDE | HALF | PLAIN),
    _case("h3_128_colgroup_tails", 1, BIG_M, 1024, 200, H3 | T128 | WIDE | CG, res="sep", **EPI),
    _case("h3_128_mode2", 2, BIG_M, 1024, 96, H3 | T128 | WIDE | HALF | CG),
    _case("h3_128_mode2_keep_split", 2, BIG_M, 1024, 96, H3 | T128 | WIDE | CG, act=16),
    _case("h3_128_plain_narrow", 1, BIG_M + 5, 1026, 72, H3 | T128 | PLAIN, res="sep", **EPI),  # N % 4 != 0: narrow epilogue
    _case("h3_128_misaligned_c", 1, BIG_M, 1024, 64, H3 | T128 | CG, c_shift=1, res="inplace", bias=True),  # odd c_off: narrow
    _case("h3_128_fold33", 1, 1024 + 40, 512, 64, H3 | T128 | WIDE | FOLD, batch=33, sW=512 * 64, bias=True),
    _case("b2_qk_fold36", 1, NQ, NQ, 64, H3 | FOLD, batch=NB, batch2=H, lda=3 * 256, ldw=3 * 256, ldc=H * LDP, sA=NQ * 3 * 256,
          sW=NQ * 3 * 256, sC=NQ * H * LDP, sA2=64, sW2=64, sC2=LDP, w_off=256, c_off=0, qk=True),
    # --- split kernel, pre-split weights
    _case("w16_64", 1, 777, 256, 256, W16 | WIDE | PLAIN, res="sep", **EPI),
    _case("w16_64_mode2", 2, 777, 256, 256, W16 | WIDE | HALF | PLAIN),
    _case("w16_128_tails_inplace", 1, BIG_M + 7, 1024 + 36, 200, W16 | T128 | WIDE | PLAIN, res="inplace", **EPI),
    _case("w16_128_colgroup", 1, BIG_M, 1024, 200, W16 | T128 | WIDE | CG, res="sep", bias=True),
    _case("w16_128_mode2", 2, BIG_M, 1024, 200, W16 | T128 | WIDE | HALF | CG),
    # --- whole-tile specialisation
    _case("fast_colgroup_inplace", 1, 16384, 1024, 160, W16 | T128 | FAST | WIDE | CG, res="inplace", bias=True, w16=True),
    # the bg-row layout of _tokens_with_bg (pem.py): 32 clouds x 2048 tokens, output row 0 of every cloud is the bg token
    _case("fast_bg_rows_fold32", 1, 2048, 256, 256, W16 | T128 | FAST | WIDE | FOLD, batch=32, ldc=256, sC=2049 * 256, c_off=256,
          bias=True, w16=True),
]
for _c in CASES:
    if _c["code"] & 3 == W16:
        _c["w16"] = True

REQUIRED = {  # every kernel in mode 1, the six general kernels in mode 0 or 2 where that mode reaches them, every order
    "exact64": lambda c: c & 7 == EXACT, "exact128": lambda c: c & 7 == EXACT | T128,
    "h3_64": lambda c: c & 7 == H3, "h3_128": lambda c: c & 7 == H3 | T128,
    "w16_64": lambda c: c & 7 == W16, "w16_128": lambda c: c & 15 == W16 | T128, "fast": lambda c: c & FAST,
    "h3_64_half": lambda c: c & 7 == H3 and c & HALF, "h3_128_half": lambda c: c & 7 == H3 | T128 and c & HALF,
    "w16_64_half": lambda c: c & 7 == W16 and c & HALF, "w16_128_half": lambda c: c & 7 == W16 | T128 and c & HALF,
    "plain128": lambda c: c & T128 and c & 192 == PLAIN, "colgroup": lambda c: c & 192 == CG, "fold128": lambda c: c & T128 and c & FOLD,
    "fold64": lambda c: not c & T128 and c & FOLD, "narrow128": lambda c: c & 3 and c & T128 and not c & WIDE,
    "wide128": lambda c: c & T128 and c & WIDE,
}


def _extent(off, dims, strides, row):
    return off + sum((d - 1) * s for d, s in zip(dims, strides)) + row


def _view(flat, c, off, ld, s, s2, rows, cols):
    return torch.as_strided(flat, (c["batch"], c["batch2"], rows, cols), (s, s2, ld, 1), off)


class _Buffers:
    """Device buffers of one case, guard slack included; out is NaN everywhere (the written region holds the residual for the in-place
    form)."""

    def __init__(self, c, dev, seed, a_hook=None, w_hook=None):
        from sam6d_hip import pem
        g = torch.Generator().manual_seed(seed)
        M, N, K, B1, B2 = c["M"], c["N"], c["K"], c["batch"], c["batch2"]
        if c["qk"]:  # one qkv buffer: A = q columns, W = k columns of the same rows
            ea = _extent(0, (B1, M), (c["sA"], c["lda"]), c["lda"])
            self.A = torch.randn(ea + 64, generator=g)
            self.W = self.A
        else:
            ea = _extent(c["a_off"], (B1, B2, M), (c["sA"], c["sA2"], c["lda"]), K)
            ew = _extent(c["w_off"], (B1, B2, N), (c["sW"], c["sW2"], c["ldw"]), K)
            self.A = torch.randn(ea + 64, generator=g)
            self.W = torch.randn(ew + 64, generator=g)
        if a_hook:
            a_hook(self)
        if w_hook:
            w_hook(self)
        self.bias = torch.randn(N, generator=g) if c["bias"] else None
        self.cs = (torch.rand(N, generator=g) + 0.5) if c["colscale"] else None
        self.ec = _extent(c["c_off"], (B1, B2, M), (c["sC"], c["sC2"], c["ldc"]), N) + 3 * c["ldc"] + 5  # guard rows after the last row
        b1 = torch.arange(B1).view(B1, 1, 1, 1) * c["sC"]
        b2 = torch.arange(B2).view(1, B2, 1, 1) * c["sC2"]
        m = torch.arange(M).view(1, 1, M, 1) * c["ldc"]
        n = torch.arange(N).view(1, 1, 1, N)
        self.idx = (c["c_off"] + b1 + b2 + m + n).to(dev)
        self.Rsep = None
        if c["res"] == "sep":
            self.ldr, self.sR, self.r_off = N + 8, (M + 2) * (N + 8), 5 * (N + 8)
            er = _extent(self.r_off, (B1, M), (self.sR, self.ldr), N)
            self.Rsep = torch.randn(er + 64, generator=g)
        self.Rin = torch.randn(B1, B2, M, N, generator=g) if c["res"] == "inplace" else None
        self.Ad = self.A.to(dev)
        self.Wd = self.Ad if self.W is self.A else self.W.to(dev)
        self.biasd = self.bias.to(dev) if self.bias is not None else None
        self.csd = self.cs.to(dev) if self.cs is not None else None
        self.Rsepd = self.Rsep.to(dev) if self.Rsep is not None else None
        self.w16 = pem.split_w16(self.Wd) if c["w16"] else None
        self.dev = dev
        self.reset()

    def reset(self):
        self.out = torch.full((self.ec,), float("nan"), device=self.dev)
        if self.Rin is not None:
            self.out[self.idx] = self.Rin.to(self.dev)

    def kwargs(self, c):
        kw = dict(a_off=c["a_off"], w_off=c["w_off"], c_off=c["c_off"], colscale=self.csd, batch=c["batch"], sA=c["sA"], sW=c["sW"],
                  sC=c["sC"], divisor=c["divisor"], act=c["act"], w16=self.w16)
        if c["res"] == "sep":
            kw.update(residual=self.Rsepd, r_off=self.r_off, ldr=self.ldr, sR=self.sR)
        elif c["res"] == "inplace":
            kw.update(residual=self.out, r_off=c["c_off"], ldr=c["ldc"], sR=c["sC"])
        return kw

    def route(self, c):
        from sam6d_hip import pem
        if c["batch2"] > 1:
            return pem.gemm_route(self.Ad, self.Wd, None, self.out, c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], a_off=c["a_off"],
                                  w_off=c["w_off"], c_off=c["c_off"], batch=c["batch"], sA=c["sA"], sW=c["sW"], sC=c["sC"],
                                  batch2=c["batch2"], sA2=c["sA2"], sW2=c["sW2"], sC2=c["sC2"])
        return pem.gemm_route(self.Ad, self.Wd, self.biasd, self.out, c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], **self.kwargs(c))

    def launch(self, c):
        from sam6d_hip import pem
        if c["batch2"] > 1:
            pem.gemm_b2(self.Ad, self.Wd, self.out, c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], c["batch"], c["sA"], c["sW"],
                        c["sC"], c["batch2"], c["sA2"], c["sW2"], c["sC2"], a_off=c["a_off"], w_off=c["w_off"], c_off=c["c_off"])
        else:
            pem.gemm(self.Ad, self.Wd, self.biasd, self.out, c["M"], c["N"], c["K"], c["lda"], c["ldw"], c["ldc"], **self.kwargs(c))
        torch.cuda.synchronize()

    def result(self):
        """(written elements as (batch, batch2, M, N) float64 on the host, after checking they are finite and every guard is untouched)"""
        got = self.out[self.idx]
        assert torch.isfinite(got).all(), "%d written elements are not finite (a tile was not written)" % int((~torch.isfinite(got)).sum())
        guard = torch.ones(self.ec, dtype=torch.bool, device=self.dev)
        guard[self.idx] = False
        gb = self.out[guard].view(torch.int32)
        nan_bits = torch.tensor([float("nan")], device=self.dev).view(torch.int32)
        assert bool((gb == nan_bits).all()), "%d guard elements were written" % int((gb != nan_bits).sum())
        return got.cpu().double()

    def reference(self, c, exact=False):
        """(ref, bound, P scaled) in float64 for the arithmetic of mode c['mode'] (module docstring); exact: the mode-0 bound."""
        M, N, K = c["M"], c["N"], c["K"]
        A = _view(self.A, c, c["a_off"], c["lda"], c["sA"], c["sA2"], M, K).double()
        W = _view(self.W, c, c["w_off"], c["ldw"], c["sW"], c["sW2"], N, K).double()
        acc = A @ W.transpose(-1, -2)
        P = A.abs() @ W.abs().transpose(-1, -2)
        mode = c["mode"]
        k32 = 32 * math.ceil(K / 32)
        if exact or mode == 0 or K < 32:
            tau, ab = K * U * TIGHTEN[0], 0.0
        elif mode == 2 and not c["act"] & 16 and _half_enabled():
            tau, ab = (2 * 2.0 ** -11 + 2.0 ** -22 + k32 * U) * TIGHTEN[2], None
        else:
            tau, ab = (3 * 2.0 ** -22 + 3 * k32 * U) * TIGHTEN[1], None
        if ab is None:
            s = self.w16[2] if self.w16 is not None else 1.0
            ab = 2.0 ** -24 * (A.abs().sum(-1, keepdim=True) + W.abs().sum(-1).unsqueeze(-2) / s)
        scale = 1.0 / abs(c["divisor"])
        if self.cs is not None:
            scale = scale * self.cs.double().abs()
        y = acc / c["divisor"]
        if self.cs is not None:
            y = y * self.cs.double()
        b = self.bias.double() if self.bias is not None else torch.zeros(N, dtype=torch.float64)
        y = y + b
        if c["act"] & 1:
            y = y.clamp(min=0)
        r = torch.zeros(1, dtype=torch.float64)
        if c["res"] == "sep":
            r = _view(self.Rsep, dict(c, batch2=1), self.r_off, self.ldr, self.sR, 0, M, N).double()
        elif c["res"] == "inplace":
            r = self.Rin.double()
        y = y + r
        bound = (tau * P + ab) * scale + 4 * U * (acc.abs() * scale + b.abs() + r.abs())
        return y, bound, P * scale


def _check(got, ref, bound, what):
    err = (got - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    bad = int((ratio > 1).sum())
    assert bad == 0, "%s: %d elements over the bound, worst |err| / bound %.2f at %s" % (what, bad, worst,
                                                                                       tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]))
    return worst


def _presplit_used():
    """pem.gemm passes pre-split weights in the split-precision modes of the environment's Options (not under SAM6D_MATMUL_MODE=0)."""
    from sam6d_hip import pem
    return pem._flags().w16


def _skip_if_unreachable(c):
    if c["code"] & HALF and not _half_enabled():
        pytest.skip("SAM6D_HALF_MASK clears the GEMM family: mode 2 keeps the split")
    if c["w16"] and not _presplit_used():
        pytest.skip("SAM6D_MATMUL_MODE=0 in the environment: pem.gemm does not use pre-split weights")


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_gemm_route_vs_fp64(dev, c):
    _skip_if_unreachable(c)
    bufs = _Buffers(c, dev, seed=len(c["name"]) * 1000 + c["M"] % 997 + c["N"])
    with _Mode(c["mode"]):
        code = bufs.route(c)
        assert code == c["code"], "%s: route %d, expected %d" % (c["name"], code, c["code"])
        bufs.launch(c)
    got = bufs.result()
    ref, bound, P = bufs.reference(c)
    worst = _check(got, ref, bound, c["name"])
    med = float(((got - ref).abs() / P).median())
    if code & HALF:  # floor: the lo halves really were dropped
        assert med >= 2.0 ** -20, "%s: median |err| / P = %.2e: mode 2 kept the split precision" % (c["name"], med)
    print("\n[%s] route %d, max |err| / bound %.3e, median |err| / P %.2e" % (c["name"], code, worst, med))


def test_route_matrix_covers_every_route():
    """The case table reaches every kernel, order and epilogue (each case asserts its own code at run time, so a change that moves a
    case to another route fails there)."""
    codes = {c["code"] for c in CASES}
    missing = [k for k, f in REQUIRED.items() if not any(f(x) for x in codes)]
    assert not missing, missing
    modes = {(c["code"] & 7 | c["code"] & FAST, c["mode"]) for c in CASES}
    for k in (EXACT, EXACT | T128, H3, H3 | T128, W16, W16 | T128, W16 | T128 | FAST):
        assert (k, 1) in modes, "kernel %d has no mode-1 case" % k


def test_route_query_matches_launch_decision(dev):
    """gemm_route reads the thread's mode like the launch: the same arguments route differently in modes 0 / 1 / 2, and M, N or batch
    = 0 report no launch."""
    from sam6d_hip import pem
    A = torch.zeros(BIG_M * 64, device=dev)
    W = torch.zeros(1024 * 64, device=dev)
    out = torch.zeros(BIG_M * 1024, device=dev)
    got = {}
    for mode in (0, 1, 2):
        with _Mode(mode):
            got[mode] = pem.gemm_route(A, W, None, out, BIG_M, 1024, 64, 64, 64, 1024)
    assert got[0] == EXACT | T128 | CG and got[1] == H3 | T128 | WIDE | CG
    assert got[2] == (H3 | T128 | WIDE | CG | (HALF if _half_enabled() else 0))
    for M, N, b in ((0, 1024, 1), (BIG_M, 0, 1), (BIG_M, 1024, 0)):
        assert pem.gemm_route(A, W, None, out, M, N, 64, 64, 64, 1024, batch=b) == NONE


@pytest.mark.parametrize("layout", ["bg_rows_fold32", "single_colgroup"])
def test_fast_bits_equal_general_presplit(dev, layout):
    """FAST and the general pre-split 128 x 128 kernel on the same inputs: the same bits (colscale = ones forces the general one)."""
    if not _presplit_used():
        pytest.skip("SAM6D_MATMUL_MODE=0 in the environment: pem.gemm does not use pre-split weights")
    if layout == "bg_rows_fold32":
        c = _case(layout, 1, 2048, 256, 256, 0, batch=32, ldc=256, sC=2049 * 256, c_off=256, bias=True, w16=True, res="sep")
        order = FOLD
    else:
        c = _case(layout, 1, 16384, 1024, 96, 0, bias=True, w16=True, res="inplace")
        order = CG
    bufs = _Buffers(c, dev, seed=77)
    with _Mode(1):
        assert bufs.route(c) == W16 | T128 | FAST | WIDE | order
        bufs.launch(c)
        fast = bufs.result()
        bufs.reset()
        bufs.csd = torch.ones(c["N"], device=dev)
        assert bufs.route(c) == W16 | T128 | WIDE | order
        bufs.launch(c)
        general = bufs.result()
    assert torch.equal(fast, general), "%d elements differ between the FAST and the general pre-split kernel" % int((fast != general).sum())


RANGE_ROUTES = {"h3_128": H3 | T128 | WIDE | PLAIN, "w16_128": W16 | T128 | WIDE | PLAIN, "fast": W16 | T128 | FAST | WIDE | PLAIN}


@pytest.mark.parametrize("route", list(RANGE_ROUTES))
def test_gemm_range_fallback_per_tile(dev, route):
    """Row tile 3 of A at >= 32768 and row tile 10 below 2^-6: those tiles are recomputed by the exact loop -- bit-identical to the mode-0
    kernel (so the pre-split route does not apply its weight unscale to them), every other tile bit-identical to a run without the
    outliers, and the whole result within the mode-1 bound (the recomputed tiles within the mode-0 bound)."""
    M = N = 4096
    K = 64
    code = RANGE_ROUTES[route]
    c = _case(route, 1, M, N, K, code, ldc=N, bias=True, colscale=(route != "fast"), w16=(route != "h3_128"))
    _skip_if_unreachable(c)
    clean = _Buffers(c, dev, seed=31)
    with _Mode(1):
        assert clean.route(c) == code
        clean.launch(c)
    base = clean.result()

    def outliers(b):
        a = b.A[:M * K].view(M, K)
        a[3 * 128:4 * 128] *= 40000.0
        a[10 * 128:11 * 128] *= 1e-3

    bufs = _Buffers(c, dev, seed=31, a_hook=outliers)
    with _Mode(1):
        assert bufs.route(c) == code
        bufs.launch(c)
    got = bufs.result()
    rows = torch.zeros(M, dtype=torch.bool)
    rows[3 * 128:4 * 128] = True
    rows[10 * 128:11 * 128] = True
    ref, bound, _ = bufs.reference(c)
    bound[..., rows, :] = bufs.reference(c, exact=True)[1][..., rows, :]
    worst = _check(got, ref, bound, route + " with outlier tiles")
    print("\n[range %s] max |err| / bound %.3e" % (route, worst))
    assert torch.equal(got[..., ~rows, :], base[..., ~rows, :]), "tiles without outliers changed: the fallback is not per tile"
    assert not torch.equal(got[..., rows, :], base[..., rows, :])
    bufs.reset()
    with _Mode(0):
        assert bufs.route(c) == EXACT | T128 | PLAIN
        bufs.launch(c)
    exact = bufs.result()
    assert torch.equal(got[..., rows, :], exact[..., rows, :]), "fallback tiles differ from the exact kernel"


@pytest.mark.parametrize("M,N,K,code", [(4096, 4096, 64, W16 | T128 | FAST | WIDE | PLAIN), (700, 256, 256, W16 | WIDE | PLAIN)])
def test_presplit_weight_rows_spanning_2e16(dev, M, N, K, code):
    """BN-folded weights: row n of W scaled by 2^(-16 n / (N - 1)), one pack scale for all.  Every column meets the bound at its own
    scale (the bound is per element: P carries the column's scale)."""
    c = _case("bn_rows", 1, M, N, K, code, w16=True)
    _skip_if_unreachable(c)

    def fold(b):
        w = b.W[:N * K].view(N, K)
        w *= torch.exp2(-16.0 * torch.arange(N, dtype=torch.float32) / (N - 1)).view(N, 1)

    bufs = _Buffers(c, dev, seed=5, w_hook=fold)
    with _Mode(1):
        assert bufs.route(c) == code
        bufs.launch(c)
    got = bufs.result()
    ref, bound, _ = bufs.reference(c)
    worst = _check(got, ref, bound, "pre-split rows over 2^-16 .. 1")
    print("\n[bn rows %d x %d x %d] max |err| / bound %.3e" % (M, N, K, worst))
    col = (got - ref).abs().amax(dim=(0, 1, 2)) / ref.abs().amax(dim=(0, 1, 2))
    assert float(col[-1]) < 1e-4 and float(col.max()) < 1e-4, "column-relative error %.2e" % float(col.max())


def test_gemm_error_contract(dev):
    """batch x batch2 > 65535 is refused before any launch; M = 0, N = 0 or batch = 0 launch nothing and leave `out` untouched."""
    from sam6d_hip import pem
    A = torch.randn(64 * 64, device=dev)
    out = torch.full((64 * 64,), float("nan"), device=dev)
    bits = out.view(torch.int32).clone()
    with pytest.raises(RuntimeError, match="65535"):
        pem.gemm_b2(A, A, out, 1, 1, 32, 32, 32, 1, 300, 0, 0, 0, 300, 0, 0, 0)
    with pytest.raises(RuntimeError, match="65535"):
        pem.gemm_route(A, A, None, out, 1, 1, 32, 32, 32, 1, batch=300, batch2=300)
    for M, N, b in ((0, 64, 1), (64, 0, 1), (64, 64, 0)):
        for mode in (0, 1):
            with _Mode(mode):
                pem.gemm(A, A[:64 * 32], None, out, M, N, 32, 32, 32, 64, batch=b)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), bits), "an empty GEMM wrote to out"
