"""The inputs and bounds of tests/test_attn_shapes_gpu.py, proved on the CPU: the float64 restatements of tests/attn_shapes_ref.py
reproduce the reference's own outputs at the golden shape (tests/golden/submodules.npz, transformer.npz, sparse_to_dense.npz, on the
sampled rows those files hold), the seeded builders meet the conditions they state, and the fp32 CPU evaluation of the same formulas
alone meets every entry of R.TOL on every case of the lists -- so the GPU file holds no kernel to a bound that plain fp32 arithmetic
would miss.  Each test prints the fp32 evaluation's measured error next to the bound."""
import math

import numpy as np
import pytest
import torch

from tests import attn_shapes_ref as R
from tests._util import golden


@pytest.fixture(scope="module")
def sd():
    from sam6d_hip import synth
    return synth.make_pem_weights(1)


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) if got.numel() else 0.0


COARSE = "coarse_point_matching.transformers.0"
DENSE = "fine_point_matching.transformers.0.dense_layer"


# ------------------------------------------------------------------------------------------------------- golden shape
def test_restatements_reproduce_the_golden_sinusoid():
    g = golden("submodules")
    idx, div = torch.from_numpy(g["sin_idx"]).reshape(-1), torch.from_numpy(g["sin_div_term"])
    e = _err(R.sinusoid_ref(idx, div), g["sin"].reshape(8, 256))
    print("sinusoid_ref vs the reference's fp32 embedding (arguments to 866): %.2e (bound 2e-7)" % e)
    assert e <= 2e-7


def test_restatements_reproduce_the_golden_cross_modules(sd):
    """MultiHeadAttention, AttentionLayer and TransformerLayer of the cross layer: every 4th query row (hidden, output), every 8th
    (probabilities), all rows of the whole layer -- within the bounds tests/test_submodules_gpu.py holds the kernels to"""
    g, t = golden("submodules"), golden("transformer")
    x, y, _, _ = R.layer_inputs(int(g["seed"]))
    W = R.layer_weights(sd, COARSE + ".layers.1", False)
    hid, p = R.mha64(x, y, y, W)
    figures = dict(hidden=(_err(hid[:, ::4], g["mha_hidden"]), R.TOL["mha_hidden"]), probs=(_err(p[:, :, ::8], g["mha_scores"]), R.TOL["mha_probs"]),
                   attn_out=(_err(R.attention_layer64(x, y, W)[:, ::4], g["attn_out"]), R.TOL["layer"]),
                   layer=(_err(R.layer64(x, y, W), t["cross"]), R.TOL["layer"]))
    for k, (e, b) in figures.items():
        print("cross %-9s float64 restatement vs golden: %.2e (bound %.1e)" % (k, e, b))
        assert e <= b / 4, "the restatement sits a factor of four inside the bound"


def test_restatements_reproduce_the_golden_rpe_modules(sd):
    g, t = golden("submodules"), golden("transformer")
    x, _, e0, _ = R.layer_inputs(int(g["seed"]))
    W = R.layer_weights(sd, COARSE + ".layers.0", True)
    xs, es = x[:, ::4].contiguous(), e0[:, ::4].contiguous()  # the query rows the file holds: a query row depends on no other
    hid, p = R.mha64(xs, x, x, W, es)
    figures = dict(hidden=(_err(hid, g["rpe_hidden"]), 3e-5), probs=(_err(p[:, :, ::2], g["rpe_scores"]), 3e-6),
                   attn_out=(_err(R._attn_layer(hid, xs.double(), W), g["rpe_attn_out"]), R.TOL["layer"]),
                   ffn=(_err(R.output64(xs, W), g["ffn_out"]), R.TOL["layer"]),
                   layer=(_err(R._output(R._attn_layer(hid, xs.double(), W), W), t["rpe"][:, ::4]), R.TOL["layer"]))
    for k, (e, b) in figures.items():
        print("rpe %-9s float64 restatement vs golden: %.2e (bound %.1e)" % (k, e, b))
        assert e <= b / 4


def test_restatements_reproduce_the_golden_linear_attention(sd):
    g = golden("submodules")
    gen = R.gen(int(g["seed_dense"]))
    d0 = torch.randn(1, 2049, 256, generator=gen)
    d1 = torch.randn(1, 2049, 256, generator=gen)
    q_in, m_in = d0[:, 1:].contiguous(), d1[:, 1:197].contiguous()
    W = R.layer_weights(sd, DENSE, False)
    scale = sd[DENSE + ".attention.attention.scale"].reshape(-1)
    figures = dict(attn=(_err(R.linattn_layer64(q_in, m_in, W, scale, "attn")[:, ::16], g["linattn"]), 2e-5),
                   attn_layer=(_err(R.linattn_layer64(q_in, m_in, W, scale, "attn_layer")[:, ::16], g["linattn_layer"]), R.TOL["layer"]),
                   layer=(_err(R.linattn_layer64(q_in, m_in, W, scale)[:, ::8], golden("sparse_to_dense")["lin_rows"]), R.TOL["layer"]))
    for k, (e, b) in figures.items():
        print("linear attention %-10s float64 restatement vs golden: %.2e (bound %.1e)" % (k, e, b))
        assert e <= b / 4


# ------------------------------------------------------------------------------------------------------- 1. attention
def _attn_cases():
    return [(False, s) for s in R.PLAIN_SHAPES] + [(True, s) for s in R.RPE_SHAPES]


@pytest.mark.parametrize("kind", R.ATTN_KINDS)
def test_fp32_attention_meets_the_bound(kind):
    """every shape of both routes: the fp32 evaluation is inside 3e-6 x max(1, max |want|); the builders' conditions: a lead of at least
    30 (dominant, large) with logits of a few hundred (large), bitwise equal keys and probabilities of exactly 1 / m in float64 (equal)"""
    worst = 0.0
    for rpe, (B, n, m) in _attn_cases():
        t = R.attn_inputs(kind, B, n, m, rpe)
        want, p, s = R.attention64(t.q, t.k, t.v, t.qp, t.E)
        e = _err(R.attention32(t.q, t.k, t.v, t.qp, t.E)[0], want) / max(1.0, float(want.abs().max()))
        worst = max(worst, e)
        assert e <= R.TOL["attn"], (rpe, B, n, m, e)
        if kind in ("dominant", "large"):
            lead = R.lead_key(B, n, m)
            assert R.logit_lead(s, lead) >= 30.0, (rpe, B, n, m, R.logit_lead(s, lead))
            vrow = torch.gather(t.v, 1, lead[:, :, None].expand(B, n, R.C))
            assert _err(want, vrow) <= R.rel_bound(want, R.TOL["attn"]) / 100, "float64: the output is the leading key's v row"
            if kind == "large" and m > 1:
                assert 300.0 <= float(s.max()) <= 500.0, "logits of a few hundred"
        if kind == "equal":
            assert bool((t.k == t.k[:, :1]).all()) and (t.E is None or bool((t.E == t.E[:, :, :1]).all()))
            assert _err(want, t.v.double().mean(1, keepdim=True).expand(B, n, R.C)) <= 1e-13
    print("attention %-8s fp32 evaluation, worst over %d cases: %.2e of max(1, max |want|) (bound %.1e)" % (kind, len(_attn_cases()), worst, R.TOL["attn"]))
    if kind == "random":
        assert worst <= R.TOL["attn"] / 3, "unit scale: the bound leaves a factor of three or more for another summation order"


def test_single_key_is_exact():
    t = R.attn_inputs("random", 1, 1, 1, False)
    assert torch.equal(R.attention32(t.q, t.k, t.v)[0], t.v), "one key: probability exactly 1, the output is the v row bit for bit"
    for layout, per_route in R.LAYOUT_SHAPES.items():
        for rpe, shapes in per_route.items():
            assert len(shapes) == 2 and all(s in (R.RPE_SHAPES if rpe else R.PLAIN_SHAPES) for s in shapes)
            assert layout != "qkv768" or all(n == m for _, n, m in shapes), "one (B,n,768) buffer holds as many keys as queries"


# ------------------------------------------------------------------------------------------------------- 2. softmax, sinusoid
@pytest.mark.parametrize("n", R.SOFTMAX_N)
def test_fp32_softmax_meets_the_bounds(n):
    worst, worst_sum = 0.0, 0.0
    for rows in R.SOFTMAX_ROWS:
        a, b = R.softmax_inputs(rows, n)
        for bb in (None, b):
            for scale in R.SOFTMAX_SCALES:
                want, got = R.softmax64(a, bb, scale), R.softmax32(a, bb, scale)
                worst = max(worst, _err(got, want))
                worst_sum = max(worst_sum, float((got.double().sum(1) - 1.0).abs().max()) / R.ULP1)
    print("softmax n %d: fp32 evaluation %.2e (bound %.1e), row sums off by %.2f ulp (bound %d)" % (n, worst, R.TOL["softmax"], worst_sum, R.TOL["rowsum_ulp"]))
    assert worst <= R.TOL["softmax"] and worst_sum <= R.TOL["rowsum_ulp"]


@pytest.mark.parametrize("n,d_model", R.SINUSOID_CASES)
def test_fp32_sinusoid_within_one_ulp(n, d_model):
    x, div = R.sinusoid_x(n), R.div_term(d_model)
    assert div.numel() == d_model // 2 and float(div[0]) == 1.0
    if n >= 8:
        assert float(x.max()) == 1e4 and float(x.min()) == -1e4 and bool((x == 0).any()) and bool((x < 0).any())
        assert bool((x == np.float32(866.0254)).any())
    want = R.sinusoid_ref(x, div)
    assert want.shape == (n, d_model)
    half = d_model // 2
    w64 = x.double()[:, None] * div.double()[None, :]
    far = _err(want.reshape(n, half, 2)[..., 0], torch.sin(w64))
    ulps, diff = R.ulp_distance(R.sinusoid32(x, div).numpy(), want.numpy())
    print("sinusoid (%d, %d): fp32 evaluation %.2f ulp, %d of %d entries not bit-equal (bound %d ulp); the fp32 product alone moves "
          "sin by %.1e against exact products" % (n, d_model, ulps, diff, want.numel(), R.TOL["sinusoid_ulp"], far))
    assert ulps <= R.TOL["sinusoid_ulp"]


# ------------------------------------------------------------------------------------------------------- 3. linear attention
def test_focus_conditions_and_fp32():
    scale = R.focus_scale()
    sp = torch.nn.functional.softplus(scale.double())
    assert float(sp.max()) <= R.SOFTPLUS_MAX and float(torch.nn.functional.softplus(torch.tensor(1.0))) <= R.SOFTPLUS_MAX
    tiny = (1e-6 / float(sp.max())) ** 6
    assert tiny >= float(np.finfo(np.float32).tiny), "the square of every cube of an all-non-positive row is a normal fp32 number"
    worst = 0.0
    for rows in R.FOCUS_K_ROWS:
        x = R.focus_rows(rows)
        if rows >= 3:
            assert int((x[1] > 0).sum()) == 1 and not bool((x[2] > 0).any()) and bool(torch.signbit(x[2, 1]))
        want = R.phi64(x, scale)
        worst = max(worst, _err(R.phi32(x, scale), want) / float(want.abs().max()))
    # an all-non-positive row under one scale for all channels: every channel is 1e-6 / softplus(scale)
    u = R.focus_scale(uniform=1.0)
    flat = R.phi64(-R.focus_rows(4).abs(), u)
    assert _err(flat, torch.full_like(flat, 1e-6 / math.log1p(math.e))) <= 1e-20
    worst = max(worst, _err(R.phi32(-R.focus_rows(4).abs(), u), flat) / float(flat.abs().max()))
    print("focus_k: fp32 evaluation %.2e of max |want| (bound %.1e = 8 x the figure measured when written)" % (worst, R.TOL["focus_k"]))
    assert worst <= R.TOL["focus_k"] <= R.LINATTN_CAP
    assert R.TOL["focus_k"] <= 10 * worst, "TOL.focus_k is 8 x the fp32 error measured when written (a quarter more for another CPU)"


def test_focus_q_fp32():
    scale = R.focus_scale()
    worst = 0.0
    for B, rpb in R.FOCUS_Q_CASES:
        q = R.focus_rows(B * rpb, seed=1).reshape(B, rpb, R.C)
        ksum = R.kv64(*R.kv_inputs(B, 33))[1].float().reshape(B, R.C)
        want = R.focus_q64(q, scale, ksum)
        worst = max(worst, _err(R.focus_q32(q, scale, ksum), want) / float(want.abs().max()))
    print("focus_q: fp32 evaluation %.2e of max |want| (bound %.1e)" % (worst, R.TOL["focus_q"]))
    assert worst <= R.TOL["focus_q"] <= R.LINATTN_CAP
    assert R.TOL["focus_q"] <= 10 * worst


def test_kv_fp32_inside_the_derived_bounds():
    worst = [0.0, 0.0]
    for B in R.KV_B:
        for J in R.KV_J:
            k, v = R.kv_inputs(B, J)
            (a64, s64), (a32, s32), (ab, sb) = R.kv64(k, v), R.kv32(k, v), R.kv_bounds(k, v)
            assert bool(((a32.double() - a64).abs() <= ab).all()) and bool(((s32.double() - s64).abs() <= sb).all()), (B, J)
            worst[0] = max(worst[0], float(((a32.double() - a64).abs() / ab).max()))
            if J > 1:
                worst[1] = max(worst[1], float(((s32.double() - s64).abs() / sb).max()))
            else:
                assert torch.equal(s32, k.view(B, R.H, R.D)), "one key: the sum is the key, exactly"
    print("linattn_kv: fp32 evaluation kvT %.3f of its bound, ksum %.3f of its bound" % tuple(worst))


def test_linattn_fp32(sd):
    W = R.layer_weights(sd, DENSE, False)
    scale = R.focus_scale()
    worst = 0.0
    for B, I, J in R.LINATTN_CASES:
        assert I * J * 128 > 64 * 64 * (I + J)
        xq, xm = R.tokens(B, I, 3), R.tokens(B, J, 4)
        want = R.linattn64(xq, xm, xm, W, scale)
        worst = max(worst, _err(R.linattn32(xq, xm, xm, W, scale), want) / float(want.abs().max()))
    print("linear attention forward: fp32 evaluation %.2e of max |want| (bound %.1e)" % (worst, R.TOL["linattn"]))
    assert worst <= R.TOL["linattn"] <= R.LINATTN_CAP
    assert R.TOL["linattn"] <= 10 * worst


# ------------------------------------------------------------------------------------------------------- 4. helpers
def test_helper_restatements():
    p = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    out = R.prepend_bg(p)
    assert out.shape == (2, 3, 3) and (out[:, 0] == 100.0).all() and np.array_equal(out[:, 1:], p)
    x = np.zeros((3, 5), np.float32)
    assert R.rows_equal(x) == 1 and R.rows_equal(x[:1]) == 1
    y = x.copy()
    y[2, 4] = -0.0
    assert R.rows_equal(y) == 0, "+0.0 against -0.0 differ bitwise"
    z = np.full((3, 5), np.nan, np.float32)
    assert R.rows_equal(z) == 1, "an identical NaN payload is equal bitwise"
    z.view(np.int32)[2, 4] ^= 1
    assert R.rows_equal(z) == 0
    assert R.rows_equal(np.zeros((3, 0), np.float32)) == 1


# ------------------------------------------------------------------------------------------------------- 5. row kernels
def test_row_kernel_references():
    g = R.gen(11)
    gam, bet = 1.0 + 0.1 * torch.randn(R.C, generator=g), 0.1 * torch.randn(R.C, generator=g)
    x = torch.randn(5, R.C, generator=g) * 3 + 1
    assert _err(R.layernorm64(x, gam, bet), torch.nn.functional.layer_norm(x.double(), (R.C,), gam.double(), bet.double(), 1e-5)) <= 1e-13
    const = torch.full((1, R.C), 3.7)
    assert torch.equal(R.layernorm64(const, gam, bet)[0], bet.double()), "a constant row: beta exactly"
    big = 1e4 + torch.randn(4, R.C, generator=g)
    e = _err(R.layernorm32(big, gam, bet), R.layernorm64(big, gam, bet))
    print("layernorm on 1e4 + N(0,1): fp32 evaluation %.2e (bound %.1e)" % (e, R.TOL["layernorm"]))
    assert e <= R.TOL["layernorm"]
    e = _err(R.layernorm32(x, gam, bet), R.layernorm64(x, gam, bet))
    print("layernorm on 3 N(0,1) + 1: fp32 evaluation %.2e (bound %.1e)" % (e, R.TOL["layernorm"]))
    assert e <= R.TOL["layernorm"]
    z = torch.zeros(2, R.C)
    assert float(R.l2norm64(z).abs().max()) == 0.0
    small = torch.zeros(1, R.C)
    small[0, 3] = 1e-20
    assert abs(float(R.l2norm64(small)[0, 3]) / (float(np.float32(1e-20)) / 1e-12) - 1.0) <= 1e-12, "a norm of 1e-20 is divided by 1e-12"
    want = R.l2norm64(x)
    e = _err(R.l2norm32(x), want)
    print("l2norm: fp32 evaluation %.2e (bound %.1e)" % (e, R.l2norm_bound(want)))
    assert e <= R.l2norm_bound(want)


@pytest.mark.parametrize("B,N", R.RIGID_CASES)
def test_rigid_inverse_fp32_inside_the_derived_bound(B, N):
    x, Rm, t = R.rigid_inputs(B, N)
    assert _err(Rm.double().transpose(1, 2) @ Rm.double(), torch.eye(3, dtype=torch.float64).expand(B, 3, 3)) <= 1e-6
    want, bound = R.rigid_inverse64(x, Rm, t), R.rigid_bound(x, Rm, t)
    ratio = float(((R.rigid_inverse32(x, Rm, t).double() - want).abs() / bound).max())
    print("rigid inverse (%d, %d): fp32 evaluation %.3f of the bound" % (B, N, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------- 6. composed routes
def test_composed_routes_fp32(sd):
    Wc = R.layer_weights(sd, "coarse_point_matching.transformers.1.layers.1", False)
    Wr = R.layer_weights(sd, "coarse_point_matching.transformers.1.layers.0", True)
    for B, N, M in R.MHA_CASES + [R.MHA_RPE_CASE]:
        rpe = (B, N, M) == R.MHA_RPE_CASE
        xq, xk = R.tokens(B, N, 1), R.tokens(B, M, 2)
        E = R.embedding(B, N, M, 1) if rpe else None
        W = Wr if rpe else Wc
        (h64, p64), (h32, p32) = R.mha64(xq, xk, xk, W, E), R.mha32(xq, xk, xk, W, E)
        eh, ep = _err(h32, h64), _err(p32, p64)
        print("mha (%d,%d,%d)%s: fp32 evaluation hidden %.2e (bound %.1e), probabilities %.2e (bound %.1e)"
              % (B, N, M, " RPE" if rpe else "", eh, R.TOL["mha_hidden"], ep, R.TOL["mha_probs"]))
        assert eh <= R.TOL["mha_hidden"] and ep <= R.TOL["mha_probs"]
    for m in R.CROSS_M:
        x, mem = R.tokens(2, 5, 5), R.tokens(2, m, 6)
        e = _err(R.layer32(x, mem, Wc), R.layer64(x, mem, Wc))
        print("cross layer m %d: fp32 evaluation %.2e (bound %.1e)" % (m, e, R.TOL["layer"]))
        assert e <= R.TOL["layer"]
    for B, n in R.RPE_LAYER_CASES:
        x, E = R.tokens(B, n, 7), R.embedding(B, n, n, 2)
        e = _err(R.layer32(x, x, Wr, E), R.layer64(x, x, Wr, E))
        print("rpe self layer (%d,%d): fp32 evaluation %.2e (bound %.1e)" % (B, n, e, R.TOL["layer"]))
        assert e <= R.TOL["layer"]
