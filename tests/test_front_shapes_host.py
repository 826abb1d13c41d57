"""Host-side proof that the bounds of tests/front_shapes_ref.py are a real constraint and that the inputs are fair: at every case of the
lists a CPU emulation of the kernels' arithmetic (power-of-two scales, fp16 hi + lo, three products, fp32 sums) stays inside the
per-element bound, the same emulation without the activation lo halves leaves it for every output, and the float64 restatements agree
with independent compositions of the same layers.  No GPU, nothing of the product is imported."""
import pytest
import torch

from tests import front_shapes_ref as R

VT_FRONT_CASES = sorted({("unit", Bp * n) for Bp, n, _ in R.VT_CASES})
ALL_FRONT_CASES = R.FRONT_CASES + [c for c in VT_FRONT_CASES if c not in R.FRONT_CASES]
_ids = lambda cases: ["%s-%d" % c for c in cases]


def _ratios(kind, M, drop_lo):
    x, w = R.front_x(kind, M), R.front_weights(kind)
    return R.front_ratios(R.front_emulated(x, w, drop_lo=drop_lo), x, w)


@pytest.mark.parametrize("kind,M", ALL_FRONT_CASES, ids=_ids(ALL_FRONT_CASES))
def test_emulation_inside_the_bound(kind, M):
    """the full emulation: worst |err| / bound <= 1 for qkv, qp and qd -- chained and each fold alone -- with the tightened tau, at
    every case the GPU test runs"""
    r = _ratios(kind, M, drop_lo=False)
    print("emulation %s M=%d: worst |err| / bound  qkv %.3f  qp %.3f  qd %.4f  | folds alone  qp %.3f  qd %.3f" % ((kind, M) + tuple(r)))
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("kind,M", R.FRONT_CASES, ids=_ids(R.FRONT_CASES))
def test_dropped_lo_halves_leave_the_bound(kind, M):
    """the emulation without the activation lo halves exceeds the bound of qkv, and of qp and qd as the folds are checked alone: a
    kernel that silently lost a cross product in any of the three products would fail the GPU test at every one of these cases.  (The
    chained worst-case bounds of qp / qd alone would let it pass: printed, module docstring of front_shapes_ref.)"""
    r = _ratios(kind, M, drop_lo=True)
    print("hi-only activations %s M=%d: worst |err| / bound  qkv %.1f  qp %.1f  qd %.2f  | folds alone  qp %.1f  qd %.1f" % ((kind, M) + tuple(r)))
    assert r[0] > 1.0 and r[3] > 1.0 and r[4] > 1.0, r


def test_zero_token_is_the_bias():
    """the all-zero token of the mixed kind: its emulated qkv row is the bias bit for bit, and its bound is not zero"""
    M = R.FRONT_KIND_M[0]
    x, w = R.front_x("mixed", M), R.front_weights("mixed")
    z, s = R.mixed_special_rows(M)
    assert float(x[z].abs().max()) == 0.0 and int((x[s] != 0).sum()) == 1
    assert torch.equal(R.front_emulated(x, w)[0][z], w.b)
    assert torch.equal(R.front64(x, w)[0][z], w.b.double())
    mags = x.abs().amax(1)
    assert float(mags[mags > 0].max() / mags[mags > 0].min()) > 1e6, "rows of very different magnitude in one call"


@pytest.mark.parametrize("kind", R.FRONT_KINDS)
def test_front64_equals_a_second_composition(kind):
    M = 65
    x, w = R.front_x(kind, M), R.front_weights(kind)
    for a, b, what in zip(R.front64(x, w), R.front64_composed(x, w), ("qkv", "qp", "qd")):
        assert a.shape == b.shape
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-12 * scale, what
    qkv = R.front64(x, w)[0]
    vT = R.vt64(qkv[:60], 3, 20)
    assert vT.shape == (3, 256, 20) and float(vT[2, 7, 11]) == float(qkv[2 * 20 + 11, 512 + 7])


def _block_gpu_dense64(Dn, S, L):
    """the float64 recompute of tests/test_block_gpu.py::test_linattn_layer_vs_oracle_math, as that test states it (rows 1 .. I-1, the
    memory S[:, 1:] projected inside)"""
    d = lambda t: t.double()
    Dt = d(Dn[:, 1:])
    mem = d(S[:, 1:])
    q = Dt @ d(L["q"][0]).t() + d(L["q"][1])
    k = mem @ d(L["kv"][0][:256]).t() + d(L["kv"][1][:256])
    v = mem @ d(L["kv"][0][256:]).t() + d(L["kv"][1][256:])
    sp = torch.nn.functional.softplus(d(L["scale"]))

    def phi(z):
        z = (torch.relu(z) + 1e-6) / sp
        n = z.norm(dim=-1, keepdim=True)
        z3 = z ** 3
        return z3 / z3.norm(dim=-1, keepdim=True) * n
    q, k = phi(q), phi(k)
    hid = torch.zeros_like(q)
    for h in range(4):
        sl = slice(64 * h, 64 * h + 64)
        z = 1.0 / (torch.einsum("bic,bc->bi", q[..., sl], k[..., sl].sum(1)) + 1e-6)
        kvm = torch.einsum("bjc,bjd->bcd", k[..., sl], v[..., sl])
        hid[..., sl] = torch.einsum("bic,bcd,bi->bid", q[..., sl], kvm, z)
    ln = lambda v, gb: torch.nn.functional.layer_norm(v, (256,), d(gb[0]), d(gb[1]), 1e-5)
    y = ln(hid @ d(L["lin"][0]).t() + d(L["lin"][1]) + Dt, L["n1"])
    hh = torch.relu(y @ d(L["exp"][0]).t() + d(L["exp"][1]))
    return ln(hh @ d(L["sq"][0]).t() + d(L["sq"][1]) + y, L["n2"])


@pytest.mark.parametrize("Bp,I,qs", [(2, 2049, 1.0), (3, 300, 1.0), (1, 130, 1.0), (2, 257, 1.0e4), (2, 257, 1.0e-5)])
def test_dense_layer64_equals_the_block_test(Bp, I, qs):
    """R.dense_layer64 (any J, I, row0; the projected kv rows as input) against the restatement of tests/test_block_gpu.py at that
    test's shapes (J = 196, row0 = 1)"""
    g = R.gen(Bp * 1000 + I)
    L = R.dense_weights()
    Dn = torch.randn(Bp, I, 256, generator=g) * qs
    S = torch.randn(Bp, 197, 256, generator=g)
    kv = S[:, 1:].double() @ L["kv"][0].double().t() + L["kv"][1].double()
    a = R.dense_layer64(Dn, kv, L, 1)
    b = _block_gpu_dense64(Dn, S, L)
    assert a.shape == b.shape == (Bp, I - 1, 256)
    assert float((a - b).abs().max()) <= 1e-11


def test_dense_inputs_are_the_rounded_projection():
    L = R.dense_weights()
    for ms in [1.0] + R.DENSE_MEM_SCALES:
        Dn, kv = R.dense_inputs(3, 68, 17, ms)
        assert Dn.shape == (3, 68, 256) and kv.shape == (3, 17, 512) and kv.dtype == torch.float32
        assert bool(torch.isfinite(kv).all()) and 0.1 * ms < float(kv.abs().mean()) < 2.0 * ms + 1.0
        want = R.dense_layer64(Dn, kv, L, 3)
        assert want.shape == (3, 65, 256) and bool(torch.isfinite(want).all())


def test_case_lists_cover_what_the_issue_names():
    """the edges named in the kernels' comments are in the lists: 16-row wave / 64-row workgroup of the front, n above the one-launch
    attention's 208, the 16-key step and 32-key trip of the kv kernel, the dense layer's 64-token workgroup"""
    assert {1, 15, 16, 17, 63, 64, 65, 127, 129, 1000} <= set(R.FRONT_M)
    assert {(1, 1), (3, 5), (2, 50), (5, 64), (2, 209), (1, 260), (3, 211)} <= {(b, n) for b, n, _ in R.VT_CASES}
    assert any(e == 8 for _, _, e in R.VT_CASES) and all(R.ldp_of(n, e) >= n and R.ldp_of(n, e) % 4 == 0 for _, n, e in R.VT_CASES)
    assert {1, 15, 16, 17, 31, 32, 33, 48, 196, 197} <= set(R.KV_J) and set(R.KV_LD) == {512, 516, 768}
    assert set(R.DENSE_J) == {1, 17, 33, 196} and set(R.DENSE_ROWS) == {1, 63, 64, 65, 130} and set(R.DENSE_ROW0) == {0, 1, 3}
