"""The launch-per-op layer under the fused kernels, off the golden shape: both kernels behind sam6d_attention, sam6d_scaled_softmax,
sam6d_sinusoid_embed, the three kernels of csrc/linattn.hip, sam6d_transpose, the row helpers at the end of csrc/pe.hip,
sam6d_layernorm256 / sam6d_l2norm256 and the unfused routes of pem.py composed of them -- what matmul mode 0, the fused_* switches off,
the drop-in sub-modules and cross_layer beyond the fused kernel's range run, and what the fused-vs-unfused tests take as their yardstick.
Every entry point is called through the C ABI (or its pem wrapper) at batch sizes above one, at lengths on both sides of every tile,
wave and loop boundary of its kernel and with strided layouts, against the float64 restatements of tests/attn_shapes_ref.py; every row is
compared.  tests/test_attn_shapes_host.py proves the builders' conditions and that an fp32 CPU evaluation alone meets each bound of
R.TOL.  Every device tensor is named, so that no temporary dies before its launch; every output is pre-filled with NaN."""
import numpy as np
import pytest
import torch

from tests import attn_shapes_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
C = R.C


@pytest.fixture(scope="module")
def sd():
    from sam6d_hip import synth
    return synth.make_pem_weights(1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from sam6d_hip import _lib
    _lib.call(name, *args)


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _maxerr(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite values"
    return float((got - want).abs().max()) if got.numel() else 0.0


def _bits(x):
    return torch.as_tensor(x).contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _all_nan(x):
    return bool(torch.isnan(x).all())


# ------------------------------------------------------------------------------------------------------- 1. sam6d_attention
def _attention(dev, t, layout="sep"):
    """sam6d_attention on the inputs t (R.attn_inputs) -> out (B,n,256) on the CPU.
    sep:    q, k, v, out in four contiguous buffers
    qkv768: q | k | v as column blocks of one (B,n,768) buffer (rpe_self_layer's call)
    kv512:  q alone, k | v in one (B,m,512) buffer (cross_layer's call)
    wide:   out rows 260 floats apart and clouds n 260 + 8 floats apart in a NaN-filled buffer: every float outside the (n,256) blocks
            must still be NaN afterwards"""
    B, n, _ = t.q.shape
    m = t.k.shape[1]
    qp_d = t.qp.to(dev) if t.qp is not None else None
    E_d = t.E.to(dev) if t.E is not None else None
    if layout == "qkv768":
        assert n == m
        buf_d = torch.cat([t.q, t.k, t.v], 2).contiguous().to(dev)
        ptr = (_p(buf_d), _p(buf_d, C), _p(buf_d, 2 * C))
        ld, st = (3 * C,) * 3, (n * 3 * C,) * 3
    elif layout == "kv512":
        q_d, kv_d = t.q.to(dev), torch.cat([t.k, t.v], 2).contiguous().to(dev)
        ptr = (_p(q_d), _p(kv_d), _p(kv_d, C))
        ld, st = (C, 2 * C, 2 * C), (n * C, m * 2 * C, m * 2 * C)
    else:
        q_d, k_d, v_d = t.q.to(dev), t.k.to(dev), t.v.to(dev)
        ptr = (_p(q_d), _p(k_d), _p(v_d))
        ld, st = (C,) * 3, (n * C, m * C, m * C)
    ldo, so = (260, n * 260 + 8) if layout == "wide" else (C, n * C)
    out_d = torch.full((B, so), NAN, device=dev)
    _call("sam6d_attention", *ptr, _p(qp_d) if qp_d is not None else None, _p(E_d) if E_d is not None else None, _p(out_d), B, n, m,
          *ld, ldo, *st, so, _stream())
    torch.cuda.synchronize()
    out = out_d.cpu()
    rows = out[:, :n * ldo].reshape(B, n, ldo)
    if layout == "wide":
        assert _all_nan(rows[:, :, C:]) and _all_nan(out[:, n * ldo:]), "floats outside the (n,256) blocks of the wide buffer were written"
    return rows[:, :, :C].contiguous()


def _layouts(rpe, shape):
    return ["sep"] + [name for name, per_route in R.LAYOUT_SHAPES.items() if shape in per_route[rpe]]


ATTN_CASES = [(False, s) for s in R.PLAIN_SHAPES] + [(True, s) for s in R.RPE_SHAPES]


@pytest.mark.parametrize("rpe,shape", ATTN_CASES, ids=["%s-%d-%d-%d" % (("rpe" if r else "plain",) + s) for r, s in ATTN_CASES])
def test_attention_vs_float64(dev, rpe, shape):
    """attention_mq_kernel<4> (plain) / attention_kernel<true> (RPE) against float64 on every input kind: m below one key per wave, on
    every tail of the 4 / 8 / 16-key loops, on both sides of the 64-lane softmax trip and at the LDS bound, n % 4 != 0 and n > 256.  A
    single key gives the v row bit for bit; a dominant key its v row and bitwise equal keys the column mean of v within the bound; the
    large-logit inputs would overflow exp without the max subtraction."""
    B, n, m = shape
    for kind in R.ATTN_KINDS:
        t = R.attn_inputs(kind, B, n, m, rpe)
        want = R.attention64(t.q, t.k, t.v, t.qp, t.E)[0]
        bound = R.rel_bound(want, R.TOL["attn"])
        for layout in _layouts(rpe, shape):
            got = _attention(dev, t, layout)
            e = _maxerr(got, want)
            print("attention %s %s %s %s: max error %.2e / bound %.2e" % ("rpe" if rpe else "plain", shape, kind, layout, e, bound))
            assert e <= bound
            if m == 1:
                assert _same_bits(got, t.v.expand(B, n, C)), "one key: the probability is exactly 1 and the output the v row bit for bit"
            if kind in ("dominant", "large"):
                vrow = torch.gather(t.v, 1, R.lead_key(B, n, m)[:, :, None].expand(B, n, C))
                assert _maxerr(got, vrow) <= bound, "the output is the dominant key's v row"
            if kind == "equal":
                assert _maxerr(got, t.v.double().mean(1, keepdim=True).expand(B, n, C)) <= bound, "equal keys: the column mean of v"


@pytest.mark.parametrize("rpe", [False, True])
@pytest.mark.parametrize("shape", R.INDEPENDENCE_SHAPES)
def test_attention_batch_independence(dev, shape, rpe):
    """the result of B = 3 clouds equals three calls of one cloud bit for bit: the per-batch strides sq / sk / sv / so reach no other cloud"""
    B, n, m = shape
    t = R.attn_inputs("random", B, n, m, rpe)
    whole = _attention(dev, t)
    for b in range(B):
        one = R.types.SimpleNamespace(**{k: (None if v is None else v[b:b + 1].contiguous()) for k, v in vars(t).items()})
        assert _same_bits(_attention(dev, one), whole[b:b + 1]), "cloud %d of %s" % (b, shape)


def test_attention_refusals(dev):
    """m = 257 and m = 0, a stride that is no multiple of 4 floats, qp without E and E without qp: RuntimeError before any launch, the
    NaN-filled output untouched"""
    B, n = 1, 4
    g = R.gen(1)
    q_d, k_d, v_d = (torch.randn(B, 260, C, generator=g).to(dev) for _ in range(3))
    qp_d, E_d = torch.randn(B, n, R.H, C, generator=g).to(dev), torch.randn(B, n, 8, C, generator=g).to(dev)
    out_d = torch.full((B, n, 260), NAN, device=dev)

    def run(m, qp, E, ldq=C, so=n * 260):
        _call("sam6d_attention", _p(q_d), _p(k_d), _p(v_d), qp, E, _p(out_d), B, n, m, ldq, C, C, 260, n * C, 260 * C, 260 * C, so, _stream())

    for kw in (dict(m=257, qp=None, E=None), dict(m=0, qp=None, E=None), dict(m=8, qp=None, E=None, ldq=258),
               dict(m=8, qp=None, E=None, so=n * 260 + 2), dict(m=8, qp=_p(qp_d), E=None), dict(m=8, qp=None, E=_p(E_d)),
               dict(m=257, qp=_p(qp_d), E=_p(E_d))):
        with pytest.raises(RuntimeError):
            run(**kw)
    torch.cuda.synchronize()
    assert _all_nan(out_d)
    run(m=8, qp=_p(qp_d), E=_p(E_d))  # the same buffers with valid arguments are served
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_d[:, :, :C]).all()) and _all_nan(out_d[:, :, C:])


# ------------------------------------------------------------------------------------------------------- 2. softmax, sinusoid
@pytest.mark.parametrize("n", R.SOFTMAX_N)
def test_scaled_softmax_vs_float64(dev, n):
    """rows on both sides of the four rows of a workgroup, n on both sides of the 64-lane trip, b NULL and given, both scales, every
    leading dimension larger than n: input padding of 1e30 is never read as a key, output padding stays NaN, rows sum to 1 within 4 ulp"""
    lda, ldb, ldo = n + 3, n + 5, n + 1
    for rows in R.SOFTMAX_ROWS:
        a, b = R.softmax_inputs(rows, n)
        a_pad, b_pad = torch.full((rows, lda), 1e30), torch.full((rows, ldb), 1e30)
        a_pad[:, :n], b_pad[:, :n] = a, b
        a_d, b_d = a_pad.to(dev), b_pad.to(dev)
        for bb in (None, b):
            for scale in R.SOFTMAX_SCALES:
                out_d = torch.full((rows, ldo), NAN, device=dev)
                _call("sam6d_scaled_softmax", _p(a_d), _p(b_d) if bb is not None else None, scale, rows, n, lda, ldb, _p(out_d), ldo, _stream())
                torch.cuda.synchronize()
                out = out_d.cpu()
                assert _all_nan(out[:, n:]), "output padding written"
                e = _maxerr(out[:, :n], R.softmax64(a, bb, scale))
                s = float((out[:, :n].double().sum(1) - 1.0).abs().max()) / R.ULP1
                print("softmax rows %d n %d b %s scale %g: max error %.2e / bound %.1e; row sums off by %.2f ulp / bound %d"
                      % (rows, n, bb is not None, scale, e, R.TOL["softmax"], s, R.TOL["rowsum_ulp"]))
                assert e <= R.TOL["softmax"] and s <= R.TOL["rowsum_ulp"]


@pytest.mark.parametrize("n,d_model", R.SINUSOID_CASES)
def test_sinusoid_embed_within_one_ulp(dev, n, d_model):
    """arguments that are zero, negative, 866 (the bg point's index) and up to +-1e4: every entry within 1 fp32 ulp of the float64 sin /
    cos of the fp32 product rounded once (the kernel is written to do exactly this); nothing written past the n rows"""
    x, div = R.sinusoid_x(n), R.div_term(d_model)
    x_d, div_d = x.to(dev), div.to(dev)
    out_d = torch.full((n * d_model + 8,), NAN, device=dev)
    _call("sam6d_sinusoid_embed", _p(x_d), n, _p(div_d), d_model, _p(out_d), _stream())
    torch.cuda.synchronize()
    out = out_d.cpu()
    assert _all_nan(out[n * d_model:])
    got = out[:n * d_model].reshape(n, d_model)
    assert torch.isfinite(got).all()
    ulps, diff = R.ulp_distance(got.numpy(), R.sinusoid_ref(x, div).numpy())
    print("sinusoid (%d, %d): %.2f ulp, %d of %d entries not bit-equal / bound %d ulp" % (n, d_model, ulps, diff, got.numel(), R.TOL["sinusoid_ulp"]))
    assert ulps <= R.TOL["sinusoid_ulp"]


# ------------------------------------------------------------------------------------------------------- 3. linattn.hip
@pytest.mark.parametrize("ld", R.FOCUS_LD)
def test_linattn_focus_k_vs_float64(dev, ld):
    """phi in place on rows ld floats apart: random rows, rows with one positive channel and rows with none, on both sides of the four
    rows of a workgroup; the columns from 256 on (the v half at ld = 512) keep their bits.  Under one scale for all channels an
    all-non-positive row becomes 1e-6 / softplus(scale) in every channel."""
    scale = R.focus_scale()
    cases = [(rows, R.focus_rows(rows), scale) for rows in R.FOCUS_K_ROWS] + [(4, -R.focus_rows(4).abs(), R.focus_scale(uniform=1.0))]
    for rows, x, sc in cases:
        buf = torch.randn(rows, ld, generator=R.gen(rows + ld))
        buf[:, :C] = x
        buf_d, sc_d = buf.to(dev), sc.to(dev)
        _call("sam6d_linattn_focus_k", _p(buf_d), _p(sc_d), rows, ld, _stream())
        torch.cuda.synchronize()
        got = buf_d.cpu()
        assert _same_bits(got[:, C:], buf[:, C:]), "columns beyond 256 changed"
        want = R.phi64(x, sc)
        e = _maxerr(got[:, :C], want) / float(want.abs().max())
        print("focus_k rows %d ld %d%s: max error %.2e of max |want| / bound %.1e" % (rows, ld, " (uniform scale)" if sc is not scale else "", e, R.TOL["focus_k"]))
        assert e <= R.TOL["focus_k"]
        if sc is not scale:
            flat = 1e-6 / float(torch.nn.functional.softplus(torch.tensor(1.0, dtype=torch.float64)))
            assert _maxerr(got[:, :C], torch.full((rows, C), flat, dtype=torch.float64)) <= R.TOL["focus_k"] * flat


@pytest.mark.parametrize("B", R.KV_B)
@pytest.mark.parametrize("J", R.KV_J)
def test_linattn_kv_vs_float64(dev, J, B):
    """kv^T and the key sums on both sides of the 32-key LDS tile, entry by entry inside the derived bounds: k | v as halves of one
    (B,J,512) buffer (pem's call), and as two buffers of ld 256 whose clouds are further apart than J ld"""
    k, v = R.kv_inputs(B, J)
    (a64, s64), (ab, sb) = R.kv64(k, v), R.kv_bounds(k, v)
    kv_d = torch.cat([k, v], 2).contiguous().to(dev)
    sk, sv = J * C + 12, J * C + 20
    k_d, v_d = torch.full((B, sk), 1e30, device=dev), torch.full((B, sv), 1e30, device=dev)
    k_d[:, :J * C], v_d[:, :J * C] = k.reshape(B, -1).to(dev), v.reshape(B, -1).to(dev)
    for what, args in (("halves", (_p(kv_d), _p(kv_d, C), B, J, 2 * C, 2 * C, J * 2 * C, J * 2 * C)),
                       ("separate", (_p(k_d), _p(v_d), B, J, C, C, sk, sv))):
        kvT_d, ksum_d = torch.full((B * R.H * 4096 + 64,), NAN, device=dev), torch.full((B * C + 64,), NAN, device=dev)
        _call("sam6d_linattn_kv", *args, _p(kvT_d), _p(ksum_d), _stream())
        torch.cuda.synchronize()
        kvT, ksum = kvT_d.cpu(), ksum_d.cpu()
        assert _all_nan(kvT[B * R.H * 4096:]) and _all_nan(ksum[B * C:])
        kvT, ksum = kvT[:B * R.H * 4096].reshape(B, R.H, 64, 64), ksum[:B * C].reshape(B, R.H, 64)
        assert torch.isfinite(kvT).all() and torch.isfinite(ksum).all()
        ea, es = (kvT.double() - a64).abs(), (ksum.double() - s64).abs()
        ra = float((ea / ab).max())
        rs = float((es / sb).max()) if J > 1 else 0.0
        print("linattn_kv B %d J %d %s: kvT %.3f of its bound (max error %.2e), ksum %.3f of its bound (max error %.2e) / bound 1"
              % (B, J, what, ra, float(ea.max()), rs, float(es.max())))
        assert bool((ea <= ab).all()) and bool((es <= sb).all())


@pytest.mark.parametrize("ld", R.FOCUS_Q_LD)
@pytest.mark.parametrize("B,rpb", R.FOCUS_Q_CASES)
def test_linattn_focus_q_vs_float64(dev, B, rpb, ld):
    """phi and the per-head z scaling in place: batch boundaries inside a workgroup of four rows ((3,5)), and 16389 rows -- 4098
    workgroups' worth for a grid capped at 4096, so the grid-stride loop takes a second trip; padding columns keep their bits"""
    scale = R.focus_scale()
    q = R.focus_rows(B * rpb, seed=1).reshape(B, rpb, C)
    ksum = R.kv64(*R.kv_inputs(B, 33))[1].float().reshape(B, C).contiguous()
    buf = torch.full((B * rpb, ld), -3.0)
    buf[:, :C] = q.reshape(-1, C)
    buf_d, sc_d, ks_d = buf.to(dev), scale.to(dev), ksum.to(dev)
    _call("sam6d_linattn_focus_q", _p(buf_d), _p(sc_d), _p(ks_d), B, rpb, ld, _stream())
    torch.cuda.synchronize()
    got = buf_d.cpu()
    assert bool((got[:, C:] == -3.0).all()), "padding columns changed"
    want = R.focus_q64(q, scale, ksum).reshape(-1, C)
    e = _maxerr(got[:, :C], want) / float(want.abs().max())
    print("focus_q B %d rows %d ld %d: max error %.2e of max |want| / bound %.1e" % (B, rpb, ld, e, R.TOL["focus_q"]))
    assert e <= R.TOL["focus_q"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,I,J", R.LINATTN_CASES)
def test_linear_attention_forward_vs_float64(dev, sd, B, I, J, mode):
    """pem.linear_attention_forward: the three projections, focus_k, kv, focus_q and the four per-head contractions, every row, in both
    matmul modes.  (In mode 1 the contractions ran on the fp16 split and were off by 1.35e-5 at (2,300,197) -- rows of phi(q) z sit at
    the lower end of the split's range, see pem._linattn_contract, which now runs them on the exact loop: 7.8e-7.)"""
    from sam6d_hip import pem
    W = R.layer_weights(sd, "fine_point_matching.transformers.0.dense_layer", False)
    lq, lk, lv = (pem.Linear(W[k][0].to(dev), W[k][1].to(dev)) for k in "qkv")
    scale = R.focus_scale()
    xq, xm = R.tokens(B, I, 3), R.tokens(B, J, 4)
    xq_d, xm_d, sc_d = xq.to(dev), xm.to(dev), scale.to(dev)
    got = pem.linear_attention_forward(xq_d, xm_d, xm_d, lq, lk, lv, sc_d, options=pem.Options(matmul_mode=mode))
    torch.cuda.synchronize()
    want = R.linattn64(xq, xm, xm, W, scale)
    e = _maxerr(got, want) / float(want.abs().max())
    print("linear_attention_forward (%d,%d,%d) mode %d: max error %.2e of max |want| / bound %.1e" % (B, I, J, mode, e, R.TOL["linattn"]))
    assert e <= R.TOL["linattn"]


# ------------------------------------------------------------------------------------------------------- 4. bit-exact helpers
def _transpose(dev, src, B, n, ncol, ld_src, off, ld_dst):
    """dst[b][c][j] = src[b][j][off + c] -> the whole NaN-prefilled destination (B, ncol, ld_dst) on the CPU"""
    src_d = src.to(dev)
    dst_d = torch.full((B, ncol, ld_dst), NAN, device=dev)
    _call("sam6d_transpose", _p(src_d, off), ld_src, n * ld_src, B, n, ncol, _p(dst_d), ld_dst, ncol * ld_dst, _stream())
    torch.cuda.synchronize()
    return dst_d.cpu()


@pytest.mark.parametrize("B,n,ncol", R.TRANSPOSE_SHAPES)
def test_transpose_tile_edges(dev, B, n, ncol):
    src = torch.randn(B, n, ncol, generator=R.gen(B + n + ncol))
    for ld_dst in (n, n + 3):
        dst = _transpose(dev, src, B, n, ncol, ncol, 0, ld_dst)
        assert np.array_equal(dst[:, :, :n].numpy(), src.numpy().transpose(0, 2, 1)) and _all_nan(dst[:, :, n:])


def test_transpose_strided_pem_call(dev):
    """the v block of a (2,197,768) q | k | v buffer into rows of ld 200 (rpe_self_layer's call): the destination padding stays NaN"""
    B, n = 2, 197
    src = torch.randn(B, n, 3 * C, generator=R.gen(9))
    dst = _transpose(dev, src, B, n, C, 3 * C, 2 * C, 200)
    assert np.array_equal(dst[:, :, :n].numpy(), src[:, :, 2 * C:].numpy().transpose(0, 2, 1)) and _all_nan(dst[:, :, n:])


@pytest.mark.parametrize("Cc", [4, 256])
def test_put_rows(dev, Cc):
    """one bg row broadcast over B = 3 (s_src_b = 0), a block copy into a larger buffer at a row offset with a wider row stride, and
    rows = 0 as a no-op: every float outside the target keeps its bits"""
    g = R.gen(Cc)
    B, R0, ldd = 3, 6, Cc + 4
    bg = torch.randn(1, Cc, generator=g)
    dst = torch.randn(B, R0, ldd, generator=g)
    bg_d, dst_d = bg.to(dev), dst.to(dev)
    _call("sam6d_put_rows", _p(bg_d), 0, Cc, _p(dst_d, 2 * ldd), R0 * ldd, ldd, B, 1, Cc, _stream())
    want = dst.clone()
    want[:, 2, :Cc] = bg
    torch.cuda.synchronize()
    assert _same_bits(dst_d, want)
    rows = 3
    src = torch.randn(B, rows + 1, Cc, generator=g)  # clouds of the source a row further apart than they are long
    src_d = src.to(dev)
    _call("sam6d_put_rows", _p(src_d), (rows + 1) * Cc, Cc, _p(dst_d, 3 * ldd), R0 * ldd, ldd, B, rows, Cc, _stream())
    want[:, 3:3 + rows, :Cc] = src[:, :rows]
    torch.cuda.synchronize()
    assert _same_bits(dst_d, want)
    _call("sam6d_put_rows", _p(src_d), (rows + 1) * Cc, Cc, _p(dst_d), R0 * ldd, ldd, B, 0, Cc, _stream())
    torch.cuda.synchronize()
    assert _same_bits(dst_d, want)


@pytest.mark.parametrize("B,n", [(1, 1), (3, 196), (2, 2048)])
def test_prepend_bg_point(dev, B, n):
    pts = torch.randn(B, n, 3, generator=R.gen(B + n))
    pts_d = pts.to(dev)
    out_d = torch.full((B * (n + 1) * 3 + 4,), NAN, device=dev)
    _call("sam6d_prepend_bg_point", _p(pts_d), B, n, _p(out_d), _stream())
    torch.cuda.synchronize()
    out = out_d.cpu()
    assert np.array_equal(out[:-4].reshape(B, n + 1, 3).numpy(), R.prepend_bg(pts.numpy())) and _all_nan(out[-4:])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_add_scalar(dev, n):
    """y = x + 1e-8f in fp32 (the ball query's new_xyz): values it changes (0, +-1e-8, 1e-7) and values it leaves alone"""
    x = torch.randn(n, generator=R.gen(n))
    x[::5] = torch.tensor([0.0, 1e-8, -1e-8, 1e-7, -0.0]).repeat(n)[:x[::5].numel()]
    x_d = x.to(dev)
    y_d = torch.full((n + 4,), NAN, device=dev)
    _call("sam6d_add_scalar", _p(x_d), 1e-8, n, _p(y_d), _stream())
    torch.cuda.synchronize()
    y = y_d.cpu()
    assert np.array_equal(y[:n].numpy(), x.numpy() + np.float32(1e-8)) and _all_nan(y[n:])


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_copy_f32(dev, n):
    src = torch.randn(max(n, 1), generator=R.gen(n))
    src_d = src.to(dev)
    dst_d = torch.full((n + 4,), NAN, device=dev)
    _call("sam6d_copy_f32", _p(src_d), _p(dst_d), n, _stream())
    torch.cuda.synchronize()
    dst = dst_d.cpu()
    assert _same_bits(dst[:n], src[:n]) and _all_nan(dst[n:])


def _rows_equal(dev, x):
    B = x.shape[0]
    x_d = x.contiguous().to(dev) if x.numel() else torch.zeros(4, device=dev)
    flag_d = torch.full((2,), -9, dtype=torch.int32, device=dev)
    _call("sam6d_batch_rows_equal", _p(x_d), B, x[0].numel(), flag_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    flag = flag_d.cpu()
    assert int(flag[1]) == -9
    assert int(flag[0]) == R.rows_equal(x.numpy()), "differs from the numpy restatement"
    return int(flag[0])


@pytest.mark.parametrize("n", [0, 1, 257])
def test_batch_rows_equal(dev, n):
    """one cloud and three equal copies give 1; one flipped mantissa bit in the last element of the last copy, and +0.0 against -0.0,
    give 0; an identical NaN payload gives 1 (the comparison is bitwise)"""
    row = torch.randn(1, n, generator=R.gen(n))
    assert _rows_equal(dev, row) == 1
    same = row.repeat(3, 1)
    assert _rows_equal(dev, same) == 1
    if n == 0:
        return
    flipped = same.clone()
    flipped.view(torch.int32)[2, n - 1] ^= 1
    assert _rows_equal(dev, flipped) == 0
    zeros = torch.zeros(3, n)
    zeros[2, n - 1] = -0.0
    assert _rows_equal(dev, zeros) == 0
    nans = same.clone()
    nans[:, n - 1] = NAN
    assert _rows_equal(dev, nans) == 1


# ------------------------------------------------------------------------------------------------------- 5. row kernels
def _rows_call(dev, name, x, ldx, ldy, extra=(), tail=(), inplace=False):
    """a (rows,256) -> (rows,256) row kernel on rows ldx / ldy floats apart -> the output rows; output padding must stay NaN"""
    rows = x.shape[0]
    xb = torch.full((rows, ldx), 1e30)
    xb[:, :C] = x
    x_d = xb.to(dev)
    y_d = x_d if inplace else torch.full((rows, ldy), NAN, device=dev)
    _call(name, _p(x_d), *extra, _p(y_d), rows, ldx, ldy, *tail, _stream())
    torch.cuda.synchronize()
    y = y_d.cpu()
    assert bool((y[:, C:] == 1e30).all()) if inplace else _all_nan(y[:, C:]), "padding written"
    return y[:, :C]


@pytest.mark.parametrize("rows", R.ROW_COUNTS)
def test_layernorm256_rows(dev, rows):
    """rows on both sides of the four rows of a workgroup, ldx != ldy (768 -> 256, 256 -> 260), then the two special rows: a constant row
    returns beta exactly, and a row of 1e4 + N(0,1) stays within the project's 2e-5 -- the kernel sums the row minus its first element;
    summed as it stands, the mean of 256 values near 1e4 is misplaced by up to 1.9e-3 of the row's standard deviation (fp32, measured
    on the CPU)."""
    g = R.gen(50 + rows)
    gam, bet = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    special = torch.stack([torch.full((C,), 3.7), 1e4 + torch.randn(C, generator=g)])
    gam_d, bet_d = gam.to(dev), bet.to(dev)
    for ldx, ldy in ((768, 256), (256, 260)):
        got = _rows_call(dev, "sam6d_layernorm256", x, ldx, ldy, extra=(_p(gam_d), _p(bet_d)), tail=(1e-5,))
        sp = _rows_call(dev, "sam6d_layernorm256", special, ldx, ldy, extra=(_p(gam_d), _p(bet_d)), tail=(1e-5,))
        assert _same_bits(sp[0], bet), "a constant row returns beta exactly"
        e, e_far = _maxerr(got, R.layernorm64(x, gam, bet)), _maxerr(sp[1], R.layernorm64(special, gam, bet)[1])
        print("layernorm256 rows %d ld %d -> %d: max error %.2e, on 1e4 + N(0,1) %.2e / bound %.1e" % (rows, ldx, ldy, e, e_far, R.TOL["layernorm"]))
        assert e <= R.TOL["layernorm"] and e_far <= R.TOL["layernorm"]


@pytest.mark.parametrize("rows", R.ROW_COUNTS)
def test_l2norm256_rows(dev, rows):
    """ldx != ldy and in place; then the two special rows: a zero row returns zeros, a row of norm 1e-20 is divided by 1e-12"""
    x = torch.randn(rows, C, generator=R.gen(60 + rows)) * 3 + 1
    special = torch.zeros(2, C)
    special[1, 3] = 1e-20
    want, want_small = R.l2norm64(x), float(R.l2norm64(special)[1, 3])
    for ldx, ldy, inplace in ((768, 256, False), (256, 260, False), (260, 260, True)):
        got = _rows_call(dev, "sam6d_l2norm256", x, ldx, ldy, inplace=inplace)
        sp = _rows_call(dev, "sam6d_l2norm256", special, ldx, ldy, inplace=inplace)
        assert float(sp[0].abs().max()) == 0.0, "a zero row returns zeros"
        assert abs(float(sp[1, 3]) / want_small - 1.0) <= 1e-6 and float(sp[1].abs().sum()) == float(sp[1, 3]), "1e-20 / 1e-12"
        e = _maxerr(got, want)
        print("l2norm256 rows %d ld %d -> %d%s: max error %.2e / bound %.2e" % (rows, ldx, ldy, " in place" if inplace else "", e, R.l2norm_bound(want)))
        assert e <= R.l2norm_bound(want)


@pytest.mark.parametrize("B,N", R.RIGID_CASES)
def test_rigid_inverse_inside_the_derived_bound(dev, B, N):
    """y = (x - t) @ R per cloud, entry by entry inside 5 x 2^-24 sum_k |d_k| |R_kj| (R.rigid_bound derives it); 257 points put a cloud
    boundary inside a workgroup of 256"""
    x, Rm, t = R.rigid_inputs(B, N)
    x_d, R_d, t_d = x.to(dev), Rm.to(dev), t.to(dev)
    y_d = torch.full((B * N * 3 + 4,), NAN, device=dev)
    _call("sam6d_rigid_inverse", _p(x_d), _p(R_d), _p(t_d), B, N, _p(y_d), _stream())
    torch.cuda.synchronize()
    y = y_d.cpu()
    assert _all_nan(y[B * N * 3:])
    got = y[:B * N * 3].reshape(B, N, 3)
    assert torch.isfinite(got).all()
    err, bound = (got.double() - R.rigid_inverse64(x, Rm, t)).abs(), R.rigid_bound(x, Rm, t)
    print("rigid_inverse (%d, %d): %.3f of the bound (max error %.2e) / bound 1" % (B, N, float((err / bound).max()), float(err.max())))
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------------- 6. composed unfused routes
COARSE1 = "coarse_point_matching.transformers.1"


@pytest.fixture(scope="module")
def layers(sd, dev):
    from sam6d_hip import pem
    T = pem.pack_geo_transformer(sd, dev, COARSE1)
    torch.cuda.synchronize()
    return T


def _linears(W, dev, keys):
    from sam6d_hip import pem
    return [pem.Linear(W[k][0].to(dev), W[k][1].to(dev)) for k in keys]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,N,M", R.MHA_CASES + [R.MHA_RPE_CASE])
def test_mha_forward_vs_float64(dev, sd, B, N, M, mode):
    """pem.mha_forward -- the q.k^T GEMM, sam6d_scaled_softmax, sam6d_transpose and the P.v GEMM -- hidden states and probabilities of
    every row; (2,6,9) with embed_qk and proj_p (the RPE term as a second score tensor)"""
    from sam6d_hip import pem
    rpe = (B, N, M) == R.MHA_RPE_CASE
    W = R.layer_weights(sd, COARSE1 + (".layers.0" if rpe else ".layers.1"), rpe)
    xq, xk = R.tokens(B, N, 1), R.tokens(B, M, 2)
    E = R.embedding(B, N, M, 1) if rpe else None
    lq, lk, lv = _linears(W, dev, "qkv")
    lp = _linears(W, dev, "p")[0] if rpe else None
    xq_d, xk_d = xq.to(dev), xk.to(dev)
    E_d = E.to(dev) if rpe else None
    hid, probs = pem.mha_forward(xq_d, xk_d, xk_d, lq, lk, lv, embed_qk=E_d, proj_p=lp, options=pem.Options(matmul_mode=mode))
    torch.cuda.synchronize()
    h64, p64 = R.mha64(xq, xk, xk, W, E)
    eh, ep = _maxerr(hid, h64), _maxerr(probs, p64)
    print("mha_forward (%d,%d,%d)%s mode %d: hidden %.2e / bound %.1e, probabilities %.2e / bound %.1e"
          % (B, N, M, " RPE" if rpe else "", mode, eh, R.TOL["mha_hidden"], ep, R.TOL["mha_probs"]))
    assert eh <= R.TOL["mha_hidden"] and ep <= R.TOL["mha_probs"]
    assert float((probs.double().sum(3) - 1.0).abs().max()) <= R.TOL["rowsum_ulp"] * R.ULP1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("m", R.CROSS_M)
def test_cross_layer_past_the_fused_range(dev, sd, layers, m, mode):
    """pem.cross_layer at m = 209 and m = 256, the first and the last memory length it hands to sam6d_attention, every row against float64"""
    from sam6d_hip import pem
    W = R.layer_weights(sd, COARSE1 + ".layers.1", False)
    x, mem = R.tokens(2, 5, 5), R.tokens(2, m, 6)
    x_d, mem_d = x.to(dev), mem.to(dev)
    got = pem.on_tensor_device(pem.cross_layer)(x_d, mem_d, layers["cross"], options=pem.Options(matmul_mode=mode))
    torch.cuda.synchronize()
    e = _maxerr(got, R.layer64(x, mem, W))
    print("cross_layer m %d mode %d: max error %.2e / bound %.1e" % (m, mode, e, R.TOL["layer"]))
    assert e <= R.TOL["layer"]


@pytest.mark.parametrize("mode", [0, 1])
def test_cross_layer_refuses_257_keys(dev, layers, mode):
    """m = 257 is beyond sam6d_attention's LDS rows: RuntimeError, and the caller's output view keeps its NaN"""
    from sam6d_hip import pem
    x_d, mem_d = R.tokens(2, 5, 5).to(dev), R.tokens(2, 257, 6).to(dev)
    out_d = torch.full((2, 5, C), NAN, device=dev)
    with pytest.raises(RuntimeError):
        pem.on_tensor_device(pem.cross_layer)(x_d, mem_d, layers["cross"], out=out_d, options=pem.Options(matmul_mode=mode))
    torch.cuda.synchronize()
    assert _all_nan(out_d)


@pytest.mark.parametrize("B,n", R.RPE_LAYER_CASES)
def test_rpe_self_layer_materialised_vs_float64(dev, sd, layers, B, n):
    """pem.rpe_self_layer with the (B,n,n,256) embedding tensor given (attention_kernel<true> on the q | k | v buffer), every row"""
    from sam6d_hip import pem
    W = R.layer_weights(sd, COARSE1 + ".layers.0", True)
    x, E = R.tokens(B, n, 7), R.embedding(B, n, n, 2)
    x_d, E_d = x.to(dev), E.to(dev)
    got = pem.rpe_self_layer(x_d, E_d, layers["self"])
    torch.cuda.synchronize()
    e = _maxerr(got, R.layer64(x, x, W, E))
    print("rpe_self_layer (%d,%d): max error %.2e / bound %.1e" % (B, n, e, R.TOL["layer"]))
    assert e <= R.TOL["layer"]
