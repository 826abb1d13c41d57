"""The fused fronts of csrc/block.hip off their one shape: rpe_front_kernel (sam6d_rpe_front, sam6d_rpe_front_vt) against float64 per
element with the chained split-product bound of tests/front_shapes_ref.py, at every tile edge of the 16-row wave and the 64-row
workgroup, with rows, weights and biases of very different magnitude; tb_kv_fused_kernel (sam6d_linattn_kv_image) bit for bit against
the three launches it replaced at every edge of its 16-key step and 32-key trip, with padded rows and gaps between the clouds; and
sam6d_linattn_kv_image + sam6d_linattn_layer called directly against float64 at short memories, at the edges of the 64-token workgroup
and with row0 = 0, 1, 3.  Every kernel is called through the C ABI.  Every output sits in a NaN-filled buffer with guard rows before
and after it; whatever a call must not write is asserted bit for bit untouched.  tests/test_front_shapes_host.py proves on the CPU
that the bounds hold for the kernels' arithmetic and fail without the lo halves.  Every device tensor is named, so that no temporary
dies before its launch."""
import functools

import pytest
import torch

from tests import front_shapes_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
C = R.C
GUARD = 2  # guard rows on either side of every output


def _lib():
    from sam6d_hip import _lib as L
    return L


def _call(name, *args):
    _lib().call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(t):
    """every float of t still holds the NaN it was filled with, bit for bit"""
    return bool((_bits(t) == _bits(torch.full((1,), NAN, device=t.device))).all())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


class Out:
    """a (rows, width) fp32 output inside a NaN-filled buffer, GUARD rows before and after it"""

    def __init__(self, dev, rows, width):
        self.rows, self.width = rows, width
        self.buf = torch.full((rows + 2 * GUARD, width), NAN, device=dev)

    @property
    def ptr(self):
        return _p(self.buf, GUARD * self.width)

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.rows]

    def guards_intact(self):
        return _untouched(self.buf[:GUARD]) and _untouched(self.buf[GUARD + self.rows:])


@functools.lru_cache(maxsize=None)
def _packed(kind):
    """the weight image of an input kind on the device (pem.pack_rpe_front: the pack scales and their inverses are under test too)"""
    from sam6d_hip import pem
    dev = torch.device("cuda:0")
    w = R.front_weights(kind)
    L = dict(qkv=pem.Linear(w.Wqkv.to(dev), w.b.to(dev)), wpT=w.Wp.t().contiguous().to(dev))
    fr = pem.pack_rpe_front(L, w.dcT.to(dev).contiguous())
    torch.cuda.synchronize()
    return dict(img=fr["img"], inv=fr["inv"], b=L["qkv"].b)


def _front(dev, x, kind, vt=None):
    """sam6d_rpe_front (vt = None) or sam6d_rpe_front_vt (vt = (n, ldp)) on x (M,256): the Out buffers (qkv, qp, qd[, vT])"""
    pk = _packed(kind)
    M = x.shape[0]
    x_d = x.to(dev)
    outs = [Out(dev, M, 3 * C), Out(dev, M, R.H * C), Out(dev, M * R.H, 32)]
    head = (_p(x_d), pk["img"].data_ptr(), _p(pk["b"]), pk["inv"][0], pk["inv"][1], pk["inv"][2], outs[0].ptr, outs[1].ptr, outs[2].ptr, M)
    if vt is None:
        _call("sam6d_rpe_front", *head, _stream())
    else:
        n, ldp = vt
        outs.append(Out(dev, (M // n) * C, ldp))
        _call("sam6d_rpe_front_vt", *head, outs[3].ptr, n, ldp, _stream())
    torch.cuda.synchronize()
    for o, what in zip(outs, ("qkv", "qp", "qd", "vT")):
        assert o.guards_intact(), "%s: guard rows written" % what
    return outs


def _got(outs):
    M = outs[0].rows
    return outs[0].body.cpu(), outs[1].body.cpu().reshape(M, R.H, C), outs[2].body.cpu().reshape(M, R.H, 32)


def _check_front(got, x, w, what):
    r = R.front_ratios(got, x, w)
    print("%s: worst |err| / bound  qkv %.3f  qp %.3f  qd %.4f  | folds alone  qp %.3f  qd %.3f" % ((what,) + tuple(r)))
    assert max(r) <= 1.0, "%s: |err| / bound (qkv, qp, qd, qp fold, qd fold) = %s" % (what, r)


# ------------------------------------------------------------------------------------------------------- 1. sam6d_rpe_front
@pytest.mark.parametrize("kind,M", R.FRONT_CASES, ids=["%s-%d" % c for c in R.FRONT_CASES])
def test_rpe_front_vs_float64(dev, kind, M):
    """every element of qkv, qp and qd against float64 with its own bound (chained, and each fold alone against the kernel's own q /
    qp): M on both sides of the 16-row wave and the 64-row workgroup; rows eight decades apart in one call with an all-zero token and a
    one-channel token; x, Wqkv, Wp, D_c and the bias far from unit scale"""
    x, w = R.front_x(kind, M), R.front_weights(kind)
    outs = _front(dev, x, kind)
    got = _got(outs)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _check_front(got, x, w, "rpe_front %s M=%d" % (kind, M))
    if kind == "mixed":
        z, _ = R.mixed_special_rows(M)
        assert _same_bits(got[0][z], w.b), "an all-zero token: qkv is the bias bit for bit"
        alone = _got(_front(dev, torch.zeros(1, C), kind))
        assert all(_same_bits(g[z], a[0]) for g, a in zip(got, alone)), "an all-zero token: the bias and its folds, wherever it stands"


def test_rpe_front_token_does_not_depend_on_its_row(dev):
    """the same token at rows 0, 15, 16, 63, 64 and M - 1 of different calls gives the same 768 + 1024 + 128 values bit for bit"""
    M = R.INDEPENDENCE_M
    base = R.front_x("unit", M)
    tok = R.front_x("unit", 1, seed=99)[0] * 37.0  # (a scale of its own: its row scale differs from every neighbour's)
    ref = None
    for p in R.INDEPENDENCE_ROWS + [M - 1]:
        x = base.clone()
        x[p] = tok
        got = [g[p].clone() for g in _got(_front(dev, x, "unit"))]
        if ref is None:
            ref = got
        assert all(_same_bits(a, b) for a, b in zip(got, ref)), "row %d" % p


@pytest.mark.parametrize("M", [17, 65, 129])
def test_rpe_front_clamped_tail_leaves_the_other_rows(dev, M):
    """the lanes past M recompute row M - 1 and store it again: rows 0 .. M - 2 keep their bits when row M - 1 changes"""
    x = R.front_x("unit", M)
    a = _got(_front(dev, x, "unit"))
    y = x.clone()
    y[M - 1] = R.front_x("unit", 1, seed=7)[0] * 1e3
    b = _got(_front(dev, y, "unit"))
    assert all(_same_bits(p[:M - 1], q[:M - 1]) for p, q in zip(a, b))
    assert not _same_bits(a[0][M - 1], b[0][M - 1])
    _check_front(b, y, R.front_weights("unit"), "rpe_front changed last row M=%d" % M)


# ------------------------------------------------------------------------------------------------------- 2. sam6d_rpe_front_vt
@pytest.mark.parametrize("Bp,n,extra", R.VT_CASES, ids=["%d-%d-%d" % c for c in R.VT_CASES])
def test_rpe_front_vt_vs_float64(dev, Bp, n, extra):
    """q | k, qp, qd and the values read back from vT against float64 with the same bounds, on both sides of n = 208 (the entry's
    production range is n > 208); columns [n, ldp) of vT and the v third of qkv stay untouched"""
    M, ldp = Bp * n, R.ldp_of(n, extra)
    x, w = R.front_x("unit", M), R.front_weights("unit")
    outs = _front(dev, x, "unit", vt=(n, ldp))
    qkv, qp, qd = _got(outs)
    vT = outs[3].body.reshape(Bp, C, ldp)
    assert _untouched(outs[0].body[:, 2 * C:]), "the v third of qkv was written"
    assert _untouched(vT[:, :, n:]), "columns [n, ldp) of vT were written"
    v = vT[:, :, :n].cpu().transpose(1, 2).reshape(M, C)  # v[cloud n + tok][c] = vT[cloud][c][tok]
    assert bool(torch.isfinite(v).all())
    got = (torch.cat([qkv[:, :2 * C], v], 1), qp, qd)
    _check_front(got, x, w, "rpe_front_vt Bp=%d n=%d ldp=%d" % (Bp, n, ldp))
    e_v = R.front_bounds(x, w)[0][:, 2 * C:]
    r = R.worst_ratio(vT[:, :, :n].cpu(), R.vt64(R.front64(x, w)[0], Bp, n), R.vt64(torch.cat([e_v] * 3, 1), Bp, n))
    print("rpe_front_vt Bp=%d n=%d ldp=%d: vT worst |err| / bound %.3f" % (Bp, n, ldp, r))
    assert r <= 1.0


@pytest.mark.parametrize("Bp,n", R.VT_BITWISE)
def test_rpe_front_vt_equals_front_and_transpose(dev, Bp, n):
    """the same bits as sam6d_rpe_front + sam6d_transpose in the range pem._rpe_self_front calls the entry in (n > 208)"""
    M, ldp = Bp * n, R.ldp_of(n)
    x = R.front_x("unit", M)
    a = _front(dev, x, "unit")
    b = _front(dev, x, "unit", vt=(n, ldp))
    vT_ref = Out(dev, Bp * C, ldp)
    _call("sam6d_transpose", a[0].ptr + 4 * 2 * C, 3 * C, n * 3 * C, Bp, n, C, vT_ref.ptr, ldp, C * ldp, _stream())
    torch.cuda.synchronize()
    assert vT_ref.guards_intact()
    assert _same_bits(b[3].body, vT_ref.body), "transposed values (untouched padding included)"
    assert _same_bits(a[0].body[:, :2 * C], b[0].body[:, :2 * C]) and _same_bits(a[1].body, b[1].body) and _same_bits(a[2].body, b[2].body)


# ------------------------------------------------------------------------------------------------------- 3. sam6d_linattn_kv_image
def _kv_rows(dev, B, J, ld, gap, seed):
    """(B, J + gap, ld) buffer: the J x 512 rows of every cloud ~ 1.7 N(0,1), the gap rows and the columns past 512 NaN"""
    g = R.gen(8000 + 100 * B + J + ld + gap + seed)
    kv = torch.full((B, J + gap, ld), NAN)
    kv[:, :J, :2 * C] = torch.randn(B, J, 2 * C, generator=g) * 1.7
    return kv.to(dev).contiguous()


def _kv_image(dev, kv_d, scale_d, B, J, ld, stride):
    """sam6d_linattn_kv_image into guarded buffers: (image bytes (B, nb), inv (B,4), ksum (B,256))"""
    nb = int(_lib().load().sam6d_linattn_kv_image_bytes())
    img = torch.full((B + 2, nb), 0xA5, dtype=torch.uint8, device=dev)
    inv, ks = Out(dev, B, 4), Out(dev, B, C)   # (GUARD rows of 4 floats = 32 bytes: inv keeps its 16-byte alignment)
    _call("sam6d_linattn_kv_image", _p(kv_d), _p(scale_d), B, J, ld, stride, img.data_ptr() + nb, inv.ptr, ks.ptr, _stream())
    torch.cuda.synchronize()
    assert bool((img[0] == 0xA5).all()) and bool((img[B + 1] == 0xA5).all()), "image guard bytes written"
    assert inv.guards_intact() and ks.guards_intact()
    return img, inv, ks


@pytest.mark.parametrize("J", R.KV_J)
def test_linattn_kv_image_equals_three_launches(dev, J):
    """the same bits as sam6d_linattn_focus_k + sam6d_linattn_kv + sam6d_linattn_kv_pack (pinned to float64 at these J by
    tests/test_attn_shapes_gpu.py) on both sides of the 16-key step and the 32-key trip, with rows of 512, 516 and 768 floats and a gap
    of two rows between the clouds; the gap rows and the columns past 512 hold NaN, which a read past J or past the 512 channels would
    carry into the sums"""
    nb = int(_lib().load().sam6d_linattn_kv_image_bytes())
    scale_d = (0.3 * torch.randn(C, generator=R.gen(J))).to(dev)
    for B in R.KV_B:
        for ld in R.KV_LD:
            for gap in R.KV_GAP:
                what = "J=%d B=%d ld=%d gap=%d" % (J, B, ld, gap)
                stride = (J + gap) * ld
                kv_d = _kv_rows(dev, B, J, ld, gap, 0)
                kv_in = kv_d.clone()
                img, inv, ks = _kv_image(dev, kv_d, scale_d, B, J, ld, stride)
                assert torch.equal(_bits(kv_d), _bits(kv_in)), what + ": the kv rows were written"
                k2 = kv_d.clone()
                _call("sam6d_linattn_focus_k", _p(k2), _p(scale_d), B * (J + gap), ld, _stream())
                kvT = torch.full((B, R.H, 64, 64), NAN, device=dev)
                ks2 = torch.full((B, C), NAN, device=dev)
                _call("sam6d_linattn_kv", _p(k2), _p(k2, C), B, J, ld, ld, stride, stride, _p(kvT), _p(ks2), _stream())
                img2 = torch.zeros(B, nb, dtype=torch.uint8, device=dev)
                inv2 = torch.full((B, 4), NAN, device=dev)
                _call("sam6d_linattn_kv_pack", _p(kvT), B, img2.data_ptr(), _p(inv2), _stream())
                torch.cuda.synchronize()
                assert bool(torch.isfinite(kvT).all()) and bool(torch.isfinite(ks2).all()), what + ": the three launches read a NaN"
                assert bool(torch.isfinite(ks.body).all()) and bool(torch.isfinite(inv.body).all()) and bool((inv.body > 0).all()), what
                assert _same_bits(ks.body, ks2), what + ": key sums"
                assert _same_bits(inv.body, inv2), what + ": image scales (one per head)"
                assert torch.equal(img[1:B + 1], img2), what + ": packed kv^T image: %d bytes differ" % int((img[1:B + 1] != img2).sum())


# ------------------------------------------------------------------------------------------------------- 4. the dense layer, directly
@functools.lru_cache(maxsize=None)
def _dense_packed():
    from sam6d_hip import pem
    dev = torch.device("cuda:0")
    L = R.dense_weights()
    Ld = {k: (pem.Linear(v[0].to(dev), v[1].to(dev)) if k in ("lin", "exp", "sq", "q", "kv") else tuple(t.to(dev).contiguous() for t in v))
          for k, v in L.items() if k != "scale"}
    Ld["scale"] = L["scale"].to(dev)
    tb = pem.pack_token_block(Ld, Ld["q"], Ld["scale"])
    torch.cuda.synchronize()
    return dict(img=tb["img"], cst=tb["cst"], scale=Ld["scale"])


def _dense(dev, B, I, J, row0, mem_scale=1.0):
    """sam6d_linattn_kv_image + sam6d_linattn_layer on R.dense_inputs: max |err| against float64 on rows row0 .. I-1; rows < row0 of
    every cloud and the guard rows must keep their fill"""
    pk = _dense_packed()
    Dn, kv = R.dense_inputs(B, I, J, mem_scale)
    want = R.dense_layer64(Dn, kv, R.dense_weights(), row0)
    D_d, kv_d = Dn.to(dev), kv.to(dev)
    img, inv, ks = _kv_image(dev, kv_d, pk["scale"], B, J, 2 * C, J * 2 * C)
    nb = img.shape[1]
    out = Out(dev, B * I, C)
    _call("sam6d_linattn_layer", _p(D_d), pk["img"].data_ptr(), _p(pk["cst"]), img.data_ptr() + nb, inv.ptr, ks.ptr, out.ptr, B, I, row0,
          R.EPS, _stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), "Dout guard rows written"
    body = out.body.reshape(B, I, C)
    assert _untouched(body[:, :row0]), "rows < row0 of Dout were written"
    got = body[:, row0:].cpu().double()
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max())


@pytest.mark.parametrize("J", R.DENSE_J)
def test_linattn_layer_direct_vs_float64(dev, J):
    """the whole dense layer with memories of 1, 17, 33 and 196 tokens (pem's contraction-order guard refuses the short ones: the only
    check of the packed image's decode there), I - row0 on both sides of the 64-token workgroup, row0 = 0, 1, 3, one and three clouds;
    then the memory tokens at 1e3 and 1e-3"""
    worst = 0.0
    for rows in R.DENSE_ROWS:
        for row0 in R.DENSE_ROW0:
            for B in R.DENSE_B:
                e = _dense(dev, B, rows + row0, J, row0)
                worst = max(worst, e)
                assert e <= R.DENSE_TOL, "J=%d I-row0=%d row0=%d B=%d: max error %.3e" % (J, rows, row0, B, e)
    for ms in R.DENSE_MEM_SCALES:
        e = _dense(dev, 3, 131, J, 1, ms)
        print("dense layer J=%d memory x %g: max error %.3e" % (J, ms, e))
        worst = max(worst, e)
        assert e <= R.DENSE_TOL, "J=%d memory x %g: max error %.3e" % (J, ms, e)
    print("dense layer J=%d: worst max error %.3e (bound %.1e)" % (J, worst, R.DENSE_TOL))


# ------------------------------------------------------------------------------------------------------- 5. refusals
def _refused(name, args, entry):
    lib = _lib().load()
    rc = getattr(lib, name)(*args)
    msg = lib.sam6d_last_error().decode()
    assert rc != 0, "%s%r was served" % (name, tuple(args))
    assert entry in msg, "%s: sam6d_last_error() = %r" % (name, msg)


def _swap(args, i, v):
    return args[:i] + (v,) + args[i + 1:]


def test_rpe_front_refusals(dev):
    """a pointer 4 bytes off for each of the six aligned arguments of both entries; sam6d_rpe_front_vt with M % n != 0, ldp < n, n = 0
    and vT null: an error that names the entry, nothing written; M = 0 is served and writes nothing"""
    pk = _packed("unit")
    M, n, ldp = 10, 5, 8
    x_d = R.front_x("unit", M + 1).to(dev)
    outs = [Out(dev, M, 3 * C), Out(dev, M, R.H * C), Out(dev, M * R.H, 32), Out(dev, (M // n) * C, ldp)]
    head = (_p(x_d), pk["img"].data_ptr(), _p(pk["b"]), pk["inv"][0], pk["inv"][1], pk["inv"][2], outs[0].ptr, outs[1].ptr, outs[2].ptr, M)
    plain, vt = head + (_stream(),), head + (outs[3].ptr, n, ldp, _stream())
    for i in (0, 1, 2, 6, 7, 8):
        _refused("sam6d_rpe_front", _swap(plain, i, plain[i] + 4), "rpe_front")
        _refused("sam6d_rpe_front_vt", _swap(vt, i, vt[i] + 4), "rpe_front")
    _refused("sam6d_rpe_front_vt", _swap(vt, 11, 3), "rpe_front_vt")              # M % n != 0
    _refused("sam6d_rpe_front_vt", _swap(vt, 12, n - 1), "rpe_front_vt")          # ldp < n
    _refused("sam6d_rpe_front_vt", _swap(vt, 11, 0), "rpe_front_vt")              # n = 0
    _refused("sam6d_rpe_front_vt", _swap(vt, 10, None), "rpe_front_vt")           # vT null
    _call("sam6d_rpe_front", *_swap(plain, 9, 0))                                 # M = 0
    _call("sam6d_rpe_front_vt", *_swap(vt, 9, 0))
    torch.cuda.synchronize()
    assert all(_untouched(o.buf) for o in outs), "a refused or empty call wrote"
    _call("sam6d_rpe_front_vt", *vt)                                              # the same buffers with valid arguments are served
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[1].body).all()) and all(o.guards_intact() for o in outs)


def test_linattn_kv_image_refusals(dev):
    """J = 0, ld = 508 (< 512), ld = 514 (no multiple of 4), B = 65536, kv and scale 4 bytes off: refused, nothing written; B = 0 served"""
    B, J, ld = 2, 5, 512
    nb = int(_lib().load().sam6d_linattn_kv_image_bytes())
    kv_d = torch.randn(B * J * 520 + 4, generator=R.gen(3)).to(dev)
    scale_d = torch.zeros(C + 4, device=dev)
    img = torch.full((B, nb), 0xA5, dtype=torch.uint8, device=dev)
    inv, ks = Out(dev, B, 4), Out(dev, B, C)
    ok = (_p(kv_d), _p(scale_d), B, J, ld, J * ld, img.data_ptr(), inv.ptr, ks.ptr, _stream())
    for i, v in ((3, 0), (4, 508), (4, 514), (2, 65536), (0, _p(kv_d, 1)), (1, _p(scale_d, 1))):
        _refused("sam6d_linattn_kv_image", _swap(ok, i, v), "linattn_kv_image")
    _call("sam6d_linattn_kv_image", *_swap(ok, 2, 0))                             # B = 0
    torch.cuda.synchronize()
    assert bool((img == 0xA5).all()) and _untouched(inv.buf) and _untouched(ks.buf), "a refused or empty call wrote"
    _call("sam6d_linattn_kv_image", *ok)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ks.body).all()) and inv.guards_intact() and ks.guards_intact()


def test_linattn_layer_refusals(dev):
    """row0 = I, I = 0 and a pointer 4 bytes off for D, Dout, the weight image, the kv image and kvinv (read as one 16-byte load per
    cloud): refused, nothing written; B = 0 served"""
    pk = _dense_packed()
    B, I, J, row0 = 2, 9, 5, 1
    Dn, kv = R.dense_inputs(B, I + 1, J)
    D_d, kv_d = Dn.to(dev), kv.to(dev)
    img, inv, ks = _kv_image(dev, kv_d, pk["scale"], B, J, 2 * C, J * 2 * C)
    nb = img.shape[1]
    out = Out(dev, B * I, C)
    ok = (_p(D_d), pk["img"].data_ptr(), _p(pk["cst"]), img.data_ptr() + nb, inv.ptr, ks.ptr, out.ptr, B, I, row0, R.EPS, _stream())
    for i, v in ((9, I), (8, 0), (0, ok[0] + 4), (6, ok[6] + 4), (1, ok[1] + 4), (3, ok[3] + 4), (4, ok[4] + 4)):
        _refused("sam6d_linattn_layer", _swap(ok, i, v), "linattn_layer")
    _call("sam6d_linattn_layer", *_swap(ok, 7, 0))                                # B = 0
    torch.cuda.synchronize()
    assert _untouched(out.buf), "a refused or empty call wrote"
    _call("sam6d_linattn_layer", *ok)
    torch.cuda.synchronize()
    body = out.body.reshape(B, I, C)
    assert out.guards_intact() and _untouched(body[:, :row0]) and bool(torch.isfinite(body[:, row0:]).all())
