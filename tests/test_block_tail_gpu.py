"""The layer tail of the 197-token layers (csrc/block.hip, token_tail_kernel behind sam6d_token_block): output channels dealt to eight
waves per tile, activations exchanged through LDS.  Against a float64 recompute at the tile boundaries of both tile shapes and at the
row count where the shape rule switches; bitwise row independence (a token's result depends on its own row only, whatever M, the tile
shape and its neighbours are); no write outside the M rows.

Measured on MI355X, max |error| against float64 at M = 12608, this kernel / the panel-ring kernel it replaced, same inputs: plain
1.76e-6 / 1.76e-6; hidden x 1e5 1.95e-6 / 2.15e-6; hidden x 1e-6 1.63e-6 / 1.90e-6; weight x 300 1.60e-6 / 1.80e-6; weight x 1e-4
1.74e-6 / 1.51e-6."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5  # the contract of tests/test_block_gpu.py::test_token_block_vs_fp64
GUARD = 64  # rows of NaN on either side of the output


def _layer(gen):
    from sam6d_hip import pem
    mk = lambda o, i: pem.Linear((torch.rand(o, i, generator=gen) * 2 - 1) / math.sqrt(i), (torch.rand(o, generator=gen) * 2 - 1) / math.sqrt(i))
    return dict(lin=mk(256, 256), n1=(1 + 0.1 * torch.randn(256, generator=gen), 0.1 * torch.randn(256, generator=gen)), exp=mk(512, 256),
                sq=mk(256, 512), n2=(1 + 0.1 * torch.randn(256, generator=gen), 0.1 * torch.randn(256, generator=gen)))


def _to(L, dev):
    from sam6d_hip import pem
    out = {}
    for k, v in L.items():
        out[k] = pem.Linear(v.w.to(dev), v.b.to(dev)) if isinstance(v, pem.Linear) else tuple(x.to(dev).contiguous() for x in v)
    return out


def _tail64(hidden, x, L):
    """y = LN(hidden Wlin^T + b + x); out = LN(relu(y Wexp^T + b) Wsq^T + b + y), in float64"""
    d = lambda t: t.double()
    ln = lambda v, gb: torch.nn.functional.layer_norm(v, (256,), d(gb[0]), d(gb[1]), 1e-5)
    y = ln(d(hidden) @ d(L["lin"].w).t() + d(L["lin"].b) + d(x), L["n1"])
    h = torch.relu(y @ d(L["exp"].w).t() + d(L["exp"].b))
    return ln(h @ d(L["sq"].w).t() + d(L["sq"].b) + y, L["n2"])


def _launch(tb, hd, xd):
    """sam6d_token_block on device rows; the output sits between GUARD rows of NaN, which must stay NaN"""
    from sam6d_hip import _lib
    M = hd.shape[0]
    hd, xd = hd.contiguous(), xd.contiguous()
    buf = torch.full((M + 2 * GUARD, 256), float("nan"), device=hd.device)
    out = buf[GUARD:GUARD + M]
    _lib.call("sam6d_token_block", hd.data_ptr(), xd.data_ptr(), tb["img"].data_ptr(), tb["cst"].data_ptr(), out.data_ptr(), M, 1e-5,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + M:]).all(), "write outside the M rows"
    return out.clone()


def _check(dev, L, hidden, x, what):
    from sam6d_hip import pem
    want = _tail64(hidden, x, L)
    tb = pem.pack_token_block(_to(L, dev))
    got = _launch(tb, hidden.to(dev), x.to(dev)).cpu().double()
    assert torch.isfinite(got).all(), what
    err = float((got - want).abs().max())
    print("token tail vs fp64, %s: max |err| = %.3e" % (what, err))
    assert err < TOL, "%s: %.3e" % (what, err)


def _switch_rows(dev):
    """the largest M that still runs 32-token tiles (sam6d_token_block: while they all fit the chip at once)"""
    return 32 * torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 6304, 8192, 8193, 12608, "switch", "switch+1"])
def test_tail_vs_fp64_sizes(dev, M):
    if isinstance(M, str):
        M = _switch_rows(dev) + (1 if M.endswith("+1") else 0)
    gen = torch.Generator().manual_seed(1000 + M)
    L = _layer(gen)
    _check(dev, L, torch.randn(M, 256, generator=gen), torch.randn(M, 256, generator=gen), "M = %d" % M)


@pytest.mark.parametrize("M", [300, 12608])
@pytest.mark.parametrize("hs,ws", [(1.0e5, 1.0), (1.0e-6, 1.0), (3.0, 300.0), (1.0, 1.0e-4)])
def test_tail_vs_fp64_ranges(dev, M, hs, ws):
    """hs scales the attention output (1e5: beyond fp16's 65504; 1e-6: every lo half would be a subnormal without the row scale), ws the
    linear weight -- the range cases of test_token_block_vs_fp64, in both tile shapes"""
    from sam6d_hip import pem
    gen = torch.Generator().manual_seed(M + int(math.log10(hs) * 7) + int(math.log10(ws) * 3))
    L = _layer(gen)
    L["lin"] = pem.Linear(L["lin"].w * ws, L["lin"].b)
    hidden = torch.randn(M, 256, generator=gen) * hs
    x = torch.randn(M, 256, generator=gen) * (hs * ws if hs * ws > 1 else 1.0)
    _check(dev, L, hidden, x, "M = %d, hidden x %g, weight x %g" % (M, hs, ws))


@pytest.mark.parametrize("M", [40, 12608])
def test_tail_zero_and_single_channel_rows(dev, M):
    """a row of all zeros, and rows whose only non-zero sits in the channel slice of each of the eight waves in turn"""
    gen = torch.Generator().manual_seed(77 + M)
    L = _layer(gen)
    hidden = torch.randn(M, 256, generator=gen)
    x = torch.randn(M, 256, generator=gen)
    for base in (0, M - 18):  # in the first and in the last tile
        hidden[base] = 0.0
        x[base] = 0.0
        for w in range(8):
            for k, buf in enumerate((hidden, x)):
                r = base + 1 + 2 * w + k  # k = 0: hidden has the single channel (x random); k = 1: x has it (hidden random)
                buf[r] = 0.0
                buf[r, 32 * w + 5 + w] = 3.5 - w
                assert int((buf[r] != 0).sum()) == 1 and 32 * w <= int(buf[r].nonzero()) < 32 * (w + 1)
        assert not hidden[base].any() and not x[base].any()
    _check(dev, L, hidden, x, "zero / single-channel rows, M = %d" % M)


def test_tail_rows_are_independent_bitwise(dev):
    """the rows of one M = 12608 launch (64-token tiles) = the same rows as two M = 6304 launches (32-token tiles), as M = 1 launches, and
    as a launch in which every other row is 1e4 x noise (on a chip where 12608 / 6304 rows do not straddle the shape rule's switch
    point, an M that does)"""
    from sam6d_hip import pem
    gen = torch.Generator().manual_seed(4242)
    L = _layer(gen)
    tb = pem.pack_token_block(_to(L, dev))
    sw = _switch_rows(dev)
    M = 12608 if 12608 > sw >= 6304 else 2 * (sw - sw // 4)  # the whole launch in 64-token tiles, its halves in 32-token tiles
    assert M > sw >= M // 2 and M % 2 == 0
    h = torch.randn(M, 256, generator=gen).to(dev)
    x = torch.randn(M, 256, generator=gen).to(dev)
    full = _launch(tb, h, x)
    assert torch.isfinite(full).all()
    for lo in (0, M // 2):
        part = _launch(tb, h[lo:lo + M // 2], x[lo:lo + M // 2])
        assert torch.equal(part, full[lo:lo + M // 2]), "rows %d.. as an M = %d launch" % (lo, M // 2)
    for r in (0, 17, 31, 32, M // 2 - 1, M // 2, M - 2609, M - 1):
        one = _launch(tb, h[r:r + 1], x[r:r + 1])
        assert torch.equal(one[0], full[r]), "row %d as an M = 1 launch" % r
    for MM in (M, M // 2):
        hn, xn = h[:MM].clone(), x[:MM].clone()
        hn[1::2] = 1.0e4 * torch.randn(MM // 2, 256, generator=gen).to(dev)
        xn[1::2] = 1.0e4 * torch.randn(MM // 2, 256, generator=gen).to(dev)
        noisy = _launch(tb, hn, xn)
        assert torch.equal(noisy[0::2], full[:MM][0::2]), "rows between 1e4 x noise neighbours, M = %d" % MM
