"""The row kernels the ViT-B/16 and DINOv2 ViT-L/14 encoders share (csrc/vit.hip: rows_layernorm_kernel<C>, patch_rows_kernel<C, P, KPAD>)
at the smallest shapes at which they can go wrong, through both instantiations: LayerNorm against float64 on contiguous rows around a
workgroup's four rows and on the strided per-image row map of the pyramid taps and final norms; patch rows bitwise against F.unfold."""
import pytest
import torch
import torch.nn.functional as F

from sam6d_hip import _lib, dinov2, vit
from sam6d_hip.pem import _p, _s

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ENCODERS = {768: (vit, 16, 768), 1024: (dinov2, 14, 608)}  # width -> module, patch size, columns of a patch row


def _ln_case(C, rows, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3.0 + 0.7
    w, b = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return x, w, b, F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-6)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("rows", [1, 4, 5])  # a workgroup is four rows
def test_layernorm_contiguous(dev, C, rows):
    x, w, b, ref = _ln_case(C, rows, 10 + rows)
    got = ENCODERS[C][0].layernorm(x.to(dev), w.to(dev), b.to(dev))
    assert tuple(got.shape) == (rows, C) and _rel(got, ref) <= 2e-6


@pytest.mark.parametrize("C", [768, 1024])
def test_layernorm_strided_rows(dev, C):
    """nimg = 2 images of 4 rows whose first row is skipped (x_off = C, sx = 4 C) -> rows 3 b + r of a (7, 2 C) buffer, right half
    (y_off = C, ldy = 2 C, sy = 6 C); the left half and the seventh row keep the sentinel."""
    x, w, b, ref = _ln_case(C, 8, 20)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    y = torch.full((7, 2 * C), SENTINEL, device=dev)
    with torch.cuda.device(dev):
        _lib.call(ENCODERS[C][0].ENC.layernorm, _p(xd, C), _p(wd), _p(bd), _p(y, C), 2, 3, C, 4 * C, 2 * C, 6 * C, 1e-6, _s())
    y = y.cpu()
    assert _rel(y[:6, C:], ref.reshape(2, 4, C)[:, 1:].reshape(6, C)) <= 2e-6
    assert bool((y[:6, :C] == SENTINEL).all()) and bool((y[6] == SENTINEL).all())


@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("B", [1, 2])
def test_patch_rows_bitwise(dev, C, B):
    mod, P, KPAD = ENCODERS[C]
    NP, K = (224 // P) ** 2, 3 * P * P
    g = torch.Generator().manual_seed(30 + B)
    img = torch.randn(B, 3, 224, 224, generator=g)
    cls, pos = torch.randn(C, generator=g), torch.randn((NP + 1) * C, generator=g)
    A = torch.full((B * NP, KPAD), float("nan"), device=dev)
    X = torch.full((B, NP + 1, C), SENTINEL, device=dev)
    imgd, clsd, posd = img.to(dev), cls.to(dev), pos.to(dev)
    with torch.cuda.device(dev):
        _lib.call(mod.ENC.patch_rows, _p(imgd), _p(clsd), _p(posd), _p(A), _p(X), B, _s())
    A, X = A.cpu(), X.cpu()
    want = F.unfold(img, kernel_size=P, stride=P).transpose(1, 2).reshape(B * NP, K)  # columns in (c, kh, kw) order
    assert torch.equal(A[:, :K], want)
    assert bool((A[:, K:] == 0).all())  # DINOv2: columns 588..607
    assert torch.equal(X[:, 0], (cls + pos[:C]).expand(B, C))
    assert bool((X[:, 1:] == SENTINEL).all())
