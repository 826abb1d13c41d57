"""What the library's ViT encoders share on the host: PEM's ViT-B/16 (vit.py) and ISM's DINOv2 ViT-L/14 (dinov2.py) are two `Encoder`
descriptions driving one launch sequence.  torch provides device buffers only.

Layout: the residual stream is X (B*NT, D) fp32, row 0 of each image the cls token (SAM's ViT-H, samenc.py, is a third description: no
cls token, and an attention launch of its own per block).  Per block:
    LN1 -> qkv GEMM -> attention -> proj GEMM (+ X, in place) -> LN2 -> fc1 GEMM (GELU) -> fc2 GEMM (+ X, in place)
In-place residual: every GEMM route loads the residual element it adds before it stores that same element of C (the stored value
depends on it), and each element of C belongs to exactly one lane, so C == residual is safe (tests/test_vit_gpu.py checks every route).
"""
import contextlib
from typing import NamedTuple

import torch

from . import _lib
from .runtime import Linear, _empty, _p, _s, gemm, on_tensor_device, require_mode


class Encoder(NamedTuple):
    """One encoder: its sizes, its three library symbols, and the launches they parameterise."""
    name: str        # module name in error messages
    role: str        # ... and what the module is there
    D: int           # width
    HID: int         # MLP hidden width
    depth: int
    NP: int          # patches of a 224 x 224 image
    NT: int          # tokens: cls + patches
    K: int           # columns of a patch row (the patch GEMM's K)
    EPS: float
    patch_rows: str
    layernorm: str
    attention: str
    cls: bool = True  # row 0 of each image is the cls token; False: NT == NP, patch_rows writes the patch rows only
    whole_tiles: bool = False  # the block GEMMs ask for the whole-tile kernel (act + 32): an image's rows are a multiple of 128

    def require_mode(self):
        require_mode(self.name, self.role)

    def ln(self, x, gb, y, nimg, rows, ldx, sx, ldy, sy, x_off=0, y_off=0):
        """Row r of image b: x + x_off + b sx + r ldx -> y + y_off + b sy + r ldy (floats), gb = (gamma, beta)."""
        _lib.call(self.layernorm, _p(x, x_off), _p(gb[0]), _p(gb[1]), _p(y, y_off), nimg, rows, ldx, sx, ldy, sy, self.EPS, _s())

    def embed(self, images, W, X, A):
        """X (B*NT, D) = [cls_token; patch_embed(images)] + pos; A (>= B*NP*K floats) is the patch-row workspace."""
        B = images.shape[0]
        if self.cls:
            _lib.call(self.patch_rows, _p(images), _p(W.cls), _p(W.pos), _p(A), _p(X), B, _s())
        else:
            _lib.call(self.patch_rows, _p(images), _p(A), B, _s())
        self.embed_rows(A, W, X, B)

    def embed_rows(self, A, W, X, B):
        """The patch GEMM alone: X's patch rows = A (B*NP, K), the images' patch rows, times the patch weight + bias + pos.  With a cls
        token the cls rows of X are the patch-rows kernel's to write (`embed`)."""
        D, K = self.D, self.K
        # one problem per image: rows land one below the image's cls row, pos[1:] is the residual (batch stride 0)
        off = D if self.cls else 0
        gemm(A, W.patch.w, W.patch.b, X, self.NP, D, K, K, K, D, c_off=off, residual=W.pos, r_off=off, ldr=D, batch=B, sA=self.NP * K,
             sW=0, sC=self.NT * D, sR=0, w16=W.patch.w16())

    def attend(self, T, Y, B, n, blk):
        """Y (B*n, D) = the multi-head attention of the qkv rows T (B*n, 3 D); blk: the block's weights, for an attention with operands
        of its own."""
        _lib.call(self.attention, _p(T), _p(Y), B, n, _s())

    def block(self, X, blk, B, Y, T, n=None):
        """One block on X (B*n, D) in place; Y (B*n, D) and T (>= B*n*HID floats) are workspaces."""
        D, HID = self.D, self.HID
        n = self.NT if n is None else n
        M = B * n
        wt = 32 if self.whole_tiles else 0
        self.ln(X, blk["n1"], Y, 1, M, D, 0, D, 0)
        gemm(Y, blk["qkv"].w, blk["qkv"].b, T, M, 3 * D, D, D, D, 3 * D, act=wt, w16=blk["qkv"].w16())
        self.attend(T, Y, B, n, blk)
        gemm(Y, blk["proj"].w, blk["proj"].b, X, M, D, D, D, D, D, residual=X, ldr=D, act=wt, w16=blk["proj"].w16())
        self.ln(X, blk["n2"], Y, 1, M, D, 0, D, 0)
        gemm(Y, blk["fc1"].w, blk["fc1"].b, T, M, HID, D, D, D, HID, act=2 + wt, w16=blk["fc1"].w16())
        gemm(T, blk["fc2"].w, blk["fc2"].b, X, M, D, HID, HID, HID, D, residual=X, ldr=D, act=wt, w16=blk["fc2"].w16())


# ------------------------------------------------------------------------------------------------- weights
def device_of(dev):
    """The context in which a weight set is packed: `dev` current when it is a GPU."""
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def pack_block(g, b, fold=None):
    """The weights of the block under key prefix `b`, fetched with g(key).  fold(linear prefix, scale prefix) -> (w, b), when given,
    supplies proj and fc2 with the block's LayerScale (ls1, ls2) folded in."""
    def lin(k, ls):
        if fold is not None and ls:
            return Linear(*fold(b + k, b + ls))
        return Linear(g(b + k + ".weight"), g(b + k + ".bias"))
    return dict(n1=(g(b + "norm1.weight"), g(b + "norm1.bias")), qkv=lin("attn.qkv", None), proj=lin("attn.proj", "ls1"),
                n2=(g(b + "norm2.weight"), g(b + "norm2.bias")), fc1=lin("mlp.fc1", None), fc2=lin("mlp.fc2", "ls2"))


class Weights:
    """Base of a packed weight set: .dev, .patch and .blocks (pack_block dictionaries)."""

    def linears(self):
        yield self.patch
        for b in self.blocks:
            yield from (b["qkv"], b["proj"], b["fc1"], b["fc2"])

    def cut_w16(self):
        """The fp16 halves of every weight, cut once at pack time."""
        if self.dev.type == "cuda":
            for lin in self.linears():
                lin.w16()


# ------------------------------------------------------------------------------------------------- pieces (tests)
def pieces(enc, check_images):
    """(embed, layernorm, attention, block) of `enc`: single stages behind the public entry-point conventions."""
    D, HID, NP, NT = enc.D, enc.HID, enc.NP, enc.NT

    @on_tensor_device
    def embed(images, W, options=None):
        """images (B, 3, 224, 224) -> X (B, NT, D) = cat(cls_token, patch_embed(images)) + pos_embed."""
        check_images(images)
        images = images.contiguous()
        B = images.shape[0]
        X = _empty((B * NT, D), images)
        enc.embed(images, W, X, _empty((B * NP, enc.K), images))
        return X.view(B, NT, D)

    @on_tensor_device
    def layernorm(x, gamma, beta, options=None):
        """x (..., D) -> nn.LayerNorm(D, eps=EPS)(x)."""
        x2 = x.reshape(-1, D).contiguous()
        y = torch.empty_like(x2)
        enc.ln(x2, (gamma.contiguous(), beta.contiguous()), y, 1, x2.shape[0], D, 0, D, 0)
        return y.view(x.shape)

    @on_tensor_device
    def attention(qkv, B, options=None):
        """qkv (B*n, 3 D) -> (B*n, D): the block's multi-head attention alone."""
        qkv = qkv.contiguous()
        out = _empty((qkv.shape[0], D), qkv)
        _lib.call(enc.attention, _p(qkv), _p(out), B, qkv.shape[0] // B, _s())
        return out

    @on_tensor_device
    def block(x, W, i, options=None):
        """x (B, n, D) -> block i of the encoder applied to a copy (n up to the attention symbol's token limit)."""
        enc.require_mode()
        B, n = x.shape[:2]
        X = x.reshape(B * n, D).contiguous().clone()
        enc.block(X, W.blocks[i], B, _empty((B * n, D), X), _empty((B * n, HID), X), n=n)
        return X.view(B, n, D)

    return embed, layernorm, attention, block
