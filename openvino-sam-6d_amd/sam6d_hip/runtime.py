"""The host runtime every module of the package launches through: pointers, torch's current HIP stream and workspaces (`_p`, `_s`,
`_empty`), the `Options` of a launch sequence and the entry-point decorators that fix them per call (`on_tensor_device`,
`library_call`), `Linear` with its pre-split fp16 halves, and the GEMM launch (`gemm`, `gemm_route`, `linear`).  Imports `_lib` and
torch only.  A module-level switch that callers assign to (pem.PROFILE, samenc.SLICE) stays in the module it is assigned on.
"""
import functools
import math
import os
import threading

import torch

from . import _lib

C = 256


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t, off=0):
    return t.data_ptr() + 4 * off if t is not None else None


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _getter(sd, device):
    return lambda k: sd[k].detach().to(device=device, dtype=torch.float32).contiguous()


class Options:
    """The explicit choice of arithmetic and kernel routes for a launch sequence.  An Options object travels with a weight set
    (`PemWeights(sd, dev, options=...)`) or with one call (`pem_match(..., options=...)`, any @on_tensor_device entry point); two weight
    sets in one process can therefore run different arithmetic.  Without one, `Options.from_env()` is resolved once per outermost entry
    point.  Fields (environment variable in ENV):
      matmul_mode   None = the library's process default (sam6d_set_matmul_mode / SAM6D_MATMUL_MODE), resolved into `mode` when the
                    object is built; else 0 exact fp32 MFMA, 1 fp16 x3 split, 2 fp16 single product (experimental).  Applied as the
                    calling thread's mode for the duration of the entry point (sam6d_set_thread_matmul_mode)
      fused_block   fused transformer-block kernels (csrc/block.hip); off = the launch-per-op path
      fused_rpe / rpe_products / fused_fine / overlap / microbatch   pipeline shape of pem_match (cfg keys of the same name win)
      hip_vit       the drop-in ViTEncoder's image features on the library (sam6d_hip/vit.py) instead of eager PyTorch (off by default)
    The object keeps the values it was given; the split-precision routes (fused_block, fused_rpe) read as off in mode 0, so
    `replace(matmul_mode=1)` starts again from what the caller asked for.  Read-only routes that follow from the fields: w16 (pre-split
    fp16 weight halves in the GEMMs: modes 1 and 2) and fused_front / fused_out / rows_linear (the RPE front kernel, the fine out_proj
    + normalize + split pass and the sparse-token panel kernel: with fused_block)."""
    DEFAULTS = dict(
        matmul_mode=None,
        fused_block=True,   # fused transformer-block kernels (csrc/block.hip)
        rpe_products=0,     # 0: what the weight set allows (geo_cheb_a_packed); 3: always three stage-1 products
        fused_rpe=True,     # RPE attention without the embedding tensor
        fused_fine=True,    # fine similarity + soft assignment as one pipeline (finematch.hip)
        overlap=True,       # pose-independent fine work on a second HIP stream
        microbatch=1,
        hip_vit=False,      # ViTEncoder.get_img_feats / get_obj_feats through sam6d_hip.vit
    )
    ENV = dict(matmul_mode="SAM6D_MATMUL_MODE", fused_block="SAM6D_FUSED_BLOCK", rpe_products="SAM6D_RPE_PRODUCTS",
               fused_rpe="SAM6D_FUSED_RPE", fused_fine="SAM6D_FUSED_FINE", overlap="SAM6D_OVERLAP", microbatch="SAM6D_MICROBATCH",
               hip_vit="SAM6D_HIP_VIT")
    __slots__ = ("_kw", "mode")

    def __init__(self, **kw):
        bad = set(kw) - set(self.DEFAULTS)
        if bad:
            raise TypeError("Options: unknown field(s) %s" % sorted(bad))
        self._kw = dict(self.DEFAULTS, **kw)
        m = self._kw["matmul_mode"]
        self.mode = int(_lib.load().sam6d_get_matmul_mode()) if m is None else int(m)
        if self.mode not in (0, 1, 2):
            raise ValueError("Options.matmul_mode must be None, 0, 1 or 2")

    matmul_mode = property(lambda self: self._kw["matmul_mode"])
    fused_block = property(lambda self: bool(self._kw["fused_block"]) and self.mode >= 1)
    fused_rpe = property(lambda self: bool(self._kw["fused_rpe"]) and self.mode >= 1)
    rpe_products = property(lambda self: int(self._kw["rpe_products"]))
    fused_fine = property(lambda self: self._kw["fused_fine"])
    overlap = property(lambda self: self._kw["overlap"])
    microbatch = property(lambda self: int(self._kw["microbatch"]))
    hip_vit = property(lambda self: bool(self._kw["hip_vit"]))
    w16 = property(lambda self: self.mode >= 1)
    fused_front = fused_out = rows_linear = fused_block

    @classmethod
    def from_env(cls, **over):
        """The environment's switches (read now), overridden by keyword arguments."""
        kw = {}
        for k, name in cls.ENV.items():
            v = os.environ.get(name)
            if v is None:
                continue
            d = cls.DEFAULTS[k]
            kw[k] = int(v) if (d is None or (isinstance(d, int) and not isinstance(d, bool))) else (v == "1")
        kw.update(over)
        return cls(**kw)

    def replace(self, **over):
        """A copy with some fields changed, built from the values this object was given."""
        return Options(**dict(self._kw, **over))

    def describe(self):
        return {k: getattr(self, k) for k in self.DEFAULTS if k != "matmul_mode"} | {"matmul_mode": self.mode}


class _Tls(threading.local):
    """Per-thread state of the entry points: the Options of the outermost call in flight and its nesting depth -- the library's matmul
    mode is per thread too (sam6d_set_thread_matmul_mode), so two threads may drive two models at once."""
    flags = None
    depth = 0


_TLS = _Tls()


def _flags():
    """Inside a public entry point (on_tensor_device): the Options it was entered with; outside: the environment's, read afresh."""
    if _TLS.flags is not None:
        return _TLS.flags
    return Options.from_env()


def _find_options(args, kwargs):
    o = kwargs.pop("options", None)
    if o is not None:
        return o
    for a in list(args) + list(kwargs.values()):
        o = getattr(a, "options", None)
        if isinstance(o, Options):
            return o
    return None


def on_tensor_device(fn):
    """Run `fn` with the device of its first tensor argument current: the launches go to torch's current stream OF THAT DEVICE and
    torch.empty workspaces land there, also when the caller's current device is another GPU of the node.  The outermost decorated call
    also fixes the Options of its whole launch sequence -- the `options=` keyword, else the `.options` of a weight-set argument, else
    the environment's -- and makes their arithmetic mode the calling thread's (sam6d_set_thread_matmul_mode) until it returns."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = next((a.device for a in args if torch.is_tensor(a)), None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError("%s: needs HIP device tensors (this build has no CPU path)" % fn.__name__)
        opts = _find_options(args, kwargs)
        outer = _TLS.depth == 0
        if outer:
            _TLS.flags = opts if opts is not None else Options.from_env()
            prev_mode = int(_lib.load().sam6d_get_thread_matmul_mode())
            _lib.call("sam6d_set_thread_matmul_mode", _TLS.flags.mode)
        _TLS.depth += 1
        try:
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)
        finally:
            _TLS.depth -= 1
            if outer:
                _TLS.flags = None
                _lib.call("sam6d_set_thread_matmul_mode", prev_mode)
    return wrapper


def require_mode(name, role):
    """Refuses matmul mode 2 for the module `name` (what it is there: `role`), whose kernels serve modes 0 and 1."""
    if _flags().mode == 2:
        raise NotImplementedError("%s: matmul mode 2 is not implemented for the %s (modes 0 and 1 are)" % (name, role))


def library_call(name, role):
    """Decorator of an entry point of module `name` that takes positional arguments and `options=`: `fn` runs under on_tensor_device,
    after require_mode(name, role)."""
    def decorate(fn):
        @on_tensor_device
        @functools.wraps(fn)
        def inner(*args):
            require_mode(name, role)
            return fn(*args)

        @functools.wraps(fn)
        def run(*args, options=None):
            return inner(*args, options=options)
        return run
    return decorate


# --------------------------------------------------------------------------------------------- weights
def _pow2_scale(amax):
    """Power of two s with amax * s in [2^13, 2^14) (the fp16 split then neither overflows nor reaches subnormals)."""
    amax = float(amax)
    if not (amax > 0.0 and math.isfinite(amax)):
        return 1.0
    return 2.0 ** (14 - math.frexp(amax)[1])


class Linear:
    __slots__ = ("w", "b", "_w16", "_pimg")

    def __init__(self, w, b):
        self.w, self.b = w.contiguous(), (b.contiguous() if b is not None else None)
        self._w16 = None
        self._pimg = None

    def pimg(self):
        """(image, 1 / scale, panels): the weight (256 or 512 rows x K = 256) as the 32-row panel image of csrc/block.hip's
        rows_linear_kernel (sam6d_pack_panels), or None for another shape."""
        if self._pimg is None:
            N, K = self.w.shape
            if K != C or N not in (C, 2 * C):
                self._pimg = False
            else:
                sc = _pow2_scale(self.w.abs().max())
                img = torch.zeros((N // 32) * 32768, dtype=torch.uint8, device=self.w.device)
                _lib.call("sam6d_pack_panels", _p(self.w), K, N, 0, 8, float(sc), img.data_ptr(), _s())
                self._pimg = (img, 1.0 / sc, N // 32)
        return self._pimg or None

    def w16(self):
        """(hi, lo, scale): the weight cut into fp16 halves once (sam6d_split_f16) for sam6d_gemm_nt_w16; scale = the power of
        two that puts max |w| into [2^13, 2^14)."""
        if self._w16 is None:
            sc = _pow2_scale(self.w.abs().max())
            hi = torch.empty(self.w.shape, dtype=torch.float16, device=self.w.device)
            lo = torch.empty_like(hi)
            _lib.call("sam6d_split_f16", _p(self.w), self.w.numel(), float(sc), hi.data_ptr(), lo.data_ptr(), _s())
            self._w16 = (hi, lo, float(sc))
        return self._w16


def split_w16(w):
    """(hi, lo, scale) of a weight tensor for sam6d_gemm_nt_w16 (see Linear.w16)."""
    return Linear(w, None).w16()


# --------------------------------------------------------------------------------------------- GEMM
def gemm(A, W, bias, out, M, N, K, lda, ldw, ldc, *, a_off=0, w_off=0, c_off=0, residual=None, r_off=0, ldr=0,
         colscale=None, batch=1, sA=0, sW=0, sC=0, sR=0, divisor=1.0, act=0, w16=None):
    """w16 = Linear.w16() of the weight `W` belongs to: the pre-split halves are used in the split-precision modes."""
    if w16 is not None and K >= 32 and _flags().w16:
        hi, lo, sc = w16
        _lib.call("sam6d_gemm_nt_w16", _p(A, a_off), _p(W, w_off), hi.data_ptr() + 2 * w_off, lo.data_ptr() + 2 * w_off, sc, _p(bias),
                  _p(colscale), _p(residual, r_off), _p(out, c_off), M, N, K, lda, ldw, ldc, ldr, batch, sA, sW, sC, sR,
                  float(divisor), act, _s())
        return
    _lib.call("sam6d_gemm_nt", _p(A, a_off), _p(W, w_off), _p(bias), _p(colscale), _p(residual, r_off), _p(out, c_off),
              M, N, K, lda, ldw, ldc, ldr, batch, sA, sW, sC, sR, float(divisor), act, _s())


def gemm_route(A, W, bias, out, M, N, K, lda, ldw, ldc, *, a_off=0, w_off=0, c_off=0, residual=None, r_off=0, ldr=0, colscale=None,
               batch=1, sA=0, sW=0, sC=0, sR=0, divisor=1.0, act=0, w16=None, batch2=1, sA2=0, sW2=0, sC2=0):
    """The SAM6D_GEMM_ROUTE_* bit code of the kernel `gemm` (batch2 > 1: pem.gemm_b2) launches with these arguments, in the calling
    thread's matmul mode (sam6d_gemm_route; nothing is launched).  The pre-split weights count as `gemm` would use them."""
    wh = wl = None
    sc = 0.0
    if w16 is not None and K >= 32 and _flags().w16:
        hi, lo, sc = w16
        wh, wl = hi.data_ptr() + 2 * w_off, lo.data_ptr() + 2 * w_off
    rc = _lib.load().sam6d_gemm_route(_p(A, a_off), _p(W, w_off), wh, wl, float(sc), _p(bias), _p(colscale), _p(residual, r_off),
                                      _p(out, c_off), M, N, K, lda, ldw, ldc, ldr, batch, sA, sW, sC, sR, float(divisor), act, batch2,
                                      sA2, sW2, sC2)
    if rc < 0:
        raise RuntimeError("sam6d_gemm_route failed (rc=%d): %s" % (rc, _lib.load().sam6d_last_error().decode()))
    return rc


def linear(x2d, lin, *, act=0, residual=None, out=None):
    """x2d (M,K) contiguous -> (M,N) = act(x W^T + b) (+ residual)."""
    M, K = x2d.shape
    N = lin.w.shape[0]
    if out is None:
        out = _empty((M, N), x2d)
    gemm(x2d, lin.w, lin.b, out, M, N, K, K, K, N, residual=residual, ldr=N, act=act, w16=lin.w16())
    return out
