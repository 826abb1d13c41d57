"""SAM's ViT-H image encoder on the GPU: sam6d_hip.samenc.encode, its two attention kernels alone, a block, the neck and the drop-in's
generate_masks with the encoder switched on against switched off, all against the float64 restatement (tests/sam_encoder_ref.py,
pinned to the reference on the host).

Metric: max |diff| / max |ref|.  Bound: 4 x the error of the package's eager fp32 partner (samenc.eager; for a single kernel the same
step in plain torch, samenc.rel_attention, in fp32) on the same GPU against the same float64 values, measured in the same test -- the
convention of the ViT-B, DINOv2 and mask-decoder tests.  The float64 restatement of the full path runs on the GPU too (the same
arithmetic, float64 throughout; on 8 host threads it takes 16 s at ViT-H width, on the device well under a second) and is computed
once for all tests that need it."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import sam_encoder_ref as R

pytestmark = pytest.mark.gpu
SEED = 20250311
GRID, WIN, HD, NP = 64, 14, 80, 4096
# (y, x) of a query in an interior window, in the last column of windows (8 real, 6 padded columns), in the corner window
QUERIES = {"interior": (20, 20), "last column": (20, 60), "corner": (60, 60)}


def _dev():
    return torch.device("cuda:0")


def rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _opt(mode):
    from sam6d_hip.pem import Options
    return Options(matmul_mode=mode)


def _check(name, got, ref, eag, rows=None):
    """Prints both figures, then asserts the bound; rows: {label: row index} checked on their own as well."""
    e_lib, e_eager = rel(got, ref), rel(eag, ref)
    print("\n[sam_encoder] %s: library %.3e, eager fp32 %.3e (bound %.3e), max |ref| %.3e" % (name, e_lib, e_eager, 4 * e_eager, float(ref.abs().max())))
    assert torch.isfinite(got).all(), name
    per_row = {}
    for label, r in (rows or {}).items():
        per_row[label] = float((got[r].double() - ref[r]).abs().max() / ref.abs().max())
        print("[sam_encoder] %s, %s query (row %d): library %.3e" % (name, label, r, per_row[label]))
    assert e_lib <= 4 * e_eager, (name, e_lib, e_eager)
    for label, e in per_row.items():
        assert e <= 4 * e_eager, (name, label, e, e_eager)
    return e_lib, e_eager


# ---------------------------------------------------------------------------------------------- 1. the attention kernels alone
def _attention_inputs(seed, B, heads=2, nrel=2 * WIN - 1):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B * NP, 3 * heads * HD), generator=g)
    pad = 0.5 * torch.randn((3 * heads * HD,), generator=g)
    rel_h, rel_w = 0.1 * torch.randn((nrel, HD), generator=g), 0.1 * torch.randn((nrel, HD), generator=g)
    return qkv, pad, rel_h, rel_w


def _attention_case(name, qkv, pad, rel_h, rel_w, B, win, rows=None):
    """The kernel, samenc.rel_attention in fp32 and the restatement in float64 on the same inputs (all on the GPU)."""
    from sam6d_hip import samenc
    dev = _dev()
    heads = qkv.shape[1] // (3 * HD)
    qkv, pad, rel_h, rel_w = (t.to(dev) for t in (qkv, pad, rel_h, rel_w))
    if win:
        got = samenc.pieces.window_attention(qkv, pad, rel_h, rel_w, B, options=_opt(1))
    else:
        got = samenc.pieces.global_attention(qkv, rel_h, rel_w, B, options=_opt(1))
    torch.cuda.synchronize()
    ref = R.attention(qkv.double().view(B, GRID, GRID, -1), pad.double(), rel_h.double(), rel_w.double(), heads, win).reshape(B * NP, -1)
    eag = samenc.rel_attention(qkv, pad, rel_h, rel_w, B, heads, GRID, win or GRID)
    assert tuple(got.shape) == (B * NP, heads * HD) and got.dtype == torch.float32
    _check(name, got, ref, eag, rows)
    return got


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("case", ["random", "pad keys dominant", "keys equal"])
def test_window_attention(case, B):
    heads = 2
    qkv, pad, rel_h, rel_w = _attention_inputs(11 + B, B)
    D = heads * HD
    if case == "pad keys dominant":
        # every query has a common component along channel 3 of each head; the padded key points along it, so that wherever a window
        # has padded keys they take nearly all the weight (score + 3 * 40 / sqrt(80) = 13): a kernel that drops them fails
        for h in range(heads):
            qkv[:, h * HD + 3] = 3.0 + 0.1 * qkv[:, h * HD + 3]
            pad[D + h * HD:D + (h + 1) * HD] = 0.0
            pad[D + h * HD + 3] = 40.0
    if case == "keys equal":  # every key the same, the padded one too: q . k is one number per query, the bias alone shapes the softmax
        qkv[:, D:2 * D] = qkv[:1, D:2 * D]
        pad[D:2 * D] = qkv[0, D:2 * D]
    rows = {label: (B - 1) * NP + y * GRID + x for label, (y, x) in QUERIES.items()}
    got = _attention_case("window attention, %s, B=%d" % (case, B), qkv, pad, rel_h, rel_w, B, WIN, rows)
    if case == "pad keys dominant":  # the corner query's output is v of the padding row, the interior one's is not
        v_pad = pad[2 * D:].to(_dev())
        assert float((got[rows["corner"]] - v_pad).abs().max()) < 1e-3
        assert float((got[rows["interior"]] - v_pad).abs().max()) > 0.1


@pytest.mark.parametrize("case", ["random", "one dominant key", "bias dominates"])
def test_global_attention(case):
    heads, B = 2, 1
    qkv, pad, rel_h, rel_w = _attention_inputs(21, B, nrel=2 * GRID - 1)
    D = heads * HD
    if case == "one dominant key":  # key 2077 exceeds every other score by ~20: the 4095 others' weights all but vanish
        for h in range(heads):
            qkv[:, h * HD + 3] = 3.0 + 0.1 * qkv[:, h * HD + 3]
            qkv[2077, D + h * HD:D + (h + 1) * HD] = 0.0
            qkv[2077, D + h * HD + 3] = 80.0
    if case == "bias dominates":    # rel-pos terms ~ 30 x q . k / sqrt(80)
        rel_h, rel_w = 30.0 * rel_h, 30.0 * rel_w
    rows = {label: y * GRID + x for label, (y, x) in QUERIES.items()}
    got = _attention_case("global attention, %s" % case, qkv, pad, rel_h, rel_w, B, 0, rows)
    if case == "one dominant key":
        assert float((got[100] - qkv[2077, 2 * D:].to(_dev())).abs().max()) < 1e-3


@pytest.mark.parametrize("win", [WIN, 0])
def test_attention_range(win):
    """q near fp16's subnormals (x 1e-6; k and the tables x 1e6, so that the scores keep their size) and v x 2e4, as the other encoders'
    range tests: the power-of-two operand scales must carry all of it."""
    heads, B = 2, 1
    qkv, pad, rel_h, rel_w = _attention_inputs(31, B, nrel=2 * (win or GRID) - 1)
    D = heads * HD
    for t in (qkv, pad[None]):
        t[:, :D] *= 1e-6
        t[:, D:2 * D] *= 1e6
        t[:, 2 * D:] *= 2e4
    rel_h, rel_w = 1e6 * rel_h, 1e6 * rel_w
    assert float(qkv[:, :D].abs().max()) < 6.2e-5 and float(qkv[:, 2 * D:].abs().max()) > 65504
    _attention_case("range, %s" % ("window" if win else "global"), qkv, pad, rel_h, rel_w, B, win)


# ---------------------------------------------------------------------------------------------- 2. the full path
@functools.lru_cache(maxsize=None)
def _setup():
    """A seeded depth-2 encoder at ViT-H width (block 0 windowed, block 1 global, neck), two 1024 x 1024 inputs, and for each the float64
    restatement and the eager fp32 result, all on the GPU, once for all tests."""
    from sam6d_hip import samenc
    dev = _dev()
    sd = R.seeded_weights(SEED)
    x = R.seeded_input(SEED + 1, 1024, batch=2).to(dev)
    W = samenc.SamEncoderWeights(sd, dev)
    sd64 = R.to_dtype(sd, torch.float64, dev)
    ref = torch.cat([R.forward(sd64, x[b:b + 1], 16, R.windows_of(sd)) for b in range(2)])
    eag = torch.cat([samenc.eager(x[b:b + 1], W) for b in range(2)])
    torch.cuda.synchronize()
    return sd, x, W, ref, eag


@pytest.mark.parametrize("mode", [0, 1])
def test_full_path_against_float64(mode):
    from sam6d_hip import samenc
    sd, x, W, ref, eag = _setup()
    assert W.geom.windows == (14, 0)
    got = samenc.encode(x[:1], W, options=_opt(mode))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 256, 64, 64) and got.dtype == torch.float32
    _check("full path, mode %d" % mode, got, ref[:1], eag[:1])


def test_block_gemms_take_the_whole_tile_route():
    """Mode 1, one image: the four GEMMs of a block through the route query (sam6d_gemm_route, nothing is launched) take the whole-tile
    FAST kernel on pre-split weights.  The encoder asks for it with act + 32: without the request the dispatch takes 128 x 128 tiles
    only from 1024 of them (qkv has 960 at one image, proj and fc2 320) and keeps the GELU epilogue (fc1) off FAST -- codes
    [18, 18, 22, 18].  (Matmul mode 0 ignores the request: measured slower there.)  Then fc1's shape through both kernels against
    float64: the whole-tile GELU instance is new."""
    from sam6d_hip import samenc
    from sam6d_hip.pem import _empty, gemm, on_tensor_device
    sd, x, W, ref, eag = _setup()
    fast, w16 = 8, 2  # SAM6D_GEMM_ROUTE_FAST, SAM6D_GEMM_ROUTE_H3_W16 (include/sam6d_hip.h)
    g = torch.Generator().manual_seed(5)
    a = torch.randn((NP, 1280), generator=g).to(_dev())
    fc1 = W.blocks[0]["fc1"]

    @on_tensor_device
    def run(anchor, options=None):
        outs = []
        for act in (2 + 32, 2):
            out = _empty((NP, 5120), anchor)
            gemm(anchor, fc1.w, fc1.b, out, NP, 5120, 1280, 1280, 1280, 5120, act=act, w16=fc1.w16())
            outs.append(out)
        return samenc.block_gemm_routes(W, 1), outs
    codes, (whole, checked) = run(a, options=_opt(1))
    torch.cuda.synchronize()
    print("\n[sam_encoder] block GEMM routes (qkv, proj, fc1, fc2):", codes)
    assert all((c & fast) and (c & 3) == w16 for c in codes), codes
    want = torch.nn.functional.gelu(torch.nn.functional.linear(a.double(), fc1.w.double(), fc1.b.double()))
    eager = torch.nn.functional.gelu(torch.nn.functional.linear(a, fc1.w, fc1.b))
    _check("fc1 + GELU on the whole-tile kernel", whole, want, eager)
    _check("fc1 + GELU on the checked 128 x 128 kernel", checked, want, eager)


def test_batch_independence():
    from sam6d_hip import samenc
    sd, x, W, ref, eag = _setup()
    got = samenc.encode(x, W, options=_opt(1))
    one = samenc.encode(x[1:], W, options=_opt(1))
    torch.cuda.synchronize()
    for b in range(2):
        _check("B=2, image %d" % b, got[b:b + 1], ref[b:b + 1], eag[b:b + 1])
    assert torch.equal(one[0], got[1])
    # more images than a slice holds, with a remainder: three images in slices of two
    prev = samenc.SLICE
    try:
        samenc.SLICE = 2
        three = samenc.encode(torch.cat([x, x[:1]]), W, options=_opt(1))
    finally:
        samenc.SLICE = prev
    assert torch.equal(three[:2], got) and torch.equal(three[2], got[0])


def test_block_and_neck_pieces():
    """`pieces.block` on a windowed and on a global block, and `pieces.neck`, against the restatement's same stages."""
    from sam6d_hip import samenc
    sd, x, W, ref, eag = _setup()
    dev = _dev()
    sd64 = R.to_dtype(sd, torch.float64, dev)
    sd32 = R.to_dtype(sd, torch.float32, dev)
    X = R.embed(sd32, x[:1])                                    # (1, 64, 64, 1280)
    for i, win in enumerate(W.geom.windows):
        got = samenc.pieces.block(X.reshape(1, NP, -1), W.blocks[i], options=_opt(1)).view(1, GRID, GRID, -1)
        want = R.block(sd64, "blocks.%d." % i, X.double(), 16, win)
        _check("block %d (%s)" % (i, "windowed" if win else "global"), got, want, samenc._eager_block(sd32, "blocks.%d." % i, X, 16, win, 1e-6))
    got = samenc.pieces.neck(X.reshape(1, NP, -1), W, options=_opt(1))
    _check("neck", got, R.neck(sd64, X.double()), R.neck(sd32, X))


def test_mode2_and_wrong_shapes_are_refused():
    from sam6d_hip import _lib, samenc
    sd, x, W, ref, eag = _setup()
    with pytest.raises(NotImplementedError, match="mode 2"):
        samenc.encode(x[:1], W, options=_opt(2))
    with pytest.raises(ValueError, match="1024"):
        samenc.encode(x[:1, :, :512, :512], W)
    with pytest.raises(ValueError):
        samenc.pieces.window_attention(torch.zeros((NP, 3 * HD + 1), device=_dev()), torch.zeros(3 * HD, device=_dev()),
                                       torch.zeros((27, HD), device=_dev()), torch.zeros((27, HD), device=_dev()), 1)
    with pytest.raises(ValueError):  # a windowed block's table given to the global kernel
        samenc.pieces.global_attention(torch.zeros((NP, 3 * HD), device=_dev()), torch.zeros((27, HD), device=_dev()),
                                       torch.zeros((27, HD), device=_dev()), 1)
    t = torch.zeros(4096, device=_dev())
    s = torch.cuda.current_stream().cuda_stream
    p = t.data_ptr()
    for args, text in (((p, p, p, p, p, 1, 0, s), "heads"), ((p, p, p, p, p, 1, 65, s), "heads"), ((p, p, p, p, p, -1, 16, s), "B"),
                       ((p, p + 4, p, p, p, 1, 16, s), "aligned"), ((p, None, p, p, p, 1, 16, s), "null")):
        with pytest.raises(RuntimeError, match=text):
            _lib.call("sam6d_sam_window_attention", *args)
    for args, text in (((p, p, p, p, 1, 0, s), "heads"), ((p, p, p + 4, p, 1, 16, s), "aligned"), ((None, p, p, p, 1, 16, s), "null")):
        with pytest.raises(RuntimeError, match=text):
            _lib.call("sam6d_sam_global_attention", *args)
    with pytest.raises(RuntimeError, match="B"):
        _lib.call("sam6d_sam_neck_gather", p, p, 5000, s)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("sam6d_sam_patch_rows", None, p, 1, s)


# ---------------------------------------------------------------------------------------------- 3. the drop-in
NMS_THRESH = 1.0  # (as tests/test_sam_decoder_gpu.py: random-initialised masks are blobs whose boxes nearly coincide)
BAND_CAP = 1e-4   # of a mask's pixels may lie within eps of the threshold (DESIGN row f6's cap)
# Quantile windows of the float64 values in which the two thresholds are placed.  A seeded decoder's masks are shallow (|logit| stays below
# about 5, below 1.7 for the flattest mask), and a shallow mask keeps many pixels near 0: with the stability threshold in the lower half
# of its values the flattest kept mask has 2e-4 of its pixels in the band.  The masks with the highest stability ratios are the steep
# ones, so the stability threshold goes into the top of its range (15 of 192 proposals are kept) and the iou threshold to the bottom.
Q_IOU, Q_STAB = (0.0, 0.05), (0.85, 0.95)


def _gap_threshold(values, lo, hi):
    """The middle of the widest gap between consecutive sorted values among the quantiles lo .. hi: a threshold no value is near."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    v = v[int(lo * len(v)):int(hi * len(v))]
    i = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[i] + v[i + 1])), float(v[i + 1] - v[i])


def _generator(sam, hip_encoder, thr_iou, thr_stab):
    from sam6d_hip import amg
    from tests.sam_encoder_stub import encode_image
    mod = importlib.import_module("model.sam")
    g = mod.CustomSamAutomaticMaskGenerator(sam, points_per_batch=32, pred_iou_thresh=thr_iou, stability_score_thresh=thr_stab,
                                            box_nms_thresh=NMS_THRESH, encode_image=encode_image, hip_encoder=hip_encoder)
    g.points_per_side = 8
    g.point_grids = amg.layer_point_grids(8, 0, 1)
    return g


def _dropin_chain(sam, image):
    """The float64 chain (encoder, decoder <= 5 prompts at a time, the tail's interpolation) on `image` -> full-resolution logits and
    predicted IoUs of the 192 proposals, and eps = 4 x the deviation of the eager fp32 chain from them on this device."""
    from sam6d_hip import amg, samdec
    from tests.sam_encoder_stub import preprocessed
    from tests.test_sam_decoder_gpu import _ref64
    dev = _dev()
    crop, inp = (480, 640), amg.preprocess_shape(480, 640, 1024)
    x = preprocessed(sam, image)
    feats64 = R.forward(R.to_dtype(sam.esd, torch.float64, dev), x, 16, R.windows_of(sam.esd))
    pts_img = amg.layer_point_grids(8, 0, 1)[0] * np.array([640, 480])[None, :]
    pts = torch.as_tensor(amg.apply_coords(pts_img, crop, 1024), device=dev)
    low64, iou64 = _ref64(sam.psd, sam.dsd, pts, feats64)
    low64, iou64 = low64.flatten(0, 1), iou64.flatten()
    lg64 = amg.postprocess_masks(low64, inp, crop, 1024)
    feats32 = sam.image_encoder(x)
    sam.image_encoder.calls = 0
    low32, iou32 = samdec.eager(pts, feats32, sam.eager_weights())
    lg32 = amg.postprocess_masks(low32.flatten(0, 1), inp, crop, 1024)
    eps_pix, eps_iou = 4 * float((lg32.double() - lg64).abs().max()), 4 * float((iou32.flatten().double() - iou64).abs().max())
    print("\n[sam_encoder] drop-in: features eager fp32 %.3e; eps_pix %.3e, eps_iou %.3e, max |logit| %.3e" % (rel(feats32, feats64), eps_pix, eps_iou,
                                                                                                             float(lg64.abs().max())))
    return lg64, iou64, eps_pix, eps_iou


def _dropin_decide(chain, q_iou, q_stab):
    """Thresholds in the widest gaps of the float64 values within the given quantile windows, which proposals the float64 filters
    keep, which are decided within eps, the float64 survivors in order, and the largest share of a kept mask's pixels in the band."""
    from sam6d_hip import amg
    lg64, iou64, eps_pix, eps_iou = chain
    dev = lg64.device
    n_hi, n_lo = (lg64 > 1.0).sum(dim=(1, 2)), (lg64 > -1.0).sum(dim=(1, 2))
    stab64 = (n_hi / n_lo).cpu().numpy()
    thr_iou, gap_iou = _gap_threshold(iou64.cpu().numpy(), *q_iou)
    thr_stab, gap_stab = _gap_threshold(stab64[np.isfinite(stab64)], *q_stab)
    print("[sam_encoder] drop-in: pred_iou_thresh %.6f (gap %.2e), stability_score_thresh %.6f (gap %.2e)" % (thr_iou, gap_iou, thr_stab, gap_stab))
    b_hi, b_lo = ((lg64 - 1.0).abs() <= eps_pix).sum(dim=(1, 2)), ((lg64 + 1.0).abs() <= eps_pix).sum(dim=(1, 2))
    lo = ((n_hi - b_hi) / (n_lo + b_lo)).cpu().numpy()
    hi = ((n_hi + b_hi) / (n_lo - b_lo).clamp(min=0)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        stab_decided = ((n_lo + b_lo) == 0).cpu().numpy() | ((lo >= thr_stab) & (stab64 >= thr_stab)) | ((hi < thr_stab) & (stab64 < thr_stab))
        keep64 = (iou64.cpu().numpy() > thr_iou) & (stab64 >= thr_stab)
    iou_decided = ((iou64 - thr_iou).abs() > eps_iou).cpu().numpy()
    band = lg64.abs() <= eps_pix
    mask64 = lg64 > 0.0
    box64 = amg.mask_boxes(mask64)
    box_decided = ((amg.mask_boxes(mask64 | band) == box64).all(dim=1) & (amg.mask_boxes(mask64 & ~band) == box64).all(dim=1)).cpu().numpy()
    s = iou64.cpu().numpy()
    cand = np.flatnonzero(keep64)
    close = np.zeros(len(s), dtype=bool)
    for i in cand:  # scores within 2 eps of each other may swap places
        close[i] = bool((np.abs(s[cand] - s[i]) <= 2 * eps_iou).sum() > 1)
    left_out = ~iou_decided | ~stab_decided | (keep64 & (~box_decided | close))
    frac = band.sum(dim=(1, 2)).double()[torch.as_tensor(keep64, device=dev)] / float(band.shape[1] * band.shape[2])  # (of the masks compared)
    frac = float(frac.max()) if frac.numel() else 0.0
    print("[sam_encoder] drop-in: %d of %d proposals kept by the float64 filters, %d left out; largest band fraction of a kept mask %.3e (cap %.0e)"
          % (int(keep64.sum()), len(s), int(left_out.sum()), frac, BAND_CAP))
    idx = torch.as_tensor(np.flatnonzero(keep64), device=dev)
    want = idx[amg.nms_torch(box64[idx].double(), iou64[idx], NMS_THRESH)]
    return dict(thr_iou=thr_iou, thr_stab=thr_stab, left_out=left_out, frac=frac, keep64=keep64, want=want, box64=box64, mask64=mask64, band=band)


def test_generate_masks_switch_on_against_off():
    """generate_masks on a 480 x 640 image with 8 x 8 points: a depth-2 seeded ViT-H-width encoder on the library against the same
    encoder in eager fp32, both followed by the existing decoder and mask-generator stubs (eager decoder, library tail).  Thresholds in
    gaps of the float64 values; eps = 4 x what the eager fp32 chain deviates from float64 on this GPU.  Expected: the survivors, their
    order and boxes of the float64 chain; mask bits equal outside the eps band; at most BAND_CAP of a mask's pixels in the band; no
    proposal left out of the comparison."""
    from tests.sam_encoder_stub import StubSamWithEncoder, SEEDS
    dev = _dev()
    sam = StubSamWithEncoder(dev, *SEEDS)
    image = sam.test_image()
    e = _dropin_decide(_dropin_chain(sam, image), Q_IOU, Q_STAB)
    thr_iou, thr_stab, left_out, keep64, want, box64, mask64, band = (e[k] for k in ("thr_iou", "thr_stab", "left_out", "keep64", "want", "box64",
                                                                                      "mask64", "band"))
    assert not left_out.any(), "proposals undecided within eps: %s" % np.flatnonzero(left_out)
    assert e["frac"] <= BAND_CAP
    assert 10 <= keep64.sum() <= len(keep64) - 10
    # --- the two routes
    res = {}
    for name, on in (("on", True), ("off", False)):
        before = {k: v.clone() for k, v in sam.image_encoder.state_dict().items()}
        gen = _generator(sam, on, thr_iou, thr_stab)
        res[name] = gen.generate_masks(image)
        assert gen.predictor.hip_encoder is on and gen.predictor.hip_decoder is False
        assert sam.image_encoder.calls == (0 if on else 1)  # switched on, the module is never called ...
        assert gen.predictor.model is sam and type(sam.image_encoder).__name__ == "_ImageEncoder"  # ... and `sam` is left as it was
        assert all(torch.equal(v, sam.image_encoder.state_dict()[k]) for k, v in before.items())
        sam.image_encoder.calls = 0
    for name, got in res.items():
        assert torch.equal(got["boxes"].cpu(), box64[want].cpu()), "%s: survivors, order or boxes differ from float64" % name
        diff = (got["masks"] != mask64[want]) & ~band[want]
        assert not bool(diff.any()), "%s: mask bits differ outside the eps band" % name
    assert torch.equal(res["on"]["boxes"], res["off"]["boxes"])
    print("[sam_encoder] drop-in: %d survivors, the same with the encoder on and off" % len(want))
    assert len(want) >= 2
