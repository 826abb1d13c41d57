"""SAM's point-prompt path and mask decoder on the GPU: sam6d_hip.samdec.predict_low and each kernel of csrc/samdec.hip against the
float64 restatement (tests/sam_decoder_ref.py, pinned to the reference on the host), and the drop-in's generate_masks with the decoder
switched on against switched off.

Metric: max |diff| / max |ref|.  Bound: 4 x the error of the package's eager fp32 partner (samdec.eager, for a single kernel the same
step of samdec.TorchOps in fp32) on the same GPU against the same float64 values, measured in the same test -- the convention of the
DINOv2 tests.  The float64 legs run on the GPU too and never see more than 5 prompts at once."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import sam_decoder_ref as R

pytestmark = pytest.mark.gpu
SEED = 20250117
# input frame of a 480 x 640 image (768 x 1024 inside 1024 x 1024): the origin, the far corner of the frame, a point in the padded
# strip below row 768, and two identical points
POINTS = [[0.0, 0.0], [1023.0, 1023.0], [500.25, 900.5], [301.5, 207.25], [301.5, 207.25]]


def _dev():
    return torch.device("cuda:0")


def rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _ref64(psd, dsd, points, feats):
    """The restatement in float64 on the GPU, at most 5 prompts at a time."""
    dev = _dev()
    p64 = {k: v.to(dev, torch.float64) for k, v in psd.items()}
    d64 = {k: v.to(dev, torch.float64) for k, v in dsd.items()}
    lows, ious = [], []
    for a in range(0, points.shape[0], 5):
        low, iou = R.forward(p64, d64, points[a:a + 5].to(dev), feats.to(dev), 8, (1024, 1024), (64, 64))
        lows.append(low)
        ious.append(iou)
    return torch.cat(lows), torch.cat(ious)


def _weights(psd, dsd, dtype=torch.float32):
    from sam6d_hip import samdec
    return samdec.SamDecoderWeights(psd, dsd, _dev(), dtype=dtype, num_heads=8, input_image_size=(1024, 1024), grid=(64, 64))


@functools.lru_cache(maxsize=None)
def _setup():
    """Seeded full-width weights, the float64 outputs on POINTS and the eager fp32 outputs on the GPU (once for all tests)."""
    from sam6d_hip import samdec
    psd, dsd = R.seeded_weights(SEED)
    feats = R.seeded_features(SEED + 1).to(_dev())
    W = _weights(psd, dsd)
    pts = torch.tensor(POINTS, dtype=torch.float64, device=_dev())
    ref = _ref64(psd, dsd, pts, feats)
    eag = samdec.eager(pts, feats, W)
    return psd, dsd, feats, W, pts, ref, eag


def _run(points, feats, W, mode):
    from sam6d_hip import samdec
    from sam6d_hip.pem import Options
    opt = Options(matmul_mode=mode)
    tables = samdec.image_tables(feats, W, options=opt)
    low, iou = samdec.predict_low(points, tables, W, options=opt)
    torch.cuda.synchronize()
    return low, iou


def _report(name, got, ref, eag):
    out = []
    for what, g, r, e in (("low", got[0], ref[0], eag[0]), ("iou", got[1], ref[1], eag[1])):
        e_lib, e_eager = rel(g, r), rel(e, r)
        print("\n[sam_decoder] %s %s: library %.3e, eager fp32 %.3e (bound %.3e), max |ref| %.3f" % (name, what, e_lib, e_eager, 4 * e_eager,
                                                                                                    float(r.abs().max())))
        out.append((what, e_lib, e_eager))
    for what, e_lib, e_eager in out:
        assert e_lib <= 4 * e_eager, (name, what, e_lib, e_eager)


# ---------------------------------------------------------------------------------------------- 1. the full path
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("P", [1, 3, 5])
def test_full_path_against_float64(P, mode):
    psd, dsd, feats, W, pts, ref, eag = _setup()
    got = _run(pts[:P], feats, W, mode)
    assert tuple(got[0].shape) == (P, 3, 256, 256) and tuple(got[1].shape) == (P, 3) and got[0].dtype == torch.float32
    _report("P=%d mode %d" % (P, mode), got, (ref[0][:P], ref[1][:P]), (eag[0][:P], eag[1][:P]))
    if P == 5:
        assert torch.equal(got[0][3], got[0][4]) and torch.equal(got[1][3], got[1][4])  # two identical points


def test_mode2_and_other_shapes_are_refused():
    from sam6d_hip import _lib, samdec
    from sam6d_hip.pem import Options
    psd, dsd, feats, W, pts, ref, eag = _setup()
    with pytest.raises(NotImplementedError, match="mode 2"):
        samdec.image_tables(feats, W, options=Options(matmul_mode=2))
    with pytest.raises(ValueError):
        samdec.image_tables(feats[:, :, :32], W)
    x = torch.zeros(4096, device=_dev())
    s = torch.cuda.current_stream().cuda_stream
    for shape in ((128, 8, 7, 64, 64), (256, 4, 7, 64, 64), (256, 8, 6, 64, 64), (256, 8, 7, 32, 64)):
        with pytest.raises(RuntimeError, match="built for transformer_dim 256"):
            _lib.call("sam6d_samdec_image_to_token", x.data_ptr(), 128, 0, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0,
                      x.data_ptr(), x.data_ptr(), 1e-5, x.data_ptr(), 1, *shape, s)
        with pytest.raises(RuntimeError, match="built for transformer_dim 256"):
            _lib.call("sam6d_samdec_token_to_image", x.data_ptr(), x.data_ptr(), x.data_ptr(), 128, 0, x.data_ptr(), 1, *shape, x.data_ptr(),
                      1 << 30, s)
        with pytest.raises(RuntimeError, match="built for transformer_dim 256"):
            _lib.call("sam6d_samdec_upscale_masks", x.data_ptr(), 256, 4096 * 256, x.data_ptr(), x.data_ptr(), 1e-6, x.data_ptr(), x.data_ptr(),
                      x.data_ptr(), x.data_ptr(), 1, *shape, s)


# ---------------------------------------------------------------------------------------------- 2. each kernel alone
def _ops(W):
    from sam6d_hip import samdec
    psd, dsd = _setup()[:2]
    W64 = _weights(psd, dsd, torch.float64)
    return samdec.HipOps(W), samdec.TorchOps(W), samdec.TorchOps(W64)


def _kernel_case(name, fn, args32):
    """fn(ops, *args) on HipOps / TorchOps fp32 / TorchOps float64 (arguments cast); asserts the bound and returns the library's result."""
    from sam6d_hip.pem import Options, on_tensor_device
    W = _setup()[3]
    hip, t32, t64 = _ops(W)

    @on_tensor_device
    def lib(anchor, options=None):
        return fn(hip, *args32)
    got = lib(args32[0], options=Options(matmul_mode=0))
    torch.cuda.synchronize()
    ref = fn(t64, *[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args32])
    eag = fn(t32, *args32)
    e_lib, e_eager = rel(got, ref), rel(eag, ref)
    print("\n[sam_decoder] %s: kernel %.3e, eager fp32 %.3e (bound %.3e)" % (name, e_lib, e_eager, 4 * e_eager))
    assert e_lib <= 4 * e_eager, (name, e_lib, e_eager)
    return got


@pytest.mark.parametrize("layer", [0, 1])
def test_image_to_token_kernel(layer):
    """Layer 0: q table and keys shared by the prompts (strides 0); layer 1: per prompt.  P = 3."""
    g = torch.Generator().manual_seed(31 + layer)
    P, Pg = 3, (1 if layer == 0 else 3)
    G = torch.randn((Pg, 4096, 384), generator=g).to(_dev())
    keys = torch.randn((Pg, 4096, 256), generator=g).to(_dev())
    ktok = (2.0 * torch.randn((P, 7, 128), generator=g)).to(_dev())
    vtok = torch.randn((P, 7, 128), generator=g).to(_dev())
    p = "transformer.layers.%d." % layer

    def fn(ops, G, ktok, vtok, keys):
        return ops.i2t(G, 256, ktok, ops.fold(vtok, p + "cross_attn_image_to_token.out_proj"), p, keys)
    got = _kernel_case("image->token, layer %d" % layer, fn, (G, ktok, vtok, keys))
    assert tuple(got.shape) == (P, 4096, 256)


@pytest.mark.parametrize("case", ["random", "dominant", "equal"])
def test_token_to_image_kernel(case):
    g = torch.Generator().manual_seed(41)
    P = 3
    G = torch.randn((P, 4096, 384), generator=g)
    q = torch.randn((P, 7, 128), generator=g)
    if case == "dominant":  # one key per prompt whose score exceeds every other by hundreds: the others' weights underflow
        for p_, n in enumerate((0, 2077, 4095)):
            G[p_, n, :128] = 40.0 * q[p_, 3]
    if case == "equal":     # every key the same: all 4096 scores of a (token, head) pair equal, the result is the mean of v
        G[:, :, :128] = G[:, :1, :128]
    got = _kernel_case("token->image, %s" % case, lambda ops, q, G: ops.t2i(q, G, 0, 128), (q.to(_dev()), G.to(_dev())))
    assert tuple(got.shape) == (P, 7, 128)
    shared = _kernel_case("token->image, %s, one table for all prompts" % case, lambda ops, q, G: ops.t2i(q, G, 0, 128),
                          (q.to(_dev()), G[:1].to(_dev())))
    assert torch.equal(shared[0], got[0])


def test_upscale_kernel_with_constant_channels():
    """LayerNorm2d inputs with no or almost no spread over the 64 channels of a sub-pixel: variance 0 (the output is the bias) and
    variance of the order of eps = 1e-6."""
    g = torch.Generator().manual_seed(51)
    P = 2
    G = torch.randn((P, 4096, 512), generator=g)
    G[:, :64, 256:] = 0.75                                                               # constant: variance 0
    G[:, 64:128, 256:] = 0.75 + 1e-3 * torch.randn((P, 64, 256), generator=g)             # variance ~ eps
    G[:, 128:192, 256:320] = -3.0                                                        # one sub-pixel of the four constant
    hyper = torch.randn((P, 3, 32), generator=g)
    got = _kernel_case("upscale + mask product", lambda ops, G, hyper: ops.upscale(G, 256, hyper), (G.to(_dev()), hyper.to(_dev())))
    assert tuple(got.shape) == (P, 3, 256, 256)


# ---------------------------------------------------------------------------------------------- 3. batch independence
def test_batch_independence():
    """P = 64 and P = 65 (one more than a point batch): prompts 0, 31, 63 and 64 against float64 run on those prompts alone."""
    from sam6d_hip import samdec
    psd, dsd, feats, W = _setup()[:4]
    g = torch.Generator().manual_seed(61)
    pts = (torch.rand((65, 2), generator=g, dtype=torch.float64) * torch.tensor([1023.0, 767.0], dtype=torch.float64)).to(_dev())
    pick = [0, 31, 63, 64]
    ref = _ref64(psd, dsd, pts[pick], feats)
    eag = samdec.eager(pts[pick], feats, W)
    got65 = _run(pts, feats, W, 1)
    _report("P=65, prompts 0/31/63/64", (got65[0][pick], got65[1][pick]), ref, eag)
    got64 = _run(pts[:64], feats, W, 1)
    _report("P=64, prompts 0/31/63", (got64[0][pick[:3]], got64[1][pick[:3]]), (ref[0][:3], ref[1][:3]), (eag[0][:3], eag[1][:3]))


# ---------------------------------------------------------------------------------------------- 4. range
def test_range_outside_fp16():
    """As the encoders' range tests: image embedding x 1e3, one v_proj and mlp.lin1 x 2e4, so intermediates leave fp16's range; mode 1
    must still meet the bound."""
    from sam6d_hip import samdec
    psd, dsd, feats = _setup()[:3]
    dsd = dict(dsd)
    for k in ("transformer.layers.1.cross_attn_token_to_image.v_proj.weight", "transformer.layers.0.mlp.lin1.weight"):
        dsd[k] = dsd[k] * 2e4
    feats = feats * 1e3
    W = _weights(psd, dsd)
    pts = torch.tensor(POINTS[:3], dtype=torch.float64, device=_dev())
    ref = _ref64(psd, dsd, pts, feats)
    eag = samdec.eager(pts, feats, W)
    F = torch.nn.functional  # lin1 and the scaled v_proj read LayerNorm outputs: normalised stand-ins show the size of what they produce
    hidden = F.linear(F.layer_norm(samdec._tokens(pts, W), (256,)), W.md["transformer.layers.0.mlp.lin1.weight"])
    v = F.linear(F.layer_norm(feats.flatten(2).permute(0, 2, 1), (256,)), W.md["transformer.layers.1.cross_attn_token_to_image.v_proj.weight"])
    print("\n[sam_decoder] range: max |embedding| %.3e, hidden ~ %.3e, v ~ %.3e" % (float(feats.abs().max()), float(hidden.max()), float(v.abs().max())))
    assert float(hidden.max()) > 65504 and float(v.abs().max()) > 65504, "the scaled projections should leave fp16's range"
    _report("range, mode 1", _run(pts, feats, W, 1), ref, eag)


# ---------------------------------------------------------------------------------------------- 5. the drop-in
# random-initialised masks are large blobs whose boxes nearly coincide: at 0.7 (and at 0.9) a single box survives NMS and the filters'
# decisions would go unseen.  At 1.0 no IoU exceeds the threshold in any arithmetic (inter <= union), so every proposal the filters
# keep comes out, in score order; NMS itself is row f6's subject.
NMS_THRESH = 1.0


def _generator(sam, hip_decoder, thr_iou, thr_stab):
    from sam6d_hip import amg
    from tests.sam_decoder_stub import encode_image
    mod = importlib.import_module("model.sam")
    g = mod.CustomSamAutomaticMaskGenerator(sam, points_per_batch=32, pred_iou_thresh=thr_iou, stability_score_thresh=thr_stab, box_nms_thresh=NMS_THRESH,
                                            encode_image=encode_image, hip_decoder=hip_decoder)
    g.points_per_side = 8
    g.point_grids = amg.layer_point_grids(8, 0, 1)
    return g


def _gap_threshold(values, lo, hi):
    """The middle of the widest gap between consecutive sorted values among the quantiles lo .. hi: a threshold no value is near."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    v = v[int(lo * len(v)):int(hi * len(v))]
    i = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[i] + v[i + 1])), float(v[i + 1] - v[i])


def test_generate_masks_switch_on_against_off():
    """generate_masks on a 480 x 640 image with 8 x 8 = 64 points, the decoder on the library against the eager decoder, both followed
    by the same tail.  Random-initialised weights put iou near 0, so the test sets its own thresholds (in gaps of the float64 values).
    A proposal takes part in the comparison when its float64 iou, stability ratio and box cannot change within the measured eps; at
    most 1 % may be left out.  box_nms_thresh is NMS_THRESH (see there)."""
    from sam6d_hip import amg, samdec
    from tests.sam_decoder_stub import StubSamNetwork
    dev = _dev()
    sam = StubSamNetwork(dev, seed=SEED + 7)
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    crop, inp = (480, 640), amg.preprocess_shape(480, 640, 1024)
    # --- float64: decoder (<= 5 prompts at a time) and tail
    pts_img = amg.layer_point_grids(8, 0, 1)[0] * np.array([640, 480])[None, :]
    pts = torch.as_tensor(amg.apply_coords(pts_img, crop, 1024), device=dev)
    low64, iou64 = _ref64(sam.psd, sam.dsd, pts, sam.features)
    low64, iou64 = low64.flatten(0, 1), iou64.flatten()
    lg64 = amg.postprocess_masks(low64, inp, crop, 1024)
    # --- eps: 4 x what the eager fp32 chain (decoder, then the tail's interpolation) deviates from float64 on this GPU
    low32, iou32 = samdec.eager(pts, sam.features, sam.eager_weights())
    lg32 = amg.postprocess_masks(low32.flatten(0, 1), inp, crop, 1024)
    eps_pix, eps_iou = 4 * float((lg32.double() - lg64).abs().max()), 4 * float((iou32.flatten().double() - iou64).abs().max())
    del lg32, low32
    n_hi, n_lo = (lg64 > 1.0).sum(dim=(1, 2)), (lg64 > -1.0).sum(dim=(1, 2))
    stab64 = (n_hi / n_lo).cpu().numpy()
    thr_iou, gap_iou = _gap_threshold(iou64.cpu().numpy(), 0.1, 0.4)  # each filter keeps roughly two thirds
    thr_stab, gap_stab = _gap_threshold(stab64[np.isfinite(stab64)], 0.1, 0.4)
    print("\n[sam_decoder] drop-in: eps_pix %.3e, eps_iou %.3e; pred_iou_thresh %.6f (gap %.2e), stability_score_thresh %.6f (gap %.2e)"
          % (eps_pix, eps_iou, thr_iou, gap_iou, thr_stab, gap_stab))
    # --- which proposals are decided
    b_hi, b_lo = ((lg64 - 1.0).abs() <= eps_pix).sum(dim=(1, 2)), ((lg64 + 1.0).abs() <= eps_pix).sum(dim=(1, 2))
    lo = ((n_hi - b_hi) / (n_lo + b_lo)).cpu().numpy()
    hi = ((n_hi + b_hi) / (n_lo - b_lo).clamp(min=0)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        stab_decided = ((n_lo + b_lo) == 0).cpu().numpy() | ((lo >= thr_stab) & (stab64 >= thr_stab)) | ((hi < thr_stab) & (stab64 < thr_stab))
    iou_decided = ((iou64 - thr_iou).abs() > eps_iou).cpu().numpy()
    band = lg64.abs() <= eps_pix
    mask64 = lg64 > 0.0
    box64 = amg.mask_boxes(mask64)
    box_decided = ((amg.mask_boxes(mask64 | band) == box64).all(dim=1) & (amg.mask_boxes(mask64 & ~band) == box64).all(dim=1)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        keep64 = (iou64.cpu().numpy() > thr_iou) & (stab64 >= thr_stab)
    cand = np.flatnonzero(keep64 | ~iou_decided | ~stab_decided)
    # order and NMS: scores within 2 eps of each other may swap; box IoUs are ratios of integers once the boxes are decided
    s = iou64.cpu().numpy()
    close = np.zeros(len(s), dtype=bool)
    for i in cand:
        close[i] = bool((np.abs(s[cand] - s[i]) <= 2 * eps_iou).sum() > 1)
    b = box64[torch.as_tensor(cand, device=dev)].double()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    biou = (w * h / (area[:, None] + area[None, :] - w * h)).cpu().numpy()
    nms_close = np.zeros(len(s), dtype=bool)
    with np.errstate(invalid="ignore"):
        if NMS_THRESH < 1.0:
            nms_close[cand] = (np.abs(biou - NMS_THRESH) <= 1e-6).any(axis=1)
    left_out = ~iou_decided | ~stab_decided | (keep64 & (~box_decided | close | nms_close))
    print("[sam_decoder] drop-in: %d of %d proposals kept by the float64 filters, %d left out of the comparison" % (int(keep64.sum()), len(s),
                                                                                                           int(left_out.sum())))
    assert left_out.sum() <= 0.01 * len(s), "the inputs leave more than 1 %% of the proposals undecided: %s" % np.flatnonzero(left_out)
    assert 10 <= keep64.sum() <= len(s) - 10
    # --- float64 expectation: filters, score order, greedy NMS
    idx = np.flatnonzero(keep64 & ~left_out)
    idx = torch.as_tensor(idx, device=dev)
    want = idx[amg.nms_torch(box64[idx].double(), iou64[idx], NMS_THRESH)]
    # --- the two routes
    res = {}
    for name, on in (("on", True), ("off", False)):
        gen = _generator(sam, on, thr_iou, thr_stab)
        res[name] = gen.generate_masks(image)
        assert gen.predictor.hip_decoder is on
        assert sam.mask_decoder.calls == (0 if on else 2)  # switched on, the modules are never called
    for name, got in res.items():
        boxes = got["boxes"].cpu()
        if left_out.any():  # drop survivors that are left-out proposals (their boxes are their own in this fixture)
            lob = {tuple(r) for r in box64[torch.as_tensor(np.flatnonzero(left_out), device=dev)].cpu().tolist()}
            sel = [i for i, r in enumerate(boxes.tolist()) if tuple(r) not in lob]
            boxes, masks = boxes[sel], got["masks"][sel]
        else:
            masks = got["masks"]
        assert torch.equal(boxes, box64[want].cpu()), "%s: survivors, order or boxes differ from float64" % name
        diff = (masks != mask64[want]) & ~band[want]
        assert not bool(diff.any()), "%s: mask bits differ outside the eps band" % name
    assert torch.equal(res["on"]["boxes"], res["off"]["boxes"]) or left_out.any()
    print("[sam_decoder] drop-in: %d survivors, the same with the decoder on and off" % len(want))
    assert len(want) >= 2
