"""SAM's mask-generator tail on the GPU: sam6d_amg_mask_stats / sam6d_amg_unpack_masks through the C ABI and through sam6d_hip.amg
against the float64 restatement (tests/sam_amg_ref.py), and the drop-in's generate_masks on HIP against eager_tail on the CPU.

How thresholded results are compared: eps = 4 x max|eager fp32 on this GPU - float64| is measured per geometry; the kernel's logits
must lie within eps of float64, mask bits must equal the float64 decision outside the eps band of the threshold, counts may differ by
the band's size, and the inputs keep at most 1e-4 of a mask's pixels inside a band (sam_amg_ref.check_cap)."""
import importlib
import warnings

import numpy as np
import pytest
import torch

from tests import sam_amg_ref as R
from tests._util import golden

pytestmark = pytest.mark.gpu
GUARD = -77


def _dev():
    return torch.device("cuda:0")


def _eps(low, inp, crop, S, lg64):
    """4 x the deviation of torch's own fp32 interpolation on this GPU from float64."""
    from sam6d_hip import amg
    eager = amg.postprocess_masks(torch.from_numpy(low).to(_dev()), inp, crop, S).double().cpu().numpy()
    yard = float(np.abs(eager - lg64).max())
    return 4.0 * yard, yard


def _unpack_bits(bits, ow):
    """(M, oh, wd) int32 words -> (M, oh, ow) bool, and the number of set bits per mask over all 32 * wd positions."""
    b = bits.cpu().numpy().view(np.uint32)
    allbits = ((b[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(b.shape[0], b.shape[1], -1).astype(bool)
    return allbits[:, :, :ow], allbits.sum(axis=(1, 2))


def _check(out, live, lg64, thr, off, eps, ow, name):
    masks, pop = _unpack_bits(out["bits"], ow)
    live = np.asarray(live, dtype=bool)
    area = out["area"].cpu().numpy()
    assert np.array_equal(pop[live], area[live]), "%s: popcount(bits) != area" % name
    got = dict(n_hi=out["n_hi"].cpu().numpy()[live], n_lo=out["n_lo"].cpu().numpy()[live], area=area[live], box=out["box"].cpu().numpy()[live],
               masks=masks[live])
    R.compare_stats(got, lg64[live], thr, off, eps, name)
    return masks


def test_c_abi_against_float64_on_the_fixture():
    from sam6d_hip import _lib
    z = golden("sam_amg")
    S, thr, off = int(z["S"]), float(z["thr"]), float(z["offset"])
    dev = _dev()
    for c, (H, W, x0, y0, x1, y1) in enumerate(z["cases"].tolist()):
        low = R.build_logits(z["params"], z["c%d.seeds" % c])
        M, lh, lw = low.shape
        oh, ow = y1 - y0, x1 - x0
        inp = tuple(int(v) for v in z["c%d.input_size" % c])
        lg64 = R.postprocess_masks(low, inp, (oh, ow), S)
        eps, yard = _eps(low, inp, (oh, ow), S, lg64)
        frac = R.check_cap(lg64, (thr, thr + off, thr - off), eps)
        live = z["c%d.keep_iou" % c].astype(np.uint8)
        assert live.sum() == M - 1
        wd = (ow + 31) // 32
        g = lambda *s: torch.full(s, GUARD, dtype=torch.int32, device=dev)  # noqa: E731
        n_hi, n_lo, area, box, bits = g(M + 2), g(M + 2), g(M + 2), g(M + 2, 4), g(M + 2, oh, wd)
        logits = torch.full((M + 2, oh, ow), float(GUARD), dtype=torch.float32, device=dev)
        nbytes = int(_lib.load().sam6d_amg_mask_stats_workspace_bytes(M, lh, lw, S, inp[0], oh))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lowd, lived = torch.from_numpy(low).to(dev), torch.from_numpy(live).to(dev)
        _lib.call("sam6d_amg_mask_stats", lowd.data_ptr(), lived.data_ptr(), M, lh, lw, S, inp[0], inp[1], oh, ow, thr, off,
                  n_hi[1:].data_ptr(), n_lo[1:].data_ptr(), area[1:].data_ptr(), box[1:].data_ptr(), bits[1:].data_ptr(), logits[1:].data_ptr(),
                  ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dead = [0] + [1 + m for m in range(M) if not live[m]] + [M + 1]  # guard rows around the outputs and the row of the dead mask
        for t in (n_hi, n_lo, area, box, bits, logits):
            assert bool((t[dead] == GUARD).all()), "case %d: a row that is not live was written" % c
        err = float(np.abs(logits[1:M + 1].double().cpu().numpy() - lg64)[live.astype(bool)].max())
        print("\n[sam_amg] case %d (%d x %d <- %s): eager fp32 on the GPU deviates %.2e from float64, eps %.2e, kernel %.2e, worst band fraction %.2e"
              % (c, oh, ow, inp, yard, eps, err, frac))
        assert err <= eps, (err, eps)
        out = dict(n_hi=n_hi[1:M + 1], n_lo=n_lo[1:M + 1], area=area[1:M + 1], box=box[1:M + 1], bits=bits[1:M + 1])
        masks = _check(out, live, lg64, thr, off, eps, ow, "case %d" % c)
        # keep decisions against the reference's, every live mask (the fixture's masks are all decided: the generator asserts it)
        assert R.stability_decided(lg64, thr, off, float(z["stability_thresh"]), eps).all()
        stab = (out["n_hi"] / out["n_lo"]).cpu().numpy()
        lv = live.astype(bool)
        assert np.array_equal((stab >= float(z["stability_thresh"]))[lv], z["c%d.keep_stability" % c][lv])
        assert np.array_equal(~R.near_crop_edge(out["box"].cpu().numpy(), (x0, y0, x1, y1), (H, W))[lv], z["c%d.keep_edge" % c][lv])
        # unpack through the C ABI: u8 and f32, the crop placed in the image, an out-of-range row gives zeros
        idx = torch.tensor([4, 0, M + 5, 3], dtype=torch.int64, device=dev)
        for f32 in (0, 1):
            o = torch.full((6, H, W), 9, dtype=torch.float32 if f32 else torch.uint8, device=dev)
            _lib.call("sam6d_amg_unpack_masks", out["bits"].data_ptr(), idx.data_ptr(), M, 4, oh, ow, x0, y0, H, W, f32,
                      o[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert bool((o[0] == 9).all()) and bool((o[5] == 9).all())
            want = R.uncrop(masks[[4, 0, 0, 3]], (x0, y0, x1, y1), (H, W))
            want[2] = False
            assert np.array_equal(o[1:5].cpu().numpy().astype(bool), want) and float(o[1:5].max()) == 1.0


@pytest.mark.parametrize("M,orig,box", [
    (1, (123, 77), (0, 0, 77, 123)),          # out_w not a multiple of 32, out_h not a multiple of the band, portrait
    (5, (203, 331), (17, 9, 316, 190)),       # an inner crop, 181 x 299
    (7, (61, 45), (0, 0, 45, 61)),            # small: many low-resolution rows per output row (a band shorter than 16)
    (192, (480, 640), (0, 0, 640, 480)),      # one full point batch at the shipped size
])
def test_amg_bindings_odd_sizes_and_batch(M, orig, box):
    from sam6d_hip import amg
    from tests.sam_amg_stub import BANK, SEEDS
    S, thr, off = 1024, 0.0, 1.0
    reps = (M + len(BANK) - 1) // len(BANK)
    params = (BANK[6:] + BANK[:6]) * reps  # starts with the all-border ellipse, the soft blob, the empty and the full mask
    uniq = R.build_logits(params[:min(M, len(BANK))], np.tile(SEEDS, reps)[:min(M, len(BANK))])
    low = np.concatenate([uniq] * reps)[:M]
    crop = (box[3] - box[1], box[2] - box[0])
    inp = R.preprocess_shape(crop[0], crop[1], S)
    lg_u = R.postprocess_masks(uniq, inp, crop, S)
    lg64 = np.concatenate([lg_u] * reps)[:M]
    eps, yard = _eps(uniq, inp, crop, S, lg_u)
    live = np.ones(M, dtype=np.uint8)
    if M > 2:
        live[[1, M - 1]] = 0
    out = amg.mask_stats(torch.from_numpy(low).to(_dev()), torch.from_numpy(live).to(_dev()), inp, crop, S, thr, off, logits=True)
    torch.cuda.synchronize()
    lv = live.astype(bool)
    err = float(np.abs(out["logits"].double().cpu().numpy() - lg64)[lv].max())
    print("\n[sam_amg] M=%d %s <- %s: eager deviates %.2e, eps %.2e, kernel %.2e" % (M, crop, inp, yard, eps, err))
    assert err <= eps
    for k in ("n_hi", "n_lo", "area", "box", "bits"):
        assert bool((out[k][torch.from_numpy(~lv).to(_dev())] == 0).all()), k  # rows that are not live keep the zeros they were given
    # white-box inputs of odd geometry need not meet the cap; the comparison rule itself is unchanged
    masks = _check(out, live, lg64, thr, off, eps, crop[1], "M=%d" % M)
    if M >= 4:
        assert masks[2].sum() == 0 and out["box"][2].tolist() == [0, 0, 0, 0]               # the empty mask
        assert masks[3].all() and out["box"][3].tolist() == [0, 0, crop[1] - 1, crop[0] - 1]  # the full mask
    if M >= 1 and crop[0] * 4 >= crop[1] * 3 - 4 and crop[1] > crop[0]:
        assert out["box"][0].tolist() == [0, 0, crop[1] - 1, crop[0] - 1] and not masks[0].all()  # touches all four borders
    idx = torch.arange(M, device=_dev())[torch.from_numpy(lv).to(_dev())]
    full = amg.unpack_masks(out["bits"], idx, crop, box, orig)
    assert full.dtype == torch.bool and np.array_equal(full.cpu().numpy(), R.uncrop(masks[lv], box, orig))


def _generator(device, **kw):
    mod = importlib.import_module("model.sam")
    from tests.sam_amg_stub import StubSam, encode_image
    return mod.CustomSamAutomaticMaskGenerator(StubSam(device), encode_image=encode_image, **kw)


def _bank_band(crop, eps):
    """Pixels of a crop where some bank mask's float64 logit is within eps of the mask threshold."""
    from tests.sam_amg_stub import bank_logits
    low = bank_logits()
    inp = R.preprocess_shape(crop[0], crop[1], 1024)
    lg = R.postprocess_masks(low, inp, crop, 1024)
    eps_here, _ = _eps(low, inp, crop, 1024, lg)
    R.check_cap(lg, (0.0, 1.0, -1.0), eps_here)
    assert R.stability_decided(lg, 0.0, 1.0, 0.85, eps_here).all()
    return R.band(lg, 0.0, eps_here).any(axis=0)


def test_generate_masks_hip_against_eager_cpu(monkeypatch):
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    ref = _generator("cpu").generate_masks(image)
    monkeypatch.setenv("SAM6D_HIP_AMG", "0")
    g_off = _generator(_dev())
    off = g_off.generate_masks(image)  # the switch: the eager tail on the GPU
    monkeypatch.delenv("SAM6D_HIP_AMG")
    g = _generator(_dev())
    g.generate_masks(image)  # warm-up: library load, allocator
    torch.cuda.synchronize()

    def flagged(gen):
        """Operations torch's sync debug mode flags in one pass: every blocking copy, host -> device uploads included."""
        prev = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode(1)
            try:
                res = gen.generate_masks(image)
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        return res, sum("called a synchronizing" in str(w.message) for w in rec)

    got, n16 = flagged(g)
    g4 = _generator(_dev(), points_per_batch=256)
    g4.generate_masks(image)
    got4, n4 = flagged(g4)
    print("\n[sam_amg] generate_masks: %d survivors of 3072 proposals; blocking copies flagged: %d with 16 batches, %d with 4"
          % (got["masks"].shape[0], n16, n4))
    # the network side uploads one batch of prompt points per batch (predict_low, as the reference's _process_batch does); everything
    # else is per crop: two 4-byte device -> host read-backs (the count after the filters, the count after NMS) and a handful of
    # small uploads (the crop's points, its box and offsets).  Nothing grows with the number of batches or masks.
    assert n16 - 16 == n4 - 4, (n16, n4)
    assert 2 <= n16 - 16 <= 10, n16
    assert torch.equal(got4["boxes"], got["boxes"]) and torch.equal(got4["masks"], got["masks"])
    assert g.predictor.model.calls == 2 * 16
    K = ref["masks"].shape[0]
    assert K >= 5 and got["masks"].dtype == torch.bool and got["boxes"].dtype == torch.int64 and got["masks"].is_cuda
    for name, other in (("hip", got), ("SAM6D_HIP_AMG=0", off)):
        assert torch.equal(other["boxes"].cpu(), ref["boxes"]), name  # same survivors, same order, same boxes
        diff = (other["masks"].cpu() != ref["masks"]).numpy()
        assert not (diff & ~_bank_band((480, 640), None)[None]).any(), name
    # the shipped configuration: width 640 on a 480 x 640 image, float masks and clamped float boxes
    g.segmentor_width_size = 640
    got2 = g.generate_masks(image)
    assert got2["masks"].dtype == torch.float32 and torch.equal(got2["masks"], got["masks"].float())
    assert torch.equal(got2["boxes"], got["boxes"].float().clamp_(min=0))


def test_generate_masks_with_one_crop_layer():
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    res = []
    for dev in ("cpu", _dev()):
        g = _generator(dev)
        g.set_crop_layers(1, 2)
        res.append(g.generate_masks(image))
        assert g.predictor.model.calls == 16 + 4 * 4  # 1024 points on the image, 256 on each of the four crops
    ref, got = res
    assert got["masks"].shape[0] >= 5 and tuple(got["masks"].shape[1:]) == (480, 640)
    assert torch.equal(got["boxes"].cpu(), ref["boxes"])
    from sam6d_hip import amg
    band = np.zeros((480, 640), dtype=bool)
    for (x0, y0, x1, y1) in amg.crop_boxes((480, 640), 1, 512 / 1500)[0]:
        band[y0:y1, x0:x1] |= _bank_band((y1 - y0, x1 - x0), None)
    diff = (got["masks"].cpu() != ref["masks"]).numpy()
    assert not (diff & ~band[None]).any()
