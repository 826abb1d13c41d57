"""ISM's reference data from a template set on the device (sam6d_hip.refdata, csrc/refdata.hip): the box and crop kernels against the
numpy restatement of tests/refdata_ref.py bit for bit, the one-pass descriptors against the float64 restatement of tests/dinov2_ref.py
within the project's rule (4 x the eager fp32 module's own error), and `refdata.build` against the route a caller has today through the
drop-in detector's scoring."""
import copy
import importlib
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sam6d_hip import dinov2, pem, refdata
from tests import dinov2_ref as DR
from tests import refdata_ref as RR
from tests._util import golden
from tests.test_dinov2_gpu import _Cfg, _mod, _randomize, _rel

pytestmark = pytest.mark.gpu

HEADS = 16
FLAVOURS = ("custom", "bop")
BOP_PADDING = (-2.1179039478302, -2.0357141494750977, -1.804444432258606)  # (0 - mean) / std in fp32, as torch on the CPU prints it


# ------------------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("size", RR.BOX_SIZES)
def test_boxes(dev, size):
    cases = [a for name, a in RR.box_cases() if name.startswith("%dx%d " % size)]
    bands = np.stack(cases)
    T, H, W = bands.shape
    want = RR.boxes(bands)
    assert T == 10 and (want[-1] == 0).all() and (want[:-1, 2] > want[:-1, 0]).all()
    d = torch.from_numpy(bands).to(dev)
    got = refdata.template_boxes(d)
    assert got.dtype == torch.int64 and got.is_cuda and got.tolist() == want.tolist()
    # the same bytes one byte off any alignment (the kernel's byte-wise head and tail), and images that do not follow one another
    flat = torch.zeros(1 + T * H * W, dtype=torch.uint8, device=dev)
    flat[1:] = d.reshape(-1)
    assert refdata.template_boxes(flat[1:].view(T, H, W)).tolist() == want.tolist()
    assert refdata.template_boxes(d[::3]).tolist() == want[::3].tolist()
    # the alpha band of an RGBA tensor, read in place: pixel stride 4, base 3 bytes into the tensor, colour in every pixel
    rgba = torch.randint(1, 256, (T, H, W, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(H)).to(dev)
    rgba[..., 3] = d
    assert refdata.template_boxes(rgba[..., 3]).tolist() == want.tolist()
    # a view whose rows do not follow one another is copied, not misread
    assert refdata.template_boxes(d.transpose(1, 2)).tolist() == RR.boxes(bands.transpose(0, 2, 1)).tolist()
    # the wrapper names the empty template
    with pytest.raises(ValueError, match=r"templates \[9\] have an empty box"):
        refdata.template_crops(rgba, rgba[..., 3])


def test_boxes_of_rendered_templates(dev):
    """512 x 512 masks as sam6d_hip.onboard.render_templates leaves them (an octahedron from three of the fixture poses)."""
    from sam6d_hip import onboard
    from tests import raster_ref
    v, f = raster_ref.octahedron()
    poses = golden("template_cam_poses")["cam_poses"][[0, 17, 41]]
    out = onboard.render_templates(dict(vertices=(v * np.float32(50.0)).astype(np.float32), faces=f), poses)
    mask = out["mask"]
    assert tuple(mask.shape) == (3, 512, 512) and mask.dtype == torch.uint8
    want = RR.boxes(mask.cpu().numpy())
    assert (want[:, 2] - want[:, 0] > 50).all()
    assert refdata.template_boxes(mask).tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------------------ crops
def _golden_boxes():
    return [tuple(int(v) for v in b) for b in golden("crop_resize_pad")["boxes"]]


@pytest.fixture(scope="module")
def scenes():
    big = _golden_boxes() + list(RR.CROP_BOXES_480x640)
    return {"480x640": (big, RR.template_scene(480, 640, big, 1)), "48x64": (list(RR.CROP_BOXES_48x64), RR.template_scene(48, 64, RR.CROP_BOXES_48x64, 2))}


@pytest.fixture(scope="module")
def restated(scenes):
    """the restatement's crops of both scenes and flavours, computed once"""
    return {(k, f): RR.template_crops(rgba[..., :3], rgba[..., 3], bxs, f) for k, (bxs, rgba) in scenes.items() for f in FLAVOURS}


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("scene", ["480x640", "48x64"])
def test_crops_bitwise(dev, scenes, restated, scene, flavour):
    bxs, rgba_np = scenes[scene]
    want_t, want_m = restated[scene, flavour]
    rgba = torch.from_numpy(rgba_np).to(dev)
    alpha = rgba[..., 3]  # a view: pixel stride 4
    got_t, got_m = refdata.template_crops(rgba[..., :3].contiguous(), alpha.contiguous(), flavour=flavour)  # (T,H,W,3) and (T,H,W)
    assert got_t.dtype == got_m.dtype == torch.float32 and tuple(got_t.shape) == (len(bxs), 3, 224, 224) and tuple(got_m.shape) == (len(bxs), 224, 224)
    gt, gm = got_t.cpu().numpy(), got_m.cpu().numpy()
    for t in range(len(bxs)):  # every template
        assert np.array_equal(gt[t], want_t[t]), ("rgb", t, bxs[t])
        assert np.array_equal(gm[t], want_m[t]), ("mask", t, bxs[t])
    # the RGBA tensor read in place (colours at pixel stride 4, the alpha band as the mask), and its three-channel view
    for rgb in (rgba, rgba[..., :3]):
        t4, m4 = refdata.template_crops(rgb, alpha, flavour=flavour)
        assert torch.equal(t4, got_t) and torch.equal(m4, got_m)
    # the kernel's boxes are the intended ones, and passing them in changes nothing
    kb = refdata.template_boxes(alpha)
    assert kb.tolist() == [list(b) for b in bxs]
    for given in (kb, torch.tensor(bxs, dtype=torch.int32, device=dev)):
        t5, m5 = refdata.template_crops(rgba, alpha, boxes=given, flavour=flavour)
        assert torch.equal(t5, got_t) and torch.equal(m5, got_m)
    # the plain-torch partner on the device
    te, me = refdata.eager_template_crops(rgba, alpha, flavour=flavour)
    assert torch.equal(me, got_m) and tuple(te.shape) == tuple(got_t.shape)
    if flavour == "custom":  # (bop divides by std on the device: torch's own fp32 division there is not part of this contract)
        assert torch.equal(te, got_t)
    thin = 3 if scene == "480x640" else 2  # a one-pixel-wide box: padding left and right
    assert gm[thin][0, 0] == 0.0
    if flavour == "bop":
        assert gt[thin][:, 0, 0].tolist() == list(BOP_PADDING) and gt[thin][:, 223, 223].tolist() == list(BOP_PADDING)
    else:
        assert gt[thin][:, 0, 0].tolist() == [0.0, 0.0, 0.0]


def test_check_false_reads_nothing_back(dev, scenes):
    """torch's sync debug mode flags every blocking copy: none with check=False (boxes from the kernel or passed in), at least the one
    read-back of the boxes with check=True.  An empty box then gives an all-padding crop instead of an error."""
    bxs, rgba_np = scenes["48x64"]
    rgba = torch.from_numpy(rgba_np).to(dev)
    rgba[2, ..., 3] = 0  # one empty template
    alpha = rgba[..., 3]
    given = refdata.template_boxes(alpha)
    refdata.template_crops(rgba, alpha, check=False)  # warm-up: library load, allocator
    torch.cuda.synchronize()

    def flagged(fn):
        prev = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode(1)
            try:
                res = fn()
            except ValueError as e:
                res = e
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        return res, sum("called a synchronizing" in str(w.message) for w in rec)

    (t0, m0), n0 = flagged(lambda: refdata.template_crops(rgba, alpha, check=False))
    (t1, m1), n1 = flagged(lambda: refdata.template_crops(rgba, alpha, boxes=given, flavour="bop", check=False))
    err, n2 = flagged(lambda: refdata.template_crops(rgba, alpha, check=True))
    print("\n[refdata] blocking copies flagged: check=False %d and %d, check=True %d" % (n0, n1, n2))
    assert n0 == 0 and n1 == 0
    assert n2 >= 1 and isinstance(err, ValueError) and "templates [2]" in str(err)
    assert float(t0[2].abs().max()) == 0.0 and float(m0[2].abs().max()) == 0.0 and float(m1[2].abs().max()) == 0.0
    assert t1[2, :, 5, 7].tolist() == list(BOP_PADDING) and float(t0[1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ descriptors
def _templates(n_obj, views, seed, H=96, W=128):
    """n_obj textured objects, `views` shifted and rescaled views of each: rgb (T,H,W,3) u8 and mask (T,H,W) u8 of 0 / 255 (a disc
    or a rectangle per object), object by object."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rgb = torch.randint(0, 40, (n_obj * views, H, W, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros(n_obj * views, H, W, dtype=torch.uint8)
    for o in range(n_obj):
        for k in range(views):
            t = o * views + k
            fq = 0.12 + 0.17 * o + 0.045 * k
            gain = torch.tensor((1.0, 0.55, 0.2) if o % 2 == 0 else (0.2, 0.6, 1.0))  # the objects differ in colour, the views in texture
            tex = (torch.stack([127 + 120 * torch.sin(fq * xx + o + 0.9 * k), 127 + 120 * torch.cos(fq * yy * (o + 1)),
                                127 + 120 * torch.sin(fq * (xx + (1 - 2 * o) * yy))], -1) * gain * (1.0 - 0.13 * k)).to(torch.uint8)
            cx, cy, r = 50 + 4 * k + 10 * o, 44 + 2 * k, 24 + 3 * k
            inside = (((xx - cx) / (1.4 * r)) ** 2 + ((yy - cy) / r) ** 2 <= 1.0) if o % 2 == 0 else ((xx - cx).abs() <= 1.3 * r) & ((yy - cy).abs() <= 0.8 * r)
            mask[t][inside] = 255
            rgb[t][inside] = tex[inside]
    return rgb, mask


@pytest.fixture(scope="module")
def model():
    return _randomize(_mod().DinoVisionTransformer(), 1).eval()


def _references(model, dev, crops, m224):
    """float64 restatement and eager fp32 module on the same crops -> (cls64, keep, patch64), (cls32, patch32)"""
    sd64 = DR.to_dtype(model.state_dict(), torch.float64, dev)
    parts = [DR.forward(sd64, crops[i:i + 6].double(), HEADS) for i in range(0, crops.shape[0], 6)]
    cls64, tok64 = torch.cat([p[0] for p in parts]).cpu(), torch.cat([p[1] for p in parts]).cpu()
    keep, patch64 = DR.masked_patch_features(tok64, m224.double().cpu())
    m32 = copy.deepcopy(model).to(dev)
    with torch.no_grad():
        f = m32.forward_features(crops)
    _, patch32 = DR.masked_patch_features(f["x_norm_patchtokens"].cpu(), m224.cpu())
    return (cls64, keep, patch64), (f["x_norm_clstoken"].cpu(), patch32)


@pytest.fixture(scope="module")
def six(model, dev):
    """T = 6 templates (2 objects x 3 views), their device crops and the two references, shared by both matmul modes"""
    rgb, mask = (t.to(dev) for t in _templates(2, 3, 31))
    crops, m224 = refdata.template_crops(rgb, mask)
    return rgb, mask, _references(model, dev, crops, m224)


@pytest.mark.parametrize("mode", [1, 0])
def test_descriptors_vs_float64(model, six, dev, mode):
    """Bound: the project's rule of tests/test_dinov2_gpu.py -- within 4 x the eager fp32 module's own error against the same float64
    restatement, measured here on the same crops.  The kept-patch sets are identical."""
    rgb, mask, ((cls64, keep, patch64), (cls32, patch32)) = six
    W = dinov2.DinoWeights(model.state_dict(), dev, options=pem.Options(matmul_mode=mode))
    out = refdata.descriptors(rgb, mask, W, n_objects=2)
    assert set(out) == {"descriptors", "appe_descriptors"}
    d, a = out["descriptors"], out["appe_descriptors"]
    assert tuple(d.shape) == (2, 3, 1024) and tuple(a.shape) == (2, 3, 256, 1024) and torch.isfinite(d).all() and torch.isfinite(a).all()
    a = a.reshape(6, 256, 1024).cpu()
    assert torch.equal(a.abs().amax(-1) > 0, keep) and 0 < int(keep.sum()) < keep.numel()
    assert float(a[~keep].abs().max()) == 0.0
    c, ce = _rel(d.reshape(6, 1024).cpu(), cls64), _rel(cls32, cls64)
    p, pe = _rel(a[keep], patch64[keep]), _rel(patch32[keep], patch64[keep])
    print("\n[refdata] descriptors mode %d: cls HIP %.3e eager %.3e | patch HIP %.3e eager %.3e" % (mode, c, ce, p, pe))
    assert c <= 4.0 * ce, ("cls", c, ce)
    assert p <= 4.0 * pe, ("patch", p, pe)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_build_against_todays_route(dev):
    """ref_data from refdata.build against the route a caller has today (masks to the host, PIL getbbox, the drop-in CropResizePad
    twice, compute_features + compute_masked_patch_feature: two encoder passes), both through the drop-in detector's
    compute_semantic_score and compute_appearance_score on one seeded proposal set: same selected proposals, objects and best
    templates, scores within the descriptor bound (4 x the eager fp32 module's error on these crops, measured here).  The proposal set
    is first checked with today's route alone: no score within ten bounds (and 1e-3) of the threshold or of a tie."""
    from PIL import Image
    from utils.bbox_utils import CropResizePad
    mod, loss, det = _mod(), importlib.import_module("model.loss"), importlib.import_module("model.detector")
    d = mod.CustomDINOv2("dinov2_vitl14", "x_norm_clstoken", 224, 16, 512, "unused")
    _randomize(d.model, 9)
    d.eval()
    d.model.to(dev)
    n_obj, views, thresh = 2, 6, 0.2
    T = n_obj * views
    rgb, mask = (t.to(dev) for t in _templates(n_obj, views, 41))
    g = np.random.default_rng(7)
    obj_poses = g.normal(size=(T, 4, 4)) * 100.0
    model_points = g.normal(size=(n_obj, 64, 3)).astype(np.float32)

    # -- today's route (ISM/run_inference_custom.py:132-163 with the drop-in's classes)
    boxes, masks, templates = [], [], []
    rgb_h, mask_h = rgb.cpu().numpy(), mask.cpu().numpy()
    for t in range(T):
        m = Image.fromarray(mask_h[t], "L")
        boxes.append(m.getbbox())
        image = torch.from_numpy(rgb_h[t] / 255).float()
        mk = torch.from_numpy(np.array(m) / 255).float()
        templates.append(image * mk[:, :, None])
        masks.append(mk.unsqueeze(-1))
    templates = torch.stack(templates).permute(0, 3, 1, 2)
    masks = torch.stack(masks).permute(0, 3, 1, 2)
    boxes = torch.tensor(np.array(boxes))
    proc = CropResizePad(224)
    templates, masks_cropped = proc(images=templates, boxes=boxes).to(dev), proc(images=masks, boxes=boxes).to(dev)
    today = {"descriptors": d.compute_features(templates, token_name="x_norm_clstoken").reshape(n_obj, views, 1024),
             "appe_descriptors": d.compute_masked_patch_feature(templates, masks_cropped[:, 0]).reshape(n_obj, views, 256, 1024)}

    # -- the device route
    ref = refdata.build(rgb, mask, d._weights(dev), obj_poses, model_points, n_objects=n_obj)
    assert set(ref) == {"descriptors", "appe_descriptors", "poses", "pointcloud"} and all(v.is_cuda for v in ref.values())
    assert tuple(ref["descriptors"].shape) == (n_obj, views, 1024) and tuple(ref["appe_descriptors"].shape) == (n_obj, views, 256, 1024)
    assert torch.equal(ref["pointcloud"].cpu(), torch.from_numpy(model_points))
    assert np.array_equal(ref["poses"].cpu().numpy(), refdata.reference_poses(obj_poses)) and ref["poses"].dtype == torch.float32
    crops, m224 = refdata.template_crops(rgb, mask)
    assert torch.equal(crops, templates) and torch.equal(m224, masks_cropped[:, 0])  # the encoder sees the same crops on both routes

    # -- the descriptor bound on these crops
    (cls64, keep, patch64), (cls32, patch32) = _references(d.model, dev, crops, m224)
    bound = 4.0 * max(_rel(cls32, cls64), _rel(patch32[keep], patch64[keep]))

    # -- one seeded proposal set: noisy copies of templates of both objects, and two proposals that match nothing
    gt = torch.Generator().manual_seed(5)
    picks = [(0, 1), (1, 4), (0, 5), (1, 0), (0, 3), (1, 2)]
    tc, tp = today["descriptors"].cpu(), today["appe_descriptors"].cpu()
    q, qp = [], []
    for o, k in picks:
        c = tc[o, k]
        q.append(c + 0.1 * c.norm() / 32.0 * torch.randn(1024, generator=gt))
        p = tp[o, k]
        qp.append(F.normalize(p + (p.abs().amax(-1, keepdim=True) > 0) * 0.3 / 32.0 * torch.randn(256, 1024, generator=gt), dim=-1))
    for _ in range(2):
        q.append(torch.randn(1024, generator=gt))
        qp.append(F.normalize(torch.randn(256, 1024, generator=gt), dim=-1))
    q, qp = torch.stack(q).to(dev), torch.stack(qp).to(dev)

    # today's route alone: nothing near the threshold or a tie
    margin = max(1e-3, 10.0 * bound)
    sim = torch.einsum("qd,otd->qot", F.normalize(q.double().cpu(), dim=-1), F.normalize(tc.double(), dim=-1)).clamp(0.0, 1.0)
    agg = sim.topk(5, dim=-1)[0].mean(-1)
    top2 = agg.topk(2, dim=-1)[0]
    assert (top2[:6, 0] > thresh).all() and (top2[6:, 0] < thresh).all()  # the six copies are selected, the two others are not
    obj_want = agg.argmax(-1)
    t2 = sim[torch.arange(len(q)), obj_want].topk(2, dim=-1)[0]
    gaps = (float((top2[:, 0] - thresh).abs().min()), float((top2[:6, 0] - top2[:6, 1]).min()), float((t2[:6, 0] - t2[:6, 1]).min()))
    print("\n[refdata] end to end: bound %.3e; today's margins: threshold %.3e, objects %.3e, templates %.3e" % ((bound,) + gaps))
    assert gaps[0] > margin, "semantic score too close to the threshold"
    assert gaps[1] > margin, "object arg-max too close to a tie"
    assert gaps[2] > margin, "best template too close to a tie"

    m = det.Instance_Segmentation_Model(segmentor_model=None, descriptor_model=d, onboarding_config=None,
                                        matching_config=_Cfg(metric=loss.PairwiseSimilarity("cosine", 16), aggregation_function="avg_5",
                                                             confidence_thresh=thresh),
                                        post_processing_config=None, log_interval=5, log_dir=".", visible_thred=0.5, pointcloud_sample_num=2048)

    def score(ref_data):
        m.ref_data = ref_data
        sel, obj, sem, best = m.compute_semantic_score(q)
        a, _ = m.compute_appearance_score(best, obj, qp[sel].contiguous())
        return sel.cpu(), obj.cpu(), sem.cpu(), best.cpu(), a.cpu()

    s_t, s_d = score(today), score(ref)
    assert s_t[0].tolist() == [0, 1, 2, 3, 4, 5] and s_t[1].tolist() == [o for o, _ in picks] and s_t[3].tolist() == [k for _, k in picks]
    for i, name in ((0, "selected proposals"), (1, "object ids"), (3, "best templates")):
        assert torch.equal(s_t[i], s_d[i]), name
    for i, name in ((2, "semantic score"), (4, "appearance score")):
        e = float((s_t[i] - s_d[i]).abs().max())
        print("[refdata] end to end %s: max |device route - today's route| = %.3e (bound %.3e)" % (name, e, bound))
        assert e <= bound, (name, e, bound)
