"""ISM's reference data from a template set (sam6d_hip.refdata, csrc/refdata.hip) without a GPU: the numpy restatement
(tests/refdata_ref.py) against the installed Pillow and against the composition of parts already pinned to the reference, the plain-torch
partner against the restatement, the pose recipe, what is refused, the import layer and the kernels' registers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dinov2_ref as DR
from tests import refdata_ref as RR
from tests._util import PKG, golden

FLAVOURS = ("custom", "bop")


def _golden_boxes():
    return [tuple(int(v) for v in b) for b in golden("crop_resize_pad")["boxes"]]


@pytest.fixture(scope="module")
def scenes():
    """the two template sets of the GPU tests (tests/test_refdata_gpu.py), as numpy rgba"""
    big = _golden_boxes() + list(RR.CROP_BOXES_480x640)
    return {"480x640": (big, RR.template_scene(480, 640, big, 1)), "48x64": (list(RR.CROP_BOXES_48x64), RR.template_scene(48, 64, RR.CROP_BOXES_48x64, 2))}


# ------------------------------------------------------------------------------------------------------------ 1. the box rule
def test_box_rule_is_pils_getbbox():
    """refdata_ref.getbbox equals Image.getbbox() on every box test image; PIL's None is (0,0,0,0) here.  On an RGBA image the
    installed Pillow (12.x) takes the box of the ALPHA band alone (getbbox(alpha_only=True) is its default): a pixel that has colour
    but alpha 0 does not count, and an image with colour everywhere and alpha 0 everywhere gives None -- so the alpha band is what
    template_boxes is given for BOP templates (ISM/provider/bop.py:66)."""
    from PIL import Image
    cases = RR.box_cases()
    assert len(cases) == 10 * len(RR.BOX_SIZES)
    for name, a in cases:
        want = Image.fromarray(a, "L").getbbox()
        got = RR.getbbox(a)
        assert got == ((0, 0, 0, 0) if want is None else want), name
        assert (want is None) == name.endswith("empty"), name
    g = np.random.default_rng(0)
    for name, a in cases:
        rgba = g.integers(1, 256, a.shape + (4,), dtype=np.uint8)  # colour in every pixel
        rgba[..., 3] = a
        want = Image.fromarray(rgba, "RGBA").getbbox()
        assert RR.getbbox(rgba[..., 3]) == ((0, 0, 0, 0) if want is None else want), name
    assert (RR.boxes(np.stack([c[1] for c in cases[:10]])) == np.array([RR.getbbox(c[1]) for c in cases[:10]])).all()


def test_scene_boxes_are_the_intended_ones(scenes):
    from PIL import Image
    for bxs, rgba in scenes.values():
        assert RR.boxes(rgba[..., 3]).tolist() == [list(b) for b in bxs]
        for t in (0, len(bxs) - 1):
            assert Image.fromarray(rgba[t, ..., 3], "L").getbbox() == tuple(bxs[t])
        ring = rgba[0, ..., 3][bxs[0][1], bxs[0][0]:bxs[0][2]]
        assert ((ring > 0) & (ring < 255)).all() and set(np.unique(rgba[0, ..., 3][bxs[0][1] + 1:bxs[0][3] - 1, bxs[0][0] + 1:bxs[0][2] - 1])) <= {0, 255}


def test_u8_over_255_is_the_fp32_division():
    """np.array(u8) / 255 is float64 and .float() rounds it once more: for all 256 values that is the plain fp32 division the kernel
    and the restatement write."""
    x = np.arange(256, dtype=np.uint8)
    assert ((x / 255).astype(np.float32) == x.astype(np.float32) / np.float32(255)).all()
    assert torch.equal(torch.from_numpy(x / 255).float(), torch.from_numpy(x).float() / 255)


# ------------------------------------------------------------------------------------------------------------ 2. the crops
def _composition(rgba, flavour):
    """The reference block from parts already pinned: PIL's getbbox, tests/dinov2_ref.crop_resize_pad and the literal torch operations
    of run_inference_custom.py:136-155 / bop.py:66-83."""
    from PIL import Image
    boxes, masks, templates = [], [], []
    for t in range(rgba.shape[0]):
        alpha = Image.fromarray(rgba[t, ..., 3], "L")
        boxes.append(alpha.getbbox())
        image = torch.from_numpy(np.array(Image.fromarray(rgba[t, ..., :3].copy(), "RGB")) / 255).float()
        mask = torch.from_numpy(np.array(alpha) / 255).float()
        if flavour == "custom":
            image = image * mask[:, :, None]
        templates.append(image)
        masks.append(mask.unsqueeze(-1))
    templates = torch.stack(templates).permute(0, 3, 1, 2)
    masks = torch.stack(masks).permute(0, 3, 1, 2)
    boxes = torch.tensor(np.array(boxes))
    templates = DR.crop_resize_pad(templates, boxes)
    if flavour == "bop":  # T.Normalize: sub_(mean).div_(std)
        mean = torch.tensor(DR.MEAN, dtype=torch.float32)[:, None, None]
        std = torch.tensor(DR.STD, dtype=torch.float32)[:, None, None]
        templates = templates.sub(mean).div(std)
    return templates, DR.crop_resize_pad(masks, boxes)[:, 0]


@pytest.fixture(scope="module")
def restated(scenes):
    """the restatement's crops of both scenes and flavours, shared by the tests below"""
    return {(k, f): RR.template_crops(rgba[..., :3], rgba[..., 3], RR.boxes(rgba[..., 3]), f) for k, (_, rgba) in scenes.items() for f in FLAVOURS}


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("scene", ["480x640", "48x64"])
def test_restatement_is_the_composition(scenes, restated, scene, flavour):
    want_t, want_m = _composition(scenes[scene][1], flavour)
    got_t, got_m = restated[scene, flavour]
    for t in range(len(want_t)):
        assert np.array_equal(got_t[t], want_t[t].numpy()), ("rgb", t, scenes[scene][0][t])
        assert np.array_equal(got_m[t], want_m[t].numpy()), ("mask", t, scenes[scene][0][t])
    if flavour == "bop":  # Normalize after the padding
        t = 3 if scene == "480x640" else 2  # a one-pixel-wide box: padding left and right
        pad = got_t[t][:, 0, 0]
        assert pad.tolist() == [-2.1179039478302, -2.0357141494750977, -1.804444432258606], pad.tolist()


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("scene", ["480x640", "48x64"])
def test_eager_partner_is_the_restatement(scenes, restated, scene, flavour):
    from sam6d_hip import refdata
    rgba = torch.from_numpy(scenes[scene][1])
    want_t, want_m = restated[scene, flavour]
    for rgb in (rgba[..., :3], rgba):  # a three-channel view and the four-channel tensor
        got_t, got_m = refdata.eager_template_crops(rgb, rgba[..., 3], flavour=flavour)
        assert np.array_equal(got_t.numpy(), want_t) and np.array_equal(got_m.numpy(), want_m)
    got_t2, _ = refdata.eager_template_crops(rgba, rgba[..., 3], boxes=torch.tensor(scenes[scene][0]), flavour=flavour)
    assert np.array_equal(got_t2.numpy(), want_t)
    assert (refdata.host_boxes(rgba[..., 3]) == RR.boxes(scenes[scene][1][..., 3])).all()


# ------------------------------------------------------------------------------------------------------------ 4. poses
def test_reference_poses():
    from sam6d_hip import refdata
    g = np.random.default_rng(3)
    poses = g.normal(size=(42, 4, 4)) * 300.0
    keep = poses.copy()
    want = poses.copy()
    want[:, :3, 3] *= 0.4
    want = torch.tensor(want).to(torch.float32).numpy()
    got = refdata.reference_poses(poses)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(poses, keep)
    idx = [5, 0, 41, 7]
    assert np.array_equal(refdata.reference_poses(poses, idx), want[idx])
    f32 = poses.astype(np.float32)
    w32 = f32.astype(np.float64)
    w32[:, :3, 3] *= 0.4
    assert np.array_equal(refdata.reference_poses(f32), w32.astype(np.float32))  # float64 first, whatever comes in
    with pytest.raises(ValueError, match="obj_poses"):
        refdata.reference_poses(np.zeros((4, 4)))


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_argument_errors():
    from sam6d_hip import refdata
    rgb, mask = torch.zeros(6, 8, 9, 3, dtype=torch.uint8), torch.ones(6, 8, 9, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        refdata.template_boxes(mask)
    with pytest.raises(RuntimeError, match="HIP device"):
        refdata.template_crops(rgb, mask)
    with pytest.raises(RuntimeError, match="HIP device"):
        refdata.descriptors(rgb, mask, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        refdata.build(rgb, mask, None, np.zeros((6, 4, 4)), np.zeros((16, 3)))
    for fn in (refdata.template_crops, refdata.eager_template_crops):
        with pytest.raises(ValueError, match="mask must be"):
            fn(rgb, mask.float())
        with pytest.raises(ValueError, match="rgb must be"):
            fn(rgb.float(), mask)
        with pytest.raises(ValueError, match="rgb must be"):
            fn(rgb[..., :2], mask)
        with pytest.raises(ValueError, match="differ"):
            fn(rgb, mask[:, :, :8])
        with pytest.raises(ValueError, match="unknown flavour"):
            fn(rgb, mask, flavour="imagenet")
    with pytest.raises(ValueError, match="band must be"):
        refdata.template_boxes(mask.float())
    with pytest.raises(ValueError, match="band must be"):
        refdata.template_boxes(mask[0])
    with pytest.raises(ValueError, match="boxes must be"):
        refdata.template_crops(rgb, mask, boxes=torch.zeros(6, 4))
    with pytest.raises(ValueError, match="boxes must be"):
        refdata.template_crops(rgb, mask, boxes=torch.zeros(5, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="n_objects = 4"):
        refdata.descriptors(rgb, mask, None, n_objects=4)
    with pytest.raises(ValueError, match="unknown flavour"):
        refdata.descriptors(rgb, mask, None, flavour="imagenet")
    empty = mask.clone()
    empty[[1, 4]] = 0
    with pytest.raises(ValueError, match=r"templates \[1, 4\] have an empty box"):
        refdata.eager_template_crops(rgb, empty)


def test_c_entries_refuse_by_name_before_a_launch():
    from sam6d_hip import _lib

    def boxes(T=1, H=8, W=8, ps=1, ims=64, ptr=64):  # (refused before a pointer is followed: 64 stands for "not null")
        _lib.call("sam6d_template_boxes", ptr, T, H, W, ps, ims, ptr, None)

    for kw, name in ((dict(ptr=None), "null pointer"), (dict(T=65536), "T <= 65535"), (dict(T=-1), "T <= 65535"), (dict(H=0), "bad image size"),
                     (dict(H=1 << 15, W=1 << 15), "bad image size"), (dict(ps=0), "bad strides"), (dict(ps=65), "bad strides"),
                     (dict(ims=-1), "bad strides")):
        with pytest.raises(RuntimeError, match="template_boxes: " + name):
            boxes(**kw)

    def crops(T=1, H=8, W=8, flavour=0, rgb=64, rps=3, rims=192, mask=64, mps=1, mims=64, bx=64, out=64, om=64):
        _lib.call("sam6d_template_crops", rgb, rps, rims, mask, mps, mims, bx, T, H, W, flavour, out, om, None)

    for kw, name in ((dict(flavour=2), "unknown flavour 2"), (dict(bx=None), "null pointer"), (dict(out=None, om=None), "null pointer"),
                     (dict(rgb=None), "null pointer"), (dict(mask=None), r"null pointer \(mask\)"),
                     (dict(mask=None, flavour=1), r"null pointer \(mask\)"), (dict(T=65536), "T <= 65535"), (dict(W=0), "bad image size"),
                     (dict(rps=2), "bad rgb strides"), (dict(rims=-1), "bad rgb strides"), (dict(mps=0), "bad mask strides"),
                     (dict(mims=-4), "bad mask strides")):
        with pytest.raises(RuntimeError, match="template_crops: " + name):
            crops(**kw)


# ------------------------------------------------------------------------------------------------------------ 6. import layer
def test_module_imports_without_the_pipeline(tmp_path):
    """tests/test_import_layers_host.py's rule for the new module: importable without the shared library, without sam6d_hip.pem and
    without PIL; the package itself does not import it."""
    child = ("import sys; sys.path.insert(0, %r)\nimport sam6d_hip\nassert 'sam6d_hip.refdata' not in sys.modules\nimport sam6d_hip.refdata\n"
             "print(' '.join(sorted(m for m in sys.modules if m == 'sam6d_hip' or m.startswith('sam6d_hip.') or m in ('PIL', 'cv2', 'trimesh'))))\n")
    env = dict(os.environ, SAM6D_LIB=str(tmp_path / "no_such_library.so"))
    r = subprocess.run([sys.executable, "-c", child % PKG], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    loaded = set(r.stdout.split())
    assert "sam6d_hip.refdata" in loaded and "sam6d_hip.pem" not in loaded and "PIL" not in loaded, sorted(loaded)
    assert loaded == {"sam6d_hip", "sam6d_hip._lib", "sam6d_hip.runtime", "sam6d_hip.ops", "sam6d_hip.encoder", "sam6d_hip.ism",
                      "sam6d_hip.dinov2", "sam6d_hip.refdata"}, sorted(loaded)


def test_load_templates_round_trip(tmp_path):
    from PIL import Image
    from sam6d_hip import refdata
    g = np.random.default_rng(5)
    rgb = g.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    mask = (g.random((3, 9, 11)) < 0.5).astype(np.uint8) * 255
    for i in range(3):
        Image.fromarray(rgb[i], "RGB").save(tmp_path / ("rgb_%d.png" % i))
        Image.fromarray(mask[i], "L").save(tmp_path / ("mask_%d.png" % i))
    got_rgb, got_mask = refdata.load_templates(str(tmp_path), device="cpu")
    assert got_rgb.dtype == torch.uint8 and np.array_equal(got_rgb.numpy(), rgb) and np.array_equal(got_mask.numpy(), mask)
    with pytest.raises(ValueError, match="no rgb_"):
        refdata.load_templates(str(tmp_path / "nothing"))


# ------------------------------------------------------------------------------------------------------------ 7. kernels
def test_kernel_resources():
    """neither new kernel uses scratch or spills, and each keeps within its built VGPR count rounded up to
    the next step of 8 (built: tpl_bbox 22, tpl_crop<custom> 20, tpl_crop<bop> 20).  The code object holds these kernels alone."""
    from tests._util import kernel_resources
    limits = {"tpl_bbox_kernel": 24, "tpl_crop_kernelILb0EE": 24, "tpl_crop_kernelILb1EE": 24}
    found = kernel_resources(b"tpl_bbox_kernel", r"(\w+?_kernel(?:ILb[01]EE)?)")
    print("\n[refdata] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
