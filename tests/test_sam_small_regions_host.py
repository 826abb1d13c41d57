"""Host-side checks of the min_mask_region_area clean-up (no GPU): the numpy restatement tests/small_regions_ref.py against the stored
fixture (tests/golden/sam_small_regions.npz, written with scipy by tests/gen_sam_small_regions_golden.py), against scipy and cv2 where
they import, the bindings, the CPU-tensor contract, the kernels' resources and the drop-in's unchanged signature and host route."""
import importlib
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tests import small_regions_ref as R
from tests._util import ROOT, golden

SYMBOLS = ("sam6d_mask_components", "sam6d_mask_components_workspace_bytes", "sam6d_amg_small_regions", "sam6d_amg_small_regions_workspace_bytes")


def _sets():
    g = golden("sam_small_regions")
    for j in range(int(g["n_sets"])):
        p = "s%d." % j
        H, W = (int(v) for v in g[p + "shape"])
        names = [str(n) for n in g[p + "names"]]
        masks = np.unpackbits(g[p + "bits"], axis=1)[:, :H * W].reshape(len(names), H, W).astype(bool)
        yield g, p, (H, W), names, masks


def test_restatement_against_the_fixture():
    n_cases = 0
    for g, p, (H, W), names, masks in _sets():
        for k, m in enumerate(masks):
            assert len(R.components(m)[2]) == g[p + "n_fg"][k] and len(R.components(~m)[2]) == g[p + "n_bg"][k], (H, W, names[k])
        for t in g[p + "min_areas"]:
            q = p + "t%d." % t
            want = np.unpackbits(g[q + "cleaned"], axis=1)[:, :H * W].reshape(len(names), H, W).astype(bool)
            cleaned, changed, boxes = R.clean_batch(masks, int(t))
            for k in range(len(names)):
                assert np.array_equal(cleaned[k], want[k]), (H, W, names[k], int(t))
            assert np.array_equal(changed, g[q + "changed"]) and np.array_equal(boxes, g[q + "boxes"]), (H, W, int(t))
            n_cases += len(names)
    assert n_cases >= 100


def test_fixture_inputs_are_the_generators_patterns():
    """The GPU tests build their inputs with the generators; the fixture pins what those produced when it was written."""
    seeds = {(70, 130): 200, (129, 191): 320, (480, 640): 11}
    for g, p, shape, names, masks in _sets():
        pats = R.patterns(shape[0], shape[1], seeds[shape])
        for k, n in enumerate(names):
            assert np.array_equal(masks[k], pats[n]), (shape, n)


def test_pattern_properties():
    for H, W in ((33, 65), (70, 130)):
        p = R.patterns(H, W, 1)
        count = lambda m: len(R.components(m)[2])  # noqa: E731
        assert count(p["checkerboard"]) == 1 and count(~p["checkerboard"]) == 1      # 8-connectivity; 4-connectivity gives H W / 2
        assert count(p["serpentine"]) == 1 and count(p["comb"]) == 1 and count(p["diagonal"]) == 1
        assert count(~p["diagonal"]) == 1                                            # the staircase does not cut the image under 8-connectivity
        assert count(p["lattice"]) == ((H + 1) // 2) * ((W + 1) // 2) and count(~p["lattice"]) == 1
        assert p["serpentine"].sum() == ((H + 1) // 2) * W + H // 2                    # a path: full rows and one connector per gap
        labels, areas, first, size = R.components(p["blobs"])
        assert size.sum() == p["blobs"].sum() and (np.diff(first) > 0).all() and labels.max() == first.max() + 1
        assert abs(p["blobs"].mean() - 0.5) < 0.01 and abs(p["coin"].mean() - 0.5) < 0.05


def test_restatement_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in ((70, 130), (129, 191), (480, 640)):
        pats = R.patterns(H, W, 5)
        for name in (("blobs", "coin") if H == 480 else tuple(pats)):
            for m in (pats[name], ~pats[name]):
                lab, n = ndimage.label(m, structure=R.NEIGHBOURS_8)
                labels, areas, first, size = R.components(m)
                assert len(first) == n, (H, W, name)
                # the same partition: scipy's label of a component's first pixel names all of its pixels, and the sizes agree
                ids = lab.ravel()[first]
                assert len(np.unique(ids)) == n
                table = np.zeros(n + 1, dtype=np.int64)
                table[ids] = first + 1
                assert np.array_equal(table[lab], labels), (H, W, name)
                assert np.array_equal(np.bincount(lab.ravel(), minlength=n + 1)[ids], size)


def _host_route(masks, boxes, min_area, nms_thresh):
    mod = importlib.import_module("model.sam")
    data = {"masks": torch.from_numpy(masks), "boxes": torch.from_numpy(boxes)}
    return mod.CustomSamAutomaticMaskGenerator.postprocess_small_regions(data, min_area, nms_thresh)


def _some_masks():
    H, W = 70, 130
    p = R.patterns(H, W, 9)
    masks = np.stack([p["blobs"], p["coin"], p["comb"], np.roll(p["blobs"], 17, axis=1), p["ones"], p["zeros"], p["lattice"]])
    boxes = np.array([R.mask_box(m) for m in masks], dtype=np.int64) + 500
    return masks, boxes


def test_restatement_against_cv2_through_the_dropins_host_route():
    pytest.importorskip("cv2")
    masks, boxes = _some_masks()
    for t in (1, 2, 20, 100, 70 * 130 + 1):
        out = _host_route(masks, boxes, t, 0.7)
        want_m, want_b, _ = R.postprocess(masks, boxes, t, 0.7)
        assert torch.equal(out["masks"], torch.from_numpy(want_m)) and torch.equal(out["boxes"], torch.from_numpy(want_b)), t


def test_dropins_host_route_is_unchanged_on_the_cpu(monkeypatch):
    """CPU tensors take the reference's host route whatever SAM6D_HIP_AMG says, and that route still asks cv2 for the labels: with a
    stand-in cv2 that labels through the restatement it returns the restatement's result; without cv2 it raises ImportError."""
    masks, boxes = _some_masks()

    def connected(work, connectivity):
        assert connectivity == 8 and work.dtype == np.uint8
        labels, _, first, size = R.components(work != 0)
        regions = np.searchsorted(first + 1, labels, side="right") * (labels > 0)
        stats = np.zeros((len(size) + 1, 5), dtype=np.int32)
        stats[1:, -1] = size
        stats[0, -1] = (work == 0).sum()
        return len(size) + 1, regions.astype(np.int32), stats, None

    from sam6d_hip import amg
    monkeypatch.setattr(amg, "postprocess_small_regions", lambda *a: pytest.fail("the library route was taken for CPU tensors"))
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(connectedComponentsWithStats=connected))
    for t in (2, 20, 70 * 130 + 1):
        out = _host_route(masks, boxes, t, 0.7)
        want_m, want_b, _ = R.postprocess(masks, boxes, t, 0.7)
        assert torch.equal(out["masks"], torch.from_numpy(want_m)) and torch.equal(out["boxes"], torch.from_numpy(want_b)), t
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError):
        _host_route(masks, boxes, 20, 0.7)


def test_header_declares_and_lib_binds_the_entries():
    import ctypes
    from sam6d_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "sam6d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), "%s is not declared in sam6d_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["sam6d_mask_components"]) == 10 and len(_lib.SIGNATURES["sam6d_amg_small_regions"]) == 10
    for name in ("sam6d_mask_components", "sam6d_amg_small_regions"):
        comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*size_t\s+%s_workspace_bytes" % name, hdr, flags=re.S).group(1)
        assert "amg.py:267-291" in comment, "%s: its comment does not cite the reference" % name
    load = _lib.load()
    assert load.sam6d_amg_small_regions_workspace_bytes(3, 70, 130) >= 3 * 70 * 130 * 8
    assert load.sam6d_mask_components_workspace_bytes(3, 70, 130) == 3 * 70 * 130 * 8
    for bad in ((0, 70, 130), (65536, 70, 130), (1, 0, 130), (1, 65536, 32768)):
        assert load.sam6d_amg_small_regions_workspace_bytes(*bad) == 0 and load.sam6d_mask_components_workspace_bytes(*bad) == 0


def test_ops_refuse_cpu_tensors():
    from sam6d_hip import amg
    m = torch.zeros((2, 8, 8), dtype=torch.bool)
    with pytest.raises(RuntimeError):
        amg.remove_small_regions(m, 4)
    with pytest.raises(RuntimeError):
        amg.mask_components(m)
    with pytest.raises(RuntimeError):
        amg.postprocess_small_regions({"masks": m, "boxes": torch.zeros((2, 4), dtype=torch.int64)}, 4, 0.7)
    assert amg.region_threshold(19.5) == 20 and amg.region_threshold(20) == 20 and amg.region_threshold(0) == 1 and R.threshold(19.5) == 20


def test_region_kernels_resources():
    """no kernel of csrc/regions.hip uses scratch; the tile labeller keeps within 64 VGPRs (eight waves per
    SIMD; the build reports 62), the others within 32 (they report 10 to 18)."""
    from tests._util import kernel_resources
    found = kernel_resources(b"rg_init_kernel", r"(rg_[a-z_]+_kernel)")
    print("\n[sam_small_regions] VGPRs, scratch bytes, spills: %s" % found)
    want = {"rg_init_kernel", "rg_merge_kernel", "rg_flatten_kernel", "rg_emit_kernel", "rg_state_init_kernel", "rg_roots_kernel",
            "rg_fill_kernel", "rg_keep_kernel", "rg_finish_kernel"}
    assert set(found) == want, set(found) ^ want
    for name, (vgprs, scratch, spills) in found.items():
        assert scratch == 0 and spills == 0 and vgprs <= (64 if name == "rg_init_kernel" else 32), (name, vgprs, scratch, spills)


def test_dropin_signature_is_unchanged():
    mod = importlib.import_module("model.sam")
    cls = mod.CustomSamAutomaticMaskGenerator
    assert isinstance(inspect.getattr_static(cls, "postprocess_small_regions"), staticmethod)
    assert list(inspect.signature(cls.postprocess_small_regions).parameters) == ["mask_data", "min_area", "nms_thresh"]
    empty = {"masks": torch.zeros((0, 4, 4), dtype=torch.bool), "boxes": torch.zeros((0, 4), dtype=torch.int64)}
    assert cls.postprocess_small_regions(empty, 10, 0.7) is empty
