"""SAM's min_mask_region_area clean-up on the library (csrc/regions.hip, sam6d_hip.amg.mask_components / remove_small_regions /
postprocess_small_regions, the drop-in's postprocess_small_regions) against the numpy restatement tests/small_regions_ref.py: every
comparison is exact (components of a binary image are unique).  The shapes straddle the kernels' 64-pixel chunks and 4-row workgroups:
one pixel, one row, one column, odd sizes with more than one workgroup in both directions, and the shipped 480 x 640 once."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import small_regions_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 257), (257, 1), (33, 65), (70, 130), (129, 191)]
GROUPS = [(0, 1), (1, 4), (4, 11)]  # the eleven patterns of a shape go through the entries as K = 1, 3 and 7
GUARD = 64
FILL = 0xA5


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _patterns(shape):
    p = R.patterns(shape[0], shape[1], seed=shape[0] + shape[1])
    names = tuple(p)
    masks = np.stack([p[n] for n in names])
    masks.setflags(write=False)
    return names, masks


@functools.lru_cache(maxsize=None)
def _ref_components(shape, invert):
    labels, areas = R.components_batch(_patterns(shape)[1], invert)
    labels.setflags(write=False), areas.setflags(write=False)
    return labels, areas


@functools.lru_cache(maxsize=None)
def _ref_clean(shape, min_area):
    out = R.clean_batch(_patterns(shape)[1], min_area)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _big():
    masks = np.stack([R.blobs(480, 640, 11), R.coin(480, 640, 12)])
    masks.setflags(write=False)
    return masks


def _t(a):
    """A torch tensor with a copy of a (shared, read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def _guarded(nbytes, dtype=torch.uint8):
    """A buffer of nbytes between two guards, all FILL: (whole uint8 tensor, pointer to the payload)."""
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=_dev())
    return buf, buf.data_ptr() + GUARD


def _guards_intact(buf, nbytes):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == FILL).all() and (b[GUARD + nbytes:] == FILL).all())


def _small_regions_c(masks, min_area):
    """sam6d_amg_small_regions through the C ABI with guard bytes around masks, changed and box -> cleaned, changed, boxes (numpy)."""
    from sam6d_hip import _lib
    masks = np.ascontiguousarray(masks)
    K, H, W = masks.shape
    mb, mp = _guarded(K * H * W)
    cb, cp = _guarded(K)
    bb, bp = _guarded(16 * K)
    mb[GUARD:GUARD + K * H * W] = _t(masks.astype(np.uint8).reshape(-1)).to(_dev())
    nbytes = int(_lib.load().sam6d_amg_small_regions_workspace_bytes(K, H, W))
    assert nbytes >= 8 * K * H * W
    ws = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
    _lib.call("sam6d_amg_small_regions", mp, K, H, W, int(min_area), cp, bp, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _guards_intact(mb, K * H * W) and _guards_intact(cb, K) and _guards_intact(bb, 16 * K), "a guard byte was written"
    cleaned = mb[GUARD:GUARD + K * H * W].cpu().numpy().reshape(K, H, W)
    changed = cb[GUARD:GUARD + K].cpu().numpy()
    box = bb[GUARD:GUARD + 16 * K].cpu().numpy().view(np.int32).reshape(K, 4)
    assert set(np.unique(cleaned)) <= {0, 1} and set(np.unique(changed)) <= {0, 1}
    return cleaned.astype(bool), changed.astype(bool), box.astype(np.int64)


def _check_clean(masks, min_area, want=None):
    want = R.clean_batch(masks, min_area) if want is None else want
    got = _small_regions_c(masks, min_area)
    for name, g, w in zip(("masks", "changed", "boxes"), got, want):
        assert np.array_equal(g, w), "%s differ at min_area %d" % (name, min_area)
    return got


# ------------------------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_components_patterns(shape, invert):
    from sam6d_hip import amg
    names, masks = _patterns(shape)
    want_l, want_a = _ref_components(shape, invert)
    for a, b in GROUPS:
        labels, areas = amg.mask_components(_t(masks[a:b]).to(_dev()), invert=invert)
        assert labels.dtype == torch.int32 and areas.dtype == torch.int32 and tuple(labels.shape) == (b - a,) + shape
        for k in range(a, b):
            assert torch.equal(labels[k - a].cpu(), _t(want_l[k])), (names[k], "labels")
            assert torch.equal(areas[k - a].cpu(), _t(want_a[k])), (names[k], "areas")
    if min(shape) >= 2 and "checkerboard" in names:  # one component each way under 8-connectivity (4-connectivity gives H W / 2)
        k = names.index("checkerboard")
        assert len(np.unique(want_l[k])) == 2


def test_mask_components_480x640():
    from sam6d_hip import amg
    masks = _big()
    for invert in (False, True):
        want_l, want_a = R.components_batch(masks, invert)
        labels, areas = amg.mask_components(_t(masks).to(_dev()), invert=invert)
        assert torch.equal(labels.cpu(), _t(want_l)) and torch.equal(areas.cpu(), _t(want_a))


def test_mask_components_dtypes_and_slices(monkeypatch):
    """bool, uint8 and float32 masks give the same labels, and so does a workspace budget that forces one mask per slice."""
    from sam6d_hip import amg
    _, masks = _patterns((33, 65))
    m = _t(masks).to(_dev())
    ref = amg.mask_components(m)
    for other in (m.to(torch.uint8) * 255, m.float()):
        got = amg.mask_components(other)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    monkeypatch.setattr(amg, "REGIONS_WS_BYTES", 1)
    got = amg.mask_components(m)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    cleaned = amg.remove_small_regions(m, 20)
    monkeypatch.undo()
    whole = amg.remove_small_regions(m, 20)
    assert all(torch.equal(a, b) for a, b in zip(cleaned, whole))


# ------------------------------------------------------------------------------------------------- the clean-up
@pytest.mark.parametrize("min_area", [1, 2, 20, 100, "HW+1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_remove_small_regions_patterns(shape, min_area):
    t = shape[0] * shape[1] + 1 if min_area == "HW+1" else min_area
    _, masks = _patterns(shape)
    want = _ref_clean(shape, t)
    for a, b in GROUPS:
        _check_clean(masks[a:b], t, tuple(w[a:b] for w in want))


def test_remove_small_regions_480x640():
    masks = _big()
    _, changed, _ = _check_clean(masks, 100)
    assert changed.all()


def test_many_masks_share_workgroups():
    """With K in the hundreds the kernels that end in per-mask atomics give a workgroup several tiles of a mask to walk (300 masks at
    33 x 65: 14 workgroups for 18 tiles), and the package's slicing is left to one slice."""
    masks = np.stack([(R.blobs if i % 2 else R.coin)(33, 65, 1000 + i) for i in range(300)])
    _, changed, _ = _check_clean(masks, 5)
    assert changed.any()


def _canvas(H=70, W=130):
    return np.zeros((H, W), dtype=bool)


def test_rectangles_around_the_threshold():
    """Islands and holes of min_area - 1, min_area and min_area + 1 pixels: only the ones below the threshold go; a hole that touches the
    image border is filled like any other (the reference has no border rule)."""
    t = 12
    m = _canvas()
    m[2:3, 2:13] = True       # island of 11
    m[6:9, 2:6] = True        # island of 12
    m[12:13, 2:15] = True     # island of 13
    m[20:60, 0:100] = True    # a body for the holes, reaching the left border
    m[25:26, 10:21] = False   # hole of 11
    m[30:33, 10:14] = False   # hole of 12
    m[36:37, 10:23] = False   # hole of 13
    m[45:46, 0:11] = False    # hole of 11 on the border
    cleaned, changed, box = _check_clean(m[None], t)
    c = cleaned[0]
    assert changed[0] and not c[2, 2:13].any() and c[6:9, 2:6].all() and c[12, 2:15].all()
    assert c[25, 10:21].all() and not c[30:33, 10:14].any() and not c[36, 10:23].any() and c[45, 0:11].all()
    assert box[0].tolist() == [0, 6, 99, 59]


def test_ring_is_filled_before_islands_are_judged():
    """An 8-pixel ring around a one-pixel hole, min_area 9: the holes pass makes it a 9-pixel island, which stays.  Islands first would
    delete the ring (8 < 9) and leave nothing."""
    m = _canvas(33, 65)
    m[10:13, 20:23] = True
    m[11, 21] = False
    m[20:30, 40:60] = True  # an island that is not small, so that "keep the largest" does not come into play
    cleaned, changed, box = _check_clean(m[None], 9)
    want = m.copy()
    want[11, 21] = True
    assert changed[0] and np.array_equal(cleaned[0], want) and cleaned[0][10:13, 20:23].sum() == 9


def test_all_islands_small_keeps_the_unique_largest():
    m = _canvas()
    m[5, 5:8] = True          # 3
    m[40, 100:105] = True     # 5, the largest, neither first nor last in row-major order
    m[60:62, 20:22] = True    # 4
    cleaned, changed, box = _check_clean(m[None], 10)
    want = _canvas()
    want[40, 100:105] = True
    assert changed[0] and np.array_equal(cleaned[0], want) and box[0].tolist() == [100, 40, 104, 40]


def test_package_rule_equal_largest_islands_first_in_row_major_order_stays():
    """The package's own rule (the reference leaves it to cv2's label numbering): of two largest islands of
    equal area the one whose first pixel comes first in row-major order stays."""
    m = _canvas()
    m[30:35, 100] = True      # 5, first pixel (30, 100)
    m[30, 10:13] = True       # 3, first pixel (30, 10): earlier, but smaller
    m[31, 20:25] = True       # 5, first pixel (31, 20): later in row-major order although further left
    cleaned, changed, box = _check_clean(m[None], 10)
    want = _canvas()
    want[30:35, 100] = True
    assert changed[0] and np.array_equal(cleaned[0], want)


def test_untouched_masks_come_back_byte_for_byte():
    m = np.stack([_canvas(), _canvas(), _canvas()])
    m[0, 10:40, 10:60] = True
    m[0, 20:25, 20:25] = False       # a hole of 25 >= 20
    m[1, 0:5, 0:4] = True            # exactly min_area
    m[2, :, :] = True                # nothing to label in ~m
    cleaned, changed, box = _check_clean(m, 20)
    assert not changed.any() and np.array_equal(cleaned, m)
    assert box.tolist() == [[10, 10, 59, 39], [0, 0, 3, 4], [0, 0, 129, 69]]


def test_refused_calls_write_nothing():
    from sam6d_hip import _lib
    K, H, W = 2, 33, 65
    lib = _lib.load()
    nbytes = int(lib.sam6d_amg_small_regions_workspace_bytes(K, H, W))
    assert nbytes > 0 and lib.sam6d_amg_small_regions_workspace_bytes(0, H, W) == 0
    assert lib.sam6d_amg_small_regions_workspace_bytes(1, 65536, 32768) == 0 and lib.sam6d_mask_components_workspace_bytes(65536, H, W) == 0
    bufs = [torch.full((n,), FILL, dtype=torch.uint8, device=_dev()) for n in (K * H * W, K, 16 * K, 4 * K * H * W, 4 * K * H * W, nbytes)]
    masks, changed, box, labels, areas, ws = (b.data_ptr() for b in bufs)
    s = torch.cuda.current_stream().cuda_stream
    for args, word in (((masks, 0, H, W, 5, changed, box, ws, nbytes, s), "K"), ((masks, 65536, H, W, 5, changed, box, ws, nbytes, s), "K"),
                       ((masks, K, 65536, 32768, 5, changed, box, ws, nbytes, s), "H \\* W"), ((masks, K, H, W, 0, changed, box, ws, nbytes, s), "min_area"),
                       ((masks, K, H, W, 5, changed, box, ws, nbytes - 1, s), "workspace")):
        with pytest.raises(RuntimeError, match=word):
            _lib.call("sam6d_amg_small_regions", *args)
    for args, word in (((masks, 0, H, W, 0, labels, areas, ws, nbytes, s), "K"), ((masks, K, 65536, 32768, 0, labels, areas, ws, nbytes, s), "H \\* W"),
                       ((masks, K, H, W, 0, labels, areas, ws, 8 * K * H * W - 1, s), "workspace")):
        with pytest.raises(RuntimeError, match=word):
            _lib.call("sam6d_mask_components", *args)
    torch.cuda.synchronize()
    assert all(bool((b == FILL).all()) for b in bufs)


def test_remove_small_regions_dtypes_agree():
    from sam6d_hip import amg
    _, masks = _patterns((70, 130))
    want = _ref_clean((70, 130), 20)
    m = _t(masks).to(_dev())
    for inp in (m, m.to(torch.uint8), m.float()):
        before = inp.clone()
        cleaned, changed, boxes = amg.remove_small_regions(inp, 20)
        assert cleaned.dtype == inp.dtype and changed.dtype == torch.bool and boxes.dtype == torch.int64 and torch.equal(inp, before)
        assert torch.equal(cleaned.cpu(), _t(want[0]).to(inp.dtype))
        assert torch.equal(changed.cpu(), _t(want[1])) and torch.equal(boxes.cpu(), _t(want[2]))
    # a float threshold: sizes are integers, so 19.5 is 20, and anything <= 1 changes nothing
    got = amg.remove_small_regions(m, 19.5)
    assert torch.equal(got[0].cpu(), _t(want[0])) and torch.equal(got[1].cpu(), _t(want[1]))
    got = amg.remove_small_regions(m, 0.5)
    assert torch.equal(got[0], m) and not got[1].any()


def test_coin_flip_five_runs_are_bitwise_equal():
    from sam6d_hip import amg
    m = torch.from_numpy(R.coin(129, 191, 5)[None]).to(_dev())
    first = None
    for _ in range(5):
        res = amg.mask_components(m) + amg.mask_components(m, invert=True) + amg.remove_small_regions(m, 20)
        if first is None:
            first = res
        assert all(torch.equal(a, b) for a, b in zip(res, first))


# ------------------------------------------------------------------------------------------------- with the NMS, and the drop-in
def _twelve():
    """12 masks at 70 x 130: rectangles in the cells of a 2 x 5 grid.  Masks 0 and 1 become duplicates of the unchanged masks 5 and 8
    (a speck to drop, a hole to fill), mask 2 changes and has no duplicate, the other nine are left alone."""
    def rect(i):
        m = _canvas()
        r, c = divmod(i, 5)
        m[5 + 35 * r:25 + 35 * r + i, 4 + 26 * c:20 + 26 * c] = True
        return m
    masks = [rect(2), rect(5), rect(9)] + [rect(i) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8)]
    masks[0][68, 120:123] = True                 # a speck of 3, far from rect(2)
    masks[1][50:52, 8:10] = False                # a hole of 4 in rect(5)
    masks[2][0, 0:2] = True                      # a speck of 2; rect(9) has no unchanged twin
    return np.stack(masks)


def test_postprocess_small_regions_prefers_unchanged_masks():
    from sam6d_hip import amg
    masks = _twelve()
    boxes_in = np.array([R.mask_box(m) for m in masks], dtype=np.int64) + 1000  # deliberately off: unchanged survivors must keep them
    want_m, want_b, keep = R.postprocess(masks, boxes_in, 10, 0.7)
    assert keep.tolist() == [3, 4, 5, 6, 7, 8, 9, 10, 11, 2]  # the nine unchanged in index order, then the changed mask without a twin
    for dtype in (torch.bool, torch.float32):
        data = {"masks": _t(masks).to(_dev()).to(dtype), "boxes": torch.from_numpy(boxes_in).to(_dev())}
        out = amg.postprocess_small_regions(data, 10, 0.7)
        assert set(out) == {"masks", "boxes"} and out["masks"].dtype == dtype and out["boxes"].dtype == torch.int64
        assert torch.equal(out["masks"].cpu(), _t(want_m).to(dtype)) and torch.equal(out["boxes"].cpu(), _t(want_b))
        assert (out["boxes"][:9] >= 1000).all() and out["boxes"][9].tolist() == R.mask_box(want_m[9])
    empty = {"masks": torch.zeros((0, 70, 130), dtype=torch.bool, device=_dev()), "boxes": torch.zeros((0, 4), dtype=torch.int64, device=_dev())}
    assert amg.postprocess_small_regions(empty, 10, 0.7) is empty


def test_dropin_min_mask_region_area_on_the_device():
    """generate_masks with min_mask_region_area = 50 on the HIP device (no cv2 involved) returns what the restatement makes of the same
    run's masks without the clean-up."""
    mod = importlib.import_module("model.sam")
    from tests.sam_amg_stub import StubSam, encode_image
    image = np.zeros((480, 640, 3), dtype=np.uint8)
    kw = dict(encode_image=encode_image, points_per_batch=256)
    base = mod.CustomSamAutomaticMaskGenerator(StubSam(_dev()), **kw).generate_masks(image)
    g = mod.CustomSamAutomaticMaskGenerator(StubSam(_dev()), min_mask_region_area=50, **kw)
    got = g.generate_masks(image)
    want_m, want_b, _ = R.postprocess(base["masks"].cpu().numpy(), base["boxes"].cpu().numpy(), 50, max(g.box_nms_thresh, g.crop_nms_thresh))
    assert base["masks"].shape[0] >= 5 and got["masks"].is_cuda and got["masks"].dtype == torch.bool and got["boxes"].dtype == torch.int64
    assert torch.equal(got["masks"].cpu(), _t(want_m)) and torch.equal(got["boxes"].cpu(), _t(want_b))
    # the static method itself, as the reference's callers reach it
    again = mod.CustomSamAutomaticMaskGenerator.postprocess_small_regions(base, 50, 0.7)
    assert torch.equal(again["masks"], got["masks"]) and torch.equal(again["boxes"], got["boxes"])
