"""The integer / byte kernels at the ISM -> PEM seam off their golden scenes (csrc/detections.hip, csrc/testdata.hip,
sam6d_depth_to_cloud, sam6d_select_smallest), bit for bit against tests/seam_edges_ref.py: image sizes that are no multiple of the
wave, crops that cut valid pixels off or are empty, counts on the 1024-thread chunk edges, an explicit cap, areas and IoUs exactly
at their thresholds, and NaN scores / distances under the total orders the two ranking kernels define.  No tolerances.

Why the NaN cases notice a revert of either key order (argued from the rank table, tests/test_seam_edges_host.py): under the old
float rule a NaN gets the rank of the best number of its group, scores [0.5, nan, 0.9, nan, 0.5] -> ranks [1, 0, 0, 0, 2], so one
slot holds whichever of three writes lands last and two slots keep what the buffer held; keep_idx / sel then cannot equal the
restatement, which places every NaN (first for NMS, last for the selection) in index order."""
import functools

import numpy as np
import pytest
import torch

from tests._util import PKG  # noqa: F401  (sys.path)
from tests import seam_edges_ref as R

pytestmark = pytest.mark.gpu

RADIUS = 0.2


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(H, W):
    """The depth map, the family masks and the reference geometry of one image size (computed once, never modified)."""
    depth = R.depth_map(H, W)
    fam = R.mask_families(H, W, depth)
    masks = np.stack([m for _, m in fam])
    xyz = R.xyz_maps(len(fam), H, W)
    ref_all = [R.proposal_geometry(m, depth, R.K_EDGE, 10.0) for m in masks]
    ref = [R.proposal_geometry(m, depth, R.K_EDGE, RADIUS) for m in masks]
    tem = [R.template_geometry(m, xyz[i]) for i, m in enumerate(masks)]
    return depth, [n for n, _ in fam], masks, xyz, ref_all, ref, tem


def _check_choose(dev, geom, n, chooses, clouds, bboxes, names, img_sizes=(224, 100, 7)):
    """sam6d_choose_points with a sel that covers every kept index of each item, against get_resize_rgb_choose."""
    from sam6d_hip import inputs
    ns = max(1, max(n))
    sel = np.stack([np.arange(ns, dtype=np.int32) % max(1, k) for k in n])
    for S in img_sizes:
        pts, rc = inputs.proposal_choose(geom, torch.from_numpy(sel).to(dev), S)
        pts, rc = _np(pts), _np(rc)
        assert rc.dtype == np.int64
        for i, k in enumerate(n):
            if k == 0:
                continue  # an empty crop has no ratio; the caller skips it
            assert np.array_equal(pts[i], clouds[i][sel[i]]), (names[i], S)
            assert np.array_equal(rc[i], R.rgb_choose(chooses[i][sel[i]], bboxes[i], S)), (names[i], S)


@pytest.mark.parametrize("H,W", R.SIZES)
def test_proposal_geometry_families(dev, H, W):
    from sam6d_hip import inputs
    depth, names, masks, _, ref_all, ref, _ = _scene(H, W)
    m_d, d_d = torch.from_numpy(masks).to(dev), torch.from_numpy(depth).to(dev)
    # a radius that keeps everything shows the raster-order choose and cloud of the crop as the crop kernel wrote them
    g = inputs.proposal_geometry(m_d, d_d, R.K_EDGE, 10.0)
    bbox, count, n_valid, n_keep = _np(g["bbox"]), _np(g["count"]), _np(g["n_valid"]), _np(g["n_keep"])
    for i, o in enumerate(ref_all):
        assert bbox[i].tolist() == o["bbox"] and count[i] == o["count"] and n_valid[i] == o["n_valid"] == n_keep[i], names[i]
        k = o["n_valid"]
        assert np.array_equal(_np(g["choose"][i, :k]), o["choose"]) and np.array_equal(_np(g["cloud"][i, :k]), o["cloud"]), names[i]
        assert np.array_equal(_np(g["center"][i]), o["center"]), names[i]
    g = inputs.proposal_geometry(m_d, d_d, R.K_EDGE, RADIUS)
    n_keep = _np(g["n_keep"])
    for i, o in enumerate(ref):
        k = len(o["keep_choose"])
        assert n_keep[i] == k and np.array_equal(_np(g["center"][i]), o["center"]), names[i]
        assert np.array_equal(_np(g["choose"][i, :k]), o["keep_choose"]) and np.array_equal(_np(g["cloud"][i, :k]), o["keep_cloud"]), names[i]
    _check_choose(dev, g, [len(o["keep_choose"]) for o in ref], [o["keep_choose"] for o in ref], [o["keep_cloud"] for o in ref],
                  [o["bbox"] for o in ref], names, img_sizes=(224, 7))


@pytest.mark.parametrize("H,W", R.SIZES)
def test_template_geometry_families(dev, H, W):
    from sam6d_hip import inputs
    _, names, masks, xyz, _, _, tem = _scene(H, W)
    g = inputs.template_geometry(torch.from_numpy(masks).to(dev), torch.from_numpy(xyz).to(dev))
    bbox, count, n_valid = _np(g["bbox"]), _np(g["count"]), _np(g["n_valid"])
    for i, o in enumerate(tem):
        assert bbox[i].tolist() == o["bbox"] and count[i] == o["count"] and n_valid[i] == o["n_valid"], names[i]
        k = o["n_valid"]
        assert np.array_equal(_np(g["choose"][i, :k]), o["choose"]), names[i]
        assert np.array_equal(_np(g["cloud"][i, :k]), o["cloud"]), names[i]  # xyz / 1000 in fp32, not xyz * 0.001
    _check_choose(dev, g, [o["n_valid"] for o in tem], [o["choose"] for o in tem], [o["cloud"] for o in tem], [o["bbox"] for o in tem],
                  names, img_sizes=(100,))


@pytest.mark.parametrize("radius", R.CHUNK_RADII)
def test_chunk_edges(dev, radius):
    """Crops of 32x32 and 34x34 pixels and exactly 1024 / 1025 valid pixels: the last chunk of the crop and radius-filter loops is
    full, one element long, or absent; the in-place compaction crosses a chunk.  Then the choice on crop sides 2, 34, 36 and 64."""
    from sam6d_hip import inputs
    depth, masks = R.chunk_edge_scene()
    g = inputs.proposal_geometry(torch.from_numpy(masks).to(dev), torch.from_numpy(depth).to(dev), R.K_EDGE, radius)
    ref = [R.proposal_geometry(m, depth, R.K_EDGE, radius) for m in masks]
    for i, o in enumerate(ref):
        name = R.CHUNK_NAMES[i]
        k = len(o["keep_choose"])
        assert _np(g["bbox"][i]).tolist() == o["bbox"] and int(g["count"][i]) == o["count"] and int(g["n_valid"][i]) == o["n_valid"], name
        assert int(g["n_keep"][i]) == k and np.array_equal(_np(g["center"][i]), o["center"]), name
        assert np.array_equal(_np(g["choose"][i, :k]), o["keep_choose"]) and np.array_equal(_np(g["cloud"][i, :k]), o["keep_cloud"]), name
    _check_choose(dev, g, [len(o["keep_choose"]) for o in ref], [o["keep_choose"] for o in ref], [o["keep_cloud"] for o in ref],
                  [o["bbox"] for o in ref], R.CHUNK_NAMES)


@pytest.mark.parametrize("template", [False, True])
def test_explicit_cap_through_the_c_entry(dev, template):
    """cap below the valid count: n_valid == cap, the first cap pixels in raster order, and nothing beyond the item's cap rows --
    the next item's rows and the guard behind the buffers keep their sentinel, through the crop and through the radius filter."""
    from sam6d_hip import _lib
    from sam6d_hip.runtime import _s
    depth, masks = R.chunk_edge_scene()
    masks = masks[[1, 2]].copy()  # 1156 and 1025 valid pixels in a 34x34 crop
    if template:
        masks[masks != 0] = 255
    xyz = R.xyz_maps(2, 64, 64)
    cap, SENT = 1000, -7
    m_d = torch.from_numpy(masks).to(dev)
    src = torch.from_numpy(xyz if template else depth).to(dev)
    bbox = torch.empty(2, 4, dtype=torch.int32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    if template:
        _lib.call("sam6d_template_bbox", m_d.data_ptr(), 2, 64, 64, bbox.data_ptr(), count.data_ptr(), _s())
    else:
        _lib.call("sam6d_mask_bbox", m_d.data_ptr(), src.data_ptr(), 2, 64, 64, bbox.data_ptr(), count.data_ptr(), _s())
    # room for three items; item 0 alone is processed first, then both
    choose = torch.full((3, cap), SENT, dtype=torch.int32, device=dev)
    cloud = torch.full((3, cap, 3), float(SENT), dtype=torch.float32, device=dev)
    n_valid = torch.full((3,), SENT, dtype=torch.int32, device=dev)
    K = R.K_EDGE

    def crop(n):
        if template:
            _lib.call("sam6d_template_crop_points", m_d.data_ptr(), src.data_ptr(), n, 64, 64, bbox.data_ptr(), cap, choose.data_ptr(),
                      cloud.data_ptr(), n_valid.data_ptr(), _s())
        else:
            _lib.call("sam6d_crop_masked_points", m_d.data_ptr(), src.data_ptr(), n, 64, 64, bbox.data_ptr(), float(K[0][0]), float(K[1][1]),
                      float(K[0][2]), float(K[1][2]), cap, choose.data_ptr(), cloud.data_ptr(), n_valid.data_ptr(), _s())
        torch.cuda.synchronize()

    ref = [R.template_geometry(masks[i], xyz[i], cap=cap) if template else R.proposal_geometry(masks[i], depth, K, 0.05, cap=cap) for i in range(2)]
    assert [int(c) for c in count] == [1156, 1025] and all(o["n_valid"] == cap for o in ref)
    for n in (1, 2):
        crop(n)
        for i in range(n):
            assert int(n_valid[i]) == cap
            assert np.array_equal(_np(choose[i]), ref[i]["choose"]) and np.array_equal(_np(cloud[i]), ref[i]["cloud"])
        assert bool((choose[n:] == SENT).all()) and bool((cloud[n:] == SENT).all()) and bool((n_valid[n:] == SENT).all())
    if template:
        return
    n_keep = torch.full((3,), SENT, dtype=torch.int32, device=dev)
    center = torch.full((3, 3), float(SENT), dtype=torch.float32, device=dev)
    _lib.call("sam6d_radius_filter", 2, cap, n_valid.data_ptr(), 0.05, choose.data_ptr(), cloud.data_ptr(), n_keep.data_ptr(),
              center.data_ptr(), _s())
    torch.cuda.synchronize()
    for i in range(2):
        k = len(ref[i]["keep_choose"])
        assert 4 <= k < cap and int(n_keep[i]) == k and np.array_equal(_np(center[i]), ref[i]["center"])
        assert np.array_equal(_np(choose[i, :k]), ref[i]["keep_choose"]) and np.array_equal(_np(cloud[i, :k]), ref[i]["keep_cloud"])
    assert bool((choose[2] == SENT).all()) and bool((cloud[2] == SENT).all()) and int(n_keep[2]) == SENT and bool((center[2] == SENT).all())


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (37, 53)])
def test_depth_to_cloud_windows(dev, H, W):
    from oracle import pem_oracle as O
    from sam6d_hip import inputs
    depth = R.depth_map(H, W, seed=3)
    if H * W > 1:
        assert (depth == 0).any()
    d_d = torch.from_numpy(depth).to(dev)
    wins = [None, [0, H, 0, W], [0, 1, 0, W], [H - 1, H, 0, W], [0, H, 0, 1], [0, H, W - 1, W], [H // 2, H, W // 3, W],
            [H // 2, H // 2, 0, W], [0, H, W, W], [0, 0, 0, 0]]  # whole map, single rows and columns, a sub-window, empty windows
    for bb in wins:
        want = O.depth_to_cloud(depth, R.K_EDGE, bb)
        got = _np(inputs.depth_to_cloud(d_d, R.K_EDGE, bb))
        assert got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got, want), (H, W, bb)


def test_small_keep_edges(dev):
    from oracle import ism_oracle as IO
    from sam6d_hip import ism
    for name, boxes, masks, mb, mm in R.small_keep_cases():
        want = IO.small_detection_keep(boxes, masks, mb, mm)
        got = ism.small_detection_keep(boxes.to(dev), masks.to(dev), mb, mm).cpu()
        assert got.dtype == torch.bool and torch.equal(got, want), (name, got.tolist(), want.tolist())
        assert torch.equal(got, R.small_keep_ref(boxes, masks, mb ** 2, mm)), name


@pytest.mark.parametrize("N", R.INDEX_SIZES)
def test_mask_to_indices_sizes(dev, N):
    from sam6d_hip import _lib, ism
    from sam6d_hip.runtime import _s
    SENT = -9
    for name, keep in R.keep_patterns(N).items():
        want = np.flatnonzero(keep)
        k_d = torch.from_numpy(keep).to(dev)
        got = ism.mask_to_indices(k_d)
        assert got.dtype == torch.int64 and np.array_equal(_np(got), want), (N, name)
        # through the C entry: nothing is written beyond count
        buf = torch.zeros(max(N, 1), dtype=torch.uint8, device=dev)
        buf[:N] = k_d
        idx = torch.full((N + 8,), SENT, dtype=torch.int64, device=dev)
        cnt = torch.full((2,), SENT, dtype=torch.int32, device=dev)
        _lib.call("sam6d_mask_to_indices", buf.data_ptr(), N, idx.data_ptr(), cnt.data_ptr(), _s())
        torch.cuda.synchronize()
        assert _np(cnt).tolist() == [len(want), SENT], (N, name)
        assert np.array_equal(_np(idx[: len(want)]), want) and bool((idx[len(want):] == SENT).all()), (N, name)


@pytest.mark.parametrize("row_bytes", [1, 3, 4, 12, 16, 20, 48])
def test_take_rows_widths_and_alignment(dev, row_bytes):
    """All three width paths (16-byte, 4-byte and single-byte moves): the path follows row_bytes and the alignment of the source, so
    each row size is read from views that start 0, 4 and 1 bytes into an allocation.  Negative indices count from the end, an index
    outside [-n, n) gives a zero row, M = 0 gives an empty result."""
    from sam6d_hip import ism
    n_src = 37
    g = np.random.default_rng(row_bytes)
    base = g.integers(1, 256, size=n_src * row_bytes + 32, dtype=np.uint8)  # no zero byte: a zero row is unmistakable
    base_d = torch.from_numpy(base).to(dev)
    assert base_d.data_ptr() % 16 == 0
    idx = np.array([0, n_src - 1, -1, -n_src, 5, 5, n_src, -n_src - 1, 10 ** 12, -(10 ** 12), 17, -3], np.int64)
    for off in (0, 4, 1):
        src_np = base[off: off + n_src * row_bytes].reshape(n_src, row_bytes)
        src = base_d[off: off + n_src * row_bytes].view(n_src, row_bytes)
        assert src.is_contiguous() and src.data_ptr() % 16 == off
        want = np.zeros((len(idx), row_bytes), np.uint8)
        ok = (idx >= -n_src) & (idx < n_src)
        want[ok] = src_np[idx[ok]]
        got = ism.take_rows(src, torch.from_numpy(idx).to(dev))
        assert got.dtype == torch.uint8 and np.array_equal(_np(got), want), (row_bytes, off)
        empty = ism.take_rows(src, torch.zeros(0, dtype=torch.int64, device=dev))
        assert tuple(empty.shape) == (0, row_bytes)
    if row_bytes % 4 == 0:  # the same bytes as a wider dtype
        src = base_d[: n_src * row_bytes].view(torch.float32).view(n_src, row_bytes // 4)
        sel = torch.tensor([3, -1, 0], device=dev)
        assert torch.equal(ism.take_rows(src, sel).view(torch.uint8), base_d[: n_src * row_bytes].view(n_src, row_bytes)[sel])


_NMS_CASES = R.nms_cases()


@pytest.mark.parametrize("case", range(len(_NMS_CASES)), ids=[c[0] for c in _NMS_CASES])
def test_nms_edges(dev, case):
    from sam6d_hip import ism
    name, boxes, scores, group, thr = _NMS_CASES[case]
    N = len(boxes)
    want = R.nms_ref(boxes, scores, group, thr)
    got = ism.nms(boxes.to(dev), scores.to(dev), thr, object_ids=None if group is None else group.to(dev)).cpu()
    assert got.dtype == torch.int64
    vals = got.tolist()
    assert len(set(vals)) == len(vals) and all(0 <= v < N for v in vals), "keep_idx[:count] must hold distinct indices in [0, N)"
    assert torch.equal(got, want), (name, vals[:16], want.tolist()[:16])


def test_nms_iou_equal_to_the_threshold_is_kept(dev):
    from sam6d_hip import ism
    b = torch.from_numpy(R.IOU_PAIR).to(dev)
    s = torch.tensor([0.9, 0.8], device=dev)
    assert ism.nms(b, s, 0.5).tolist() == [0, 1]
    assert ism.nms(b, s, 0.4999999).tolist() == [0]
    assert ism.nms(b, s, 0.0).tolist() == [0] and ism.nms(b, s, 1.0).tolist() == [0, 1]


def _select(dev, rows, k):
    from sam6d_hip import _lib
    from sam6d_hip.runtime import _s
    d = torch.from_numpy(np.stack(rows)).to(dev)
    B, n = d.shape
    sel = torch.full((B + 1, k), -1, dtype=torch.int32, device=dev)
    _lib.call("sam6d_select_smallest", d.data_ptr(), B, n, k, sel.data_ptr(), _s())
    torch.cuda.synchronize()
    assert bool((sel[B] == -1).all())
    return _np(sel[:B])


@pytest.mark.parametrize("n,k,numbers", [(37, 37, None), (6000, 300, None), (14319, 1, None), (14400, 300, None), (6000, 300, 250),
                                         (14400, 300, 250)])
def test_select_smallest_nan_order(dev, n, k, numbers):
    """Rows with NaN of both signs, +-inf, +-0 and ties, on the radix route (37, 6000) and on the all-pairs route (14319, 14400), and
    one row on each with so few numbers that k reaches into the NaNs: sel is the first k of the order (isnan, value, index)."""
    assert R.select_route(n, k) == ("radix" if n <= 6000 else "allpairs")
    rows = [R.select_row(n, seed=s, numbers=numbers) for s in range(2)]
    got = _select(dev, rows, k)
    for b, row in enumerate(rows):
        want = R.select_smallest_ref(row, k)
        assert sorted(set(got[b].tolist())) == sorted(got[b].tolist()) and got[b].min() >= 0 and got[b].max() < n
        assert np.array_equal(got[b], want), (n, k, b, got[b][:12], want[:12])


@pytest.mark.parametrize("numbers", [None, 100])
def test_select_smallest_routes_agree(dev, numbers):
    """The same rows through both kernels: n = 14000 takes the radix route at k = 150 and the all-pairs route at k = 300, and the
    first 150 of the longer answer are the shorter one."""
    n = 14000
    assert R.select_route(n, 150) == "radix" and R.select_route(n, 300) == "allpairs"
    rows = [R.select_row(n, seed=5 + s, numbers=numbers) for s in range(2)]
    radix, allpairs = _select(dev, rows, 150), _select(dev, rows, 300)
    assert np.array_equal(allpairs[:, :150], radix)
    for b, row in enumerate(rows):
        assert np.array_equal(allpairs[b], R.select_smallest_ref(row, 300))
