"""CPU checks of tests/seam_edges_ref.py: every case family of tests/test_seam_edges_gpu.py really contains the edge it is named for,
and the restatement agrees with the torch / numpy calls it restates (no GPU, no library call)."""
import os

import numpy as np
import torch

from tests._util import PKG
from tests import seam_edges_ref as R
from oracle import ism_oracle as IO
from oracle import pem_oracle as O

NAN = float("nan")


def test_get_bbox_stays_inside_small_images_exhaustively():
    """get_bbox over every rectangle of every image up to 8x9: the crop stays inside the image, is at most min(H, W) wide, and both
    the empty crop (a side of 1 halves to 0) and the crop that cuts valid pixels off are common."""
    n = empty = cut = 0
    for H in range(1, 9):
        for W in range(1, 10):
            for r0 in range(H):
                for r1 in range(r0 + 1, H + 1):
                    for c0 in range(W):
                        for c1 in range(c0 + 1, W + 1):
                            m = np.zeros((H, W), bool)
                            m[r0:r1, c0:c1] = True
                            y1, y2, x1, x2 = O.get_bbox(m)
                            assert 0 <= y1 <= y2 <= H and 0 <= x1 <= x2 <= W, (H, W, r0, r1, c0, c1)
                            assert y2 - y1 <= min(H, W) and x2 - x1 <= min(H, W)
                            n += 1
                            empty += (y2 - y1) * (x2 - x1) == 0
                            cut += 0 < m[y1:y2, x1:x2].sum() < m.sum()
    assert n == 19800 and empty > 1000 and cut > 5000, (n, empty, cut)


def test_mask_families_contain_their_edges():
    seen_cut = seen_empty_crop = 0
    for H, W in R.SIZES:
        depth = R.depth_map(H, W)
        assert (depth == 0).any() and 0.02 < (depth == 0).mean() < 0.25 or H * W <= 64
        fam = dict(R.mask_families(H, W, depth))
        geo = {k: R.proposal_geometry(m, depth, R.K_EDGE, 0.2) for k, m in fam.items()}
        tem = {k: R.template_geometry(m, R.xyz_maps(1, H, W)[0]) for k, m in fam.items()}
        assert geo["zero"]["count"] == 0 and geo["zero"]["bbox"] == [0, 0, 0, 0]
        assert fam["depth_zero_only"].any() and geo["depth_zero_only"]["count"] == 0 and geo["depth_zero_only"]["bbox"] == [0, 0, 0, 0]
        for k in ("corner_tl", "corner_tr", "corner_bl", "corner_br"):
            assert geo[k]["count"] == 1  # the corners' depth is positive
        assert geo["full"]["count"] == int((depth > 0).sum()) and fam["full"].all()
        # the mask values: proposals count every non-zero byte, templates only 255
        assert set(np.unique(fam["full"])) == set(R.MASK_VALUES.tolist()) or H * W < 40
        assert tem["full"]["count"] == int((fam["full"] == 255).sum()) < H * W
        if H != W:  # the box of two distant clusters is clamped to min(H, W) and loses one of them
            assert R.cuts_valid_pixels(geo["two_clusters"]) or geo["two_clusters"]["n_valid"] == 0
        # each shift branch of get_bbox is taken: the square around a bar on a border would leave the image on that side, so the crop
        # starts at the border and reaches past the bar's two pixels
        if min(H, W) >= 16:
            for side in ("top", "bottom", "left", "right"):
                for s in (11, 12):
                    y1, y2, x1, x2 = geo["rect%d_%s" % (s, side)]["bbox"]
                    assert {"top": y1 == 0 and y2 > 2, "bottom": y2 == H and y1 < H - 2, "left": x1 == 0 and x2 > 2,
                            "right": x2 == W and x1 < W - 2}[side], (H, W, s, side)
                    assert y2 - y1 == x2 - x1 and (y2 - y1) % 2 == 0  # a square of even side: an odd extent loses a row or column
        seen_cut += sum(R.cuts_valid_pixels(g) and g["n_valid"] > 0 for g in geo.values())
        seen_empty_crop += sum(g["count"] > 0 and g["n_valid"] == 0 for g in geo.values())
    assert seen_cut >= 20 and seen_empty_crop >= 10, (seen_cut, seen_empty_crop)


def test_template_division_is_inexact():
    x = R.xyz_maps(1, 8, 8)[0]
    q = x / np.float32(1000.0)
    assert q.dtype == np.float32 and (q.astype(np.float64) * 1000.0 != x.astype(np.float64)).any()
    assert (q != (x * np.float32(0.001))).any(), "a multiplication by 0.001 must be distinguishable from the division"


def test_chunk_edge_scene_counts():
    depth, masks = R.chunk_edge_scene()
    assert (depth > 0).all()
    want = {"crop32_valid1024": (32, 1024), "crop34_full": (34, 1156), "crop34_valid1025": (34, 1025), "crop34_valid1024": (34, 1024),
            "crop36_full": (36, 1296), "crop64_full": (64, 4096), "crop2": (2, 4)}
    for i, name in enumerate(R.CHUNK_NAMES):
        g_all, g_part, g_few = [R.proposal_geometry(masks[i], depth, R.K_EDGE, r) for r in R.CHUNK_RADII]
        y1, y2, x1, x2 = g_all["bbox"]
        assert (y2 - y1, x2 - x1) == (want[name][0],) * 2 and g_all["n_valid"] == g_all["count"] == want[name][1], name
        assert len(g_all["keep_choose"]) == g_all["n_valid"]           # a radius that keeps everything
        assert len(g_few["keep_choose"]) < 4                             # one that keeps fewer than 4
        if g_all["n_valid"] > 4:
            assert 4 <= len(g_part["keep_choose"]) < g_all["n_valid"]  # and one that compacts in place
    # an explicit cap below the valid count takes the first pixels in raster order
    g = R.proposal_geometry(masks[1], depth, R.K_EDGE, 10.0, cap=1000)
    full = R.proposal_geometry(masks[1], depth, R.K_EDGE, 10.0)
    assert g["n_valid"] == 1000 and np.array_equal(g["choose"], full["choose"][:1000]) and np.all(np.diff(g["choose"]) > 0)


def test_sequential_mean_is_numpys_axis0_mean():
    depth, masks = R.chunk_edge_scene()
    g = R.proposal_geometry(masks[5], depth, R.K_EDGE, 10.0)
    assert np.array_equal(g["center"], np.mean(g["cloud"], axis=0))
    o = O.proposal_geometry(masks[5], depth, R.K_EDGE, np.float32(0.05))
    mine = R.proposal_geometry(masks[5], depth, R.K_EDGE, 0.05)
    assert o["bbox"] == mine["bbox"] and np.array_equal(o["choose"], mine["keep_choose"]) and np.array_equal(o["cloud"], mine["keep_cloud"])
    assert np.array_equal(o["center"], mine["center"])


def test_rgb_choose_ratios_are_not_integers():
    for side in (2, 34, 36, 64):
        ratios = [s / side for s in (224, 100, 7)]
        assert any(r != int(r) for r in ratios)
    ch = np.arange(34 * 34)
    rc = R.rgb_choose(ch, [3, 37, 8, 42], 7)
    assert rc.dtype == np.int64 and rc.min() == 0 and rc.max() == 48


def test_small_keep_cases_sit_on_the_threshold():
    names = [c[0] for c in R.small_keep_cases()]
    assert {"rand_1x1", "rand_3x5", "rand_7x9"} <= set(names)  # H*W not a multiple of 4: the scalar path
    for name, boxes, masks, mb, mm in R.small_keep_cases():
        hw = masks.shape[1] * masks.shape[2]
        want = IO.small_detection_keep(boxes, masks, mb, mm)
        # the kernel receives float(min_box_size ** 2) and float(min_mask_size): same answer as the oracle's float64 thresholds
        assert torch.equal(R.small_keep_ref(boxes, masks, mb ** 2, mm), want), name
        if name.startswith("rand"):
            assert (hw % 4 == 0) == (name in ("rand_2x2", "rand_4x6"))
            ext = torch.stack([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], 1)
            assert (ext == 0).any() and (ext < 0).any() and int(boxes.abs().max()) > (1 << 33)
            assert want.any() and not want.all() or hw == 1
        else:
            # row 0: mask fraction exactly at the threshold -> False; row 1: one pixel more -> True; row 2: box area exactly at it
            frac = masks[0].sum() / hw
            assert float(frac) == float(np.float32(mm)) and not bool(want[0]) and bool(want[1]), name
            area = (boxes[2, 2] - boxes[2, 0]) * (boxes[2, 3] - boxes[2, 1]) / hw
            assert float(area) == float(np.float32(mb ** 2)) and not bool(want[2]) and bool(want[3]), name


def test_iou_pair_is_exactly_at_the_threshold():
    assert R.iou_f32(*R.IOU_PAIR) == np.float32(0.5)
    b = torch.from_numpy(R.IOU_PAIR)
    assert IO.nms(b, torch.tensor([0.9, 0.8]), 0.5).tolist() == [0, 1]          # equal to the threshold: not suppressed
    assert IO.nms(b, torch.tensor([0.9, 0.8]), 0.4999999).tolist() == [0]
    for N in R.NMS_SIZES[1:]:
        assert torch.equal(R.nms_boxes(N)[N - 2:], b)


def test_nms_cases_hold_what_they_name():
    cases = {c[0]: c for c in R.nms_cases()}
    for N in R.NMS_SIZES:
        assert len(cases["ties_N%d" % N][1]) == N
        s = cases["nan_N%d" % N][2]
        if N >= 63:
            bits = s.numpy().view(np.uint32)
            assert (np.isnan(s.numpy()) & (bits >> 31 == 1)).any() and (np.isnan(s.numpy()) & (bits >> 31 == 0)).any()
            assert len(np.unique(s.numpy()[~np.isnan(s.numpy())])) < N // 2  # ties among the numbers
            b = cases["ties_N%d" % N][1]
            wh = b[:, 2:] - b[:, :2]
            assert (wh == 0).all(1).any() and (wh < 0).any() and (b != b.round()).any()
            assert any(torch.equal(b[i], b[j]) for i in range(8) for j in range(N // 2, N // 2 + 3) if i != j)  # exact duplicates
            g = cases["wide_groups_N%d" % N][3]
            assert int(g.max()) > (1 << 32) and int(g.min()) < -(1 << 32) and len(torch.unique(g)) == 4
    for N in (65, 129):
        _, b, s, g, thr = cases["all_nan_group_N%d" % N]
        assert torch.isnan(s[g == 5]).all() and (g == 5).sum() > 3 and not torch.isnan(s[g != 5]).all()
        assert len(torch.unique(cases["each_group_N%d" % N][3])) == N and len(torch.unique(cases["one_group_N%d" % N][3])) == 1
        z = cases["zeros_N%d" % N][2].numpy()
        assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
        # thresholds 0 and 1 do different things to the same boxes
        k0, k1 = R.nms_ref(*cases["thr0_N%d" % N][1:]), R.nms_ref(*cases["thr1_N%d" % N][1:])
        assert len(k0) < len(k1) <= N
    for name, b, s, g, thr in cases.values():
        keep = R.nms_ref(b, s, g, thr)
        assert len(set(keep.tolist())) == len(keep) and (len(keep) == 0 or (0 <= int(keep.min()) and int(keep.max()) < len(b))), name


def test_nms_order_is_torch_sort_and_the_old_rule_collides():
    """The rank table of the fix: under the old rule a NaN ranks with the best number of its group, so two boxes share a slot and
    another slot is never written; under the key order every slot is written once, NaN first as torch.sort places it."""
    s = np.array([0.5, NAN, 0.9, -NAN, 0.5], np.float32)
    assert R.nms_old_ranks(s).tolist() == [1, 0, 0, 0, 2]                        # slots 3 and 4 never written
    order = R.nms_order(s)
    assert order.tolist() == [1, 3, 2, 0, 4] and sorted(order.tolist()) == list(range(5))
    assert torch.sort(torch.from_numpy(s), descending=True, stable=True).indices.tolist() == order.tolist()
    for name, b, sc, g, thr in R.nms_cases():
        order = R.nms_order(sc.numpy(), None if g is None else g.numpy())
        assert sorted(order.tolist()) == list(range(len(sc))), name
        if g is None:
            assert order.tolist() == torch.sort(sc, descending=True, stable=True).indices.tolist(), name
            if "nan" in name and len(sc) >= 63:
                assert len(set(R.nms_old_ranks(sc.numpy()).tolist())) < len(sc), "%s would not notice the old order" % name
            # survivors come out in that order
            keep = R.nms_ref(b, sc, None, thr).tolist()
            pos = {int(v): i for i, v in enumerate(order)}
            assert all(pos[a] < pos[c] for a, c in zip(keep, keep[1:])), name


def test_select_rows_and_order():
    """select_smallest_ref is torch's ascending stable sort (NaN of either sign after +inf, in index order), whose first k values are
    torch.topk(largest=False)'s; the old all-pairs rule collides on every test row; the four shapes take the routes they name."""
    src = open(os.path.join(PKG, "csrc", "pose.hip")).read()
    assert "#define SR_STATIC_LDS (2048 * 4 + 64)" in src and "(size_t)(n + 2 * k) * 4 + SR_STATIC_LDS <= 65536" in src
    assert [R.select_route(n, k) for n, k in ((37, 37), (6000, 300), (14319, 1), (14400, 300))] == ["radix", "radix", "allpairs", "allpairs"]
    assert R.select_route(14318, 1) == "radix"
    for n, k, numbers in ((37, 37, None), (6000, 300, None), (14319, 1, None), (14400, 300, None), (6000, 300, 250), (14400, 300, 250)):
        row = R.select_row(n, numbers=numbers)
        bits = row.view(np.uint32)
        nan = np.isnan(row)
        assert (nan & (bits >> 31 == 1)).any() and (nan & (bits >> 31 == 0)).any()
        if numbers is None:
            assert 0 < nan.mean() < 0.1 if n > 100 else nan.any()
            if n > 100:
                assert np.isposinf(row).any() and np.isneginf(row).any() and ((row == 0) & np.signbit(row)).any() and ((row == 0) & ~np.signbit(row)).any()
        else:
            assert (~nan).sum() == numbers < k  # k reaches into the NaNs
        want = R.select_smallest_ref(row, k)
        t = torch.from_numpy(row.copy())
        assert np.array_equal(want, torch.sort(t, stable=True).indices[:k].numpy().astype(np.int32))
        tv = torch.topk(t, k, largest=False).values.numpy()
        assert np.array_equal(np.isnan(tv), np.isnan(row[want])) and np.array_equal(tv[~np.isnan(tv)], row[want][~np.isnan(tv)])
        if n <= 6000:
            ranks = R.select_old_ranks(row)
            assert len(set(ranks.tolist())) < n, "the old rank rule must collide on this row"
    assert R.select_old_ranks(np.array([0.5, NAN, 0.1, -NAN, 0.5], np.float32)).tolist() == [1, 0, 0, 0, 2]
    assert R.select_smallest_ref(np.array([0.5, NAN, 0.1, -NAN, 0.5, -np.inf, np.inf], np.float32), 7).tolist() == [5, 2, 0, 4, 6, 1, 3]


def test_keep_patterns():
    for N in R.INDEX_SIZES:
        p = R.keep_patterns(N)
        assert set(p) == {"none", "all", "first", "last", "alternating", "random"}
        if N > 1:
            assert np.flatnonzero(p["first"]).tolist() == [0] and np.flatnonzero(p["last"]).tolist() == [N - 1]
            assert p["random"].max() > 1 or N < 8  # any non-zero byte counts
