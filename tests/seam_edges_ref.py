"""TEST INFRASTRUCTURE ONLY -- case builders and a plain numpy restatement for the integer / byte kernels at the ISM -> PEM seam
(csrc/detections.hip, csrc/testdata.hip, sam6d_depth_to_cloud of csrc/next.hip, sam6d_select_smallest of csrc/pose.hip), at the
edges their golden scenes never reach: image sizes that are no multiple of the wave, crops that cut valid pixels off, counts on a
1024-thread chunk edge, an explicit cap, areas and IoUs exactly at their thresholds, NaN scores and distances.

The restatement is composed from oracle.pem_oracle (get_bbox, depth_to_cloud, get_resize_rgb_choose) and oracle.ism_oracle
(small_detection_keep, nms, nms_per_object_id); unlike oracle.pem_oracle.proposal_geometry it returns every intermediate also for the
proposals the reference skips.  tests/test_seam_edges_host.py checks on the CPU that each case family really contains the edge it
is named for; tests/test_seam_edges_gpu.py compares the kernels with it bit for bit."""
import numpy as np
import torch

from oracle import ism_oracle as IO
from oracle import pem_oracle as O

SIZES = [(1, 40), (40, 1), (3, 100), (100, 3), (37, 53), (64, 64), (65, 63), (96, 130)]
MASK_VALUES = np.array([1, 128, 254, 255], np.uint8)  # proposals count every non-zero value, templates only 255
K_EDGE = np.array([[150.25, 0.0, 31.7], [0.0, 149.5, 20.3], [0.0, 0.0, 1.0]], np.float32)  # non-integer cx, cy


# ------------------------------------------------------------------------------------------------------------ images
def depth_map(H, W, seed=0):
    """(H,W) f32 metres with about 10 % zeros; the four corners are positive and the centre pixel is a zero at every size."""
    g = np.random.default_rng(1000 + seed + 7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (0.5 + 0.004 * xx + 0.003 * yy + 0.3 * g.random((H, W))).astype(np.float32)
    d[g.random((H, W)) < 0.1] = 0
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        d[r, c] = np.float32(0.75)
    if H * W > 4:
        d[H // 2, W // 2] = 0
    return d


def _paint(g, shape, where):
    m = np.zeros(shape, np.uint8)
    vals = MASK_VALUES[g.integers(0, len(MASK_VALUES), size=shape)]
    m[where] = vals[where]
    return m


def mask_families(H, W, depth, seed=0):
    """[(family name, (H,W) u8 mask)]: the mask families of the geometry tests, values drawn from MASK_VALUES."""
    g = np.random.default_rng(2000 + seed + 13 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []

    def add(name, where):
        out.append((name, _paint(g, (H, W), where)))

    add("zero", np.zeros((H, W), bool))
    add("depth_zero_only", depth == 0)
    for name, (r, c) in (("corner_tl", (0, 0)), ("corner_tr", (0, W - 1)), ("corner_bl", (H - 1, 0)), ("corner_br", (H - 1, W - 1))):
        add(name, (yy == r) & (xx == c))
    add("full_row", yy == H // 2)
    add("full_col", xx == W // 2)
    add("full", np.ones((H, W), bool))
    for s in (11, 12):  # bars two pixels thick and s long (odd and even side) along each border: each shift branch of get_bbox
        rc, cc = max(0, (H - s) // 2), max(0, (W - s) // 2)
        add("rect%d_top" % s, (yy < 2) & (xx >= cc) & (xx < cc + s))
        add("rect%d_bottom" % s, (yy >= H - 2) & (xx >= cc) & (xx < cc + s))
        add("rect%d_left" % s, (xx < 2) & (yy >= rc) & (yy < rc + s))
        add("rect%d_right" % s, (xx >= W - 2) & (yy >= rc) & (yy < rc + s))
    add("two_clusters", ((yy < 2) & (xx < 2)) | ((yy >= H - 2) & (xx >= W - 2)))
    for k in range(2):
        cy, cx = g.integers(0, H), g.integers(0, W)
        r = int(g.integers(2, max(3, max(H, W) // 2)))
        add("blob%d" % k, (((xx - cx) ** 2 + (yy - cy) ** 2) < r * r) & (g.random((H, W)) > 0.25))
    return out


def xyz_maps(T, H, W, seed=0):
    """(T,H,W,3) f32 millimetres: values whose quotient by 1000 is not exact in fp32."""
    g = np.random.default_rng(3000 + seed + H + W)
    return ((g.random((T, H, W, 3)) - 0.5) * 431.7).astype(np.float32)


CHUNK_NAMES = ["crop32_valid1024", "crop34_full", "crop34_valid1025", "crop34_valid1024", "crop36_full", "crop64_full", "crop2"]
CHUNK_RADII = (10.0, 0.05, 1e-4)  # keeps everything / a part (in-place compaction across chunks) / fewer than 4


def chunk_edge_scene():
    """64x64: proposals whose crops and valid counts sit on the 1024-thread chunk edges of the crop and radius-filter kernels, and
    the crop sides 2, 34, 36 and 64 of the choose test.  -> (depth, masks (7,64,64) u8), proposals named by CHUNK_NAMES.  The depth
    is positive everywhere, so the mask alone decides the counts."""
    H = W = 64
    g = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (0.6 + 0.002 * xx + 0.001 * yy + 0.05 * g.random((H, W))).astype(np.float32)
    m = np.zeros((len(CHUNK_NAMES), H, W), bool)
    m[0, 10:42, 20:52] = True  # 32x32 = 1024 pixels: exactly one chunk of the crop and of the filter
    m[1, 3:37, 8:42] = True    # 34x34 = 1156: a second, short chunk
    for i, want in ((2, 1025), (3, 1024)):  # the same 34x34 crop (its border rows and columns stay), thinned inside
        m[i] = m[1]
        inner = np.argwhere(m[i][4:36, 9:41]) + np.array([4, 9])
        for r, c in inner[g.permutation(len(inner))[: 1156 - want]]:
            m[i, r, c] = False
    m[4, 20:56, 1:37] = True   # 36x36
    m[5] = True                # the whole image
    m[6, 30:32, 62:64] = True  # 2x2 on the right border
    masks = _paint(g, (len(CHUNK_NAMES), H, W), m)
    return depth, masks


# ------------------------------------------------------------------------------------------------------------ geometry
def _bbox(valid):
    return O.get_bbox(valid) if valid.any() else [0, 0, 0, 0]  # the library's answer for an empty mask (the reference skips it)


def _sequential_mean(cloud):
    """np.mean(axis=0) of an (n,3) float32 array as numpy evaluates it: a sequential fp32 sum over the rows, then / n."""
    s = np.zeros(3, np.float32)
    for row in cloud:
        s = s + row
    return s / np.float32(len(cloud)) if len(cloud) else s


def proposal_geometry(mask, depth, K, radius, cap=None):
    """Every intermediate of one proposal of get_test_data (PEM/run_inference_custom_pytorch.py:316-337), also where the reference
    skips it: bbox and count; the raster-order choose and cloud of the crop (the first `cap` of them); the sequential-fp32 centre
    (zeros for an empty crop, where numpy's mean is NaN and the reference moves on); the set kept at
    float32(float64(float32(radius)) * 1.2)."""
    valid = np.logical_and(mask != 0, depth > 0)
    bbox = _bbox(valid)
    y1, y2, x1, x2 = bbox
    choose = valid[y1:y2, x1:x2].flatten().nonzero()[0]
    cloud = O.depth_to_cloud(depth, K, bbox).reshape(-1, 3)[choose, :]
    if cap is not None:
        choose, cloud = choose[:cap], cloud[:cap]
    center = _sequential_mean(cloud)
    thr = np.float32(np.float64(np.float32(radius)) * 1.2)
    flag = np.linalg.norm(cloud - center[None, :], axis=1) < thr
    return dict(bbox=bbox, count=int(valid.sum()), n_valid=len(choose), choose=choose.astype(np.int32), cloud=cloud, center=center,
                keep_choose=choose[flag].astype(np.int32), keep_cloud=cloud[flag])


def template_geometry(mask, xyz_mm, cap=None):
    """_get_template up to the choice (PEM/run_inference_custom_pytorch.py:199-219): valid = mask == 255, xyz = float32 map / 1000."""
    valid = mask == 255
    bbox = _bbox(valid)
    y1, y2, x1, x2 = bbox
    choose = valid[y1:y2, x1:x2].flatten().nonzero()[0]
    cloud = (xyz_mm[y1:y2, x1:x2, :].reshape(-1, 3)[choose, :] / np.float32(1000.0)).astype(np.float32)
    if cap is not None:
        choose, cloud = choose[:cap], cloud[:cap]
    return dict(bbox=bbox, count=int(valid.sum()), n_valid=len(choose), choose=choose.astype(np.int32), cloud=cloud)


def rgb_choose(choose, bbox, img_size):
    return O.get_resize_rgb_choose(np.asarray(choose, np.int64), bbox, img_size)


def cuts_valid_pixels(geom):
    return geom["n_valid"] < geom["count"]


# ------------------------------------------------------------------------------------------------------------ small keep
def small_keep_cases():
    """[(name, boxes (N,4) i64, masks (N,H,W) f32, min_box_size, min_mask_size)].  The kernel takes thr_box = min_box_size ** 2."""
    out = []
    big = 1 << 33
    for H, W in ((1, 1), (3, 5), (7, 9), (2, 2), (4, 6)):
        g = np.random.default_rng(H * 31 + W)
        hw = H * W
        boxes = [[0, 0, W, H], [0, 0, 0, H], [2, 0, 1, H], [W, H, 0, 0], [0, 0, 1, 1], [big, big, big + W, big + H],
                 [-big, 0, -big + 1, 1], [0, 0, big, 1], [0, 0, big, -1]]
        n = len(boxes)
        masks = (g.random((n, H, W)) < 0.6).astype(np.float32)
        masks[0] = 1
        masks[1] = 0
        out.append(("rand_%dx%d" % (H, W), torch.tensor(boxes, dtype=torch.int64), torch.from_numpy(masks), 0.5, 0.5 / hw))
    # fractions exactly at the threshold (strict >) and one above: 4 of 16 at 0.25, 5 of 16
    H, W = 4, 4
    masks = np.zeros((6, H, W), np.float32)
    masks[0].flat[:4] = 1
    masks[1].flat[:5] = 1
    masks[2:] = 1
    boxes = [[0, 0, 4, 4], [0, 0, 4, 4], [0, 0, 2, 2], [0, 0, 5, 1], [1, 1, 3, 3], [0, 0, 1, 5]]  # areas 16, 16, 4, 5, 4, 5
    out.append(("at_threshold_4x4", torch.tensor(boxes, dtype=torch.int64), torch.from_numpy(masks), 0.5, 0.25))
    # the same on the scalar path, H*W = 5*5: 5 of 25 mask pixels at 0.2 -- float32(5) / float32(25) rounds to float32(0.2), the
    # threshold the kernel receives -- and a box of area 25 at min_box_size 1.0
    H, W = 5, 5
    masks = np.zeros((4, H, W), np.float32)
    masks[0].flat[:5] = 1
    masks[1].flat[:6] = 1
    masks[2:] = 1
    boxes = [[0, 0, 13, 2], [0, 0, 13, 2], [0, 0, 5, 5], [0, 0, 13, 2]]  # areas 26, 26, 25, 26 against 1.0 * 25
    out.append(("at_threshold_5x5", torch.tensor(boxes, dtype=torch.int64), torch.from_numpy(masks), 1.0, 0.2))
    return out


def small_keep_ref(boxes, masks, thr_box, thr_mask):
    """keep[i] = area / (H*W) > thr_box and sum / (H*W) > thr_mask with the thresholds the kernel receives as floats: the oracle's
    rule (torch's int64 / int true_divide -> fp32) on the squared box threshold."""
    img = masks.shape[1] * masks.shape[2]
    box_areas = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) / img
    mask_areas = masks.sum(dim=(1, 2)) / img
    return torch.logical_and(box_areas > np.float32(thr_box).item(), mask_areas > np.float32(thr_mask).item())


# ------------------------------------------------------------------------------------------------------------ indices and rows
INDEX_SIZES = [0, 1, 63, 64, 65, 128, 129, 4500]


def keep_patterns(N):
    g = np.random.default_rng(N + 5)
    pats = {"none": np.zeros(N, np.uint8), "all": np.full(N, 1, np.uint8), "first": np.zeros(N, np.uint8), "last": np.zeros(N, np.uint8),
            "alternating": (np.arange(N) % 2).astype(np.uint8), "random": (g.random(N) < 0.4).astype(np.uint8) * np.uint8(200)}
    if N:
        pats["first"][0] = 255
        pats["last"][-1] = 1
    return pats


# ------------------------------------------------------------------------------------------------------------ NMS
NMS_SIZES = [1, 2, 63, 64, 65, 128, 129, 1025]
IOU_PAIR = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], np.float32)  # IoU = 50 / (100 + 50 - 50) = 0.5 exactly


def iou_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.maximum(np.float32(0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
    h = np.maximum(np.float32(0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    inter = np.float32(w * h)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def nms_boxes(N, seed=0):
    """(N,4) f32 fractional boxes: clusters of near-duplicates, exact duplicates, zero-area and inverted boxes, and IOU_PAIR."""
    g = torch.Generator().manual_seed(N * 17 + seed)
    xy = torch.rand(N, 2, generator=g) * 60
    wh = torch.rand(N, 2, generator=g) * 30 + 2.5
    b = torch.cat([xy, xy + wh], 1)
    if N >= 8:
        h = N // 2
        b[h:] = b[: N - h] + (torch.rand(N - h, 4, generator=g) - 0.5) * 4  # near-duplicates of the first half
        b[h + 1] = b[1]                       # an exact duplicate
        b[2, 2:] = b[2, :2]                   # zero area
        b[3, 2] = b[3, 0] - 3.25              # inverted in x
        b[4, 2:] = b[4, :2] - 1.5             # inverted in both
        b[5] = b[2]                           # two identical zero-area boxes: IoU 0/0
    if N >= 2:
        b[N - 2:] = torch.from_numpy(IOU_PAIR)
    return b


def nms_scores(N, kind, seed=0):
    g = torch.Generator().manual_seed(N * 29 + seed)
    if kind == "ties":
        return (torch.rand(N, generator=g) * 20).round() / 20
    if kind == "equal":
        return torch.full((N,), 0.5)
    if kind == "zeros":
        s = torch.zeros(N)
        s[::2] = -0.0
        s[::5] = 0.25
        return s
    if kind == "nan":  # NaN of both signs among tied numbers, -0 / +0 and infinities
        s = (torch.rand(N, generator=g) * 8).round() / 8 - 0.25
        s[torch.rand(N, generator=g) < 0.2] = float("nan")
        neg = torch.rand(N, generator=g) < 0.5
        s = torch.where(torch.isnan(s) & neg, -torch.tensor(float("nan")), s)
        if N >= 8:
            s[0], s[1], s[6], s[7] = float("inf"), -float("inf"), -0.0, 0.0
        return s
    return torch.rand(N, generator=g)


def nms_groups(N, kind, seed=0):
    """int64 ids: 'wide' = four ids, one beyond 32 bits, one negative; 'one'; 'each' = N groups of one (descending, so the output
    order is not the input order)."""
    g = torch.Generator().manual_seed(N * 3 + seed)
    if kind == "one":
        return torch.full((N,), 7, dtype=torch.int64)
    if kind == "each":
        return torch.arange(N, 0, -1, dtype=torch.int64) * ((1 << 33) + 1) - (1 << 34)
    ids = torch.tensor([(1 << 40) + 3, -((1 << 35) + 1), 0, 5], dtype=torch.int64)
    return ids[torch.randint(0, 4, (N,), generator=g)]


def nms_cases():
    """[(name, boxes, scores, group or None, thresh)]"""
    out = []
    for N in NMS_SIZES:
        b = nms_boxes(N)
        out.append(("ties_N%d" % N, b, nms_scores(N, "ties"), None, 0.5))
        out.append(("wide_groups_N%d" % N, b, nms_scores(N, "ties", 1), nms_groups(N, "wide"), 0.5))
        out.append(("nan_N%d" % N, b, nms_scores(N, "nan"), None, 0.5))
        out.append(("nan_groups_N%d" % N, b, nms_scores(N, "nan", 1), nms_groups(N, "wide", 1), 0.25))
    for N in (65, 129):
        b = nms_boxes(N, 1)
        out.append(("thr0_N%d" % N, b, nms_scores(N, "rand"), None, 0.0))
        out.append(("thr1_N%d" % N, b, nms_scores(N, "rand"), None, 1.0))
        out.append(("equal_N%d" % N, b, nms_scores(N, "equal"), None, 0.5))
        out.append(("zeros_N%d" % N, b, nms_scores(N, "zeros"), nms_groups(N, "wide"), 0.5))
        out.append(("one_group_N%d" % N, b, nms_scores(N, "ties"), nms_groups(N, "one"), 0.5))
        out.append(("each_group_N%d" % N, b, nms_scores(N, "ties"), nms_groups(N, "each"), 0.0))
        # a group that is all NaN: every box of id 5 gets a NaN score
        s, grp = nms_scores(N, "nan", 2), nms_groups(N, "wide", 2)
        s[grp == 5] = float("nan")
        s[(grp == 5) & (torch.arange(N) % 2 == 0)] = -float("nan")
        out.append(("all_nan_group_N%d" % N, b, s, grp, 0.5))
    return out


def nms_ref(boxes, scores, group, thresh):
    if group is None:
        return IO.nms(boxes, scores, thresh)
    return IO.nms_per_object_id(boxes, scores, group, thresh)


def nms_order(scores, group=None):
    """The library's total order: group ascending, then a NaN of either sign before every number, score descending with -0 == +0,
    index ascending -- torch.sort(descending=True, stable=True) inside each id.  A permutation of 0..N-1 for any input."""
    s = np.asarray(scores, np.float32)
    nan = np.isnan(s)
    grp = np.zeros(len(s), np.int64) if group is None else np.asarray(group, np.int64)
    return np.lexsort((np.arange(len(s)), -np.where(nan, np.float32(0), s), ~nan, grp))


def nms_old_ranks(scores):
    """The rank rule nms_order_kernel used before it ranked by integer keys, sj > si or (sj == si and j < i), inside one group: for
    showing on the CPU that a NaN makes it collide (tests/test_seam_edges_host.py)."""
    s = np.asarray(scores, np.float32)
    idx = np.arange(len(s))
    with np.errstate(invalid="ignore"):
        return np.array([int(np.sum((s > s[i]) | ((s == s[i]) & (idx < i)))) for i in range(len(s))])


# ------------------------------------------------------------------------------------------------------------ select smallest
SELECT_RADIX_LDS = 65536 - (2048 * 4 + 64)  # select_radix_kernel's dynamic LDS limit: (n + 2k) * 4 bytes must fit (csrc/pose.hip)


def select_route(n, k):
    """The dispatch condition of sam6d_select_smallest, restated: 'radix' while (n + 2k) * 4 bytes fit beside the histogram."""
    return "radix" if (n + 2 * k) * 4 <= SELECT_RADIX_LDS else "allpairs"


def select_row(n, seed=0, numbers=None):
    """One row of n distances: ties, +-0, +-inf and about 1 % NaN of both signs.  numbers = how many entries are not NaN (default:
    about 99 %)."""
    g = np.random.default_rng(4000 + seed + n)
    d = (g.integers(0, max(2, n // 3), size=n) / np.float32(max(2, n // 3))).astype(np.float32)  # many exact ties
    d[g.random(n) < 0.03] = np.float32(0.0)
    d[g.random(n) < 0.03] = np.float32(-0.0)
    d[g.random(n) < 0.01] = np.float32(np.inf)
    d[g.random(n) < 0.01] = np.float32(-np.inf)
    d[g.random(n) < 0.05] *= np.float32(-1)
    if numbers is None:
        nan = g.random(n) < 0.01
        if n >= 8:
            nan[[1, n - 1]] = True
    else:
        nan = np.ones(n, bool)
        nan[g.permutation(n)[:numbers]] = False
    neg = g.random(n) < 0.5
    if numbers is None and n >= 8:
        neg[1], neg[n - 1] = False, True  # both signs in every row
    bits = d.view(np.uint32).copy()
    bits[nan & ~neg] = np.uint32(0x7FC00000) | g.integers(0, 1 << 22, size=int((nan & ~neg).sum()), dtype=np.uint32)
    bits[nan & neg] = np.uint32(0xFFC00000) | g.integers(0, 1 << 22, size=int((nan & neg).sum()), dtype=np.uint32)
    return bits.view(np.float32)


def select_smallest_ref(row, k):
    """sel = the first k indices under the sort key (isnan, value, index): numbers ascending with -0 == +0 and equal values in index
    order, then every NaN of either sign in index order -- where torch.topk(largest=False) puts them."""
    row = np.asarray(row, np.float32)
    nan = np.isnan(row)
    val = np.where(nan, np.float32(0), row)
    order = np.lexsort((np.arange(len(row)), val, nan))
    return order[:k].astype(np.int32)


def select_old_ranks(row):
    """The rank rule the all-pairs kernel used before it ranked by integer keys, o < v or (o == v and j < i), for showing on the CPU
    that a NaN makes it collide (tests/test_seam_edges_host.py)."""
    row = np.asarray(row, np.float32)
    idx = np.arange(len(row))
    with np.errstate(invalid="ignore"):
        return np.array([int(np.sum((row < row[i]) | ((row == row[i]) & (idx < i)))) for i in range(len(row))])
