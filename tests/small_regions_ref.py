"""SAM's min_mask_region_area clean-up restated in plain numpy (ISM/segment_anything/utils/amg.py:267-291 remove_small_regions,
ISM/segment_anything/automatic_mask_generator.py:324-372 postprocess_small_regions), with code of its own: what the library's
sam6d_mask_components / sam6d_amg_small_regions and sam6d_hip.amg.postprocess_small_regions are compared with, bit for bit.

Labelling is by row runs and union-find: the runs [x0, x1) of every row, two runs on neighbouring rows [p0, p1) and [x0, x1) touch
under 8-connectivity if p0 <= x1 and p1 >= x0.  Runs are numbered in row-major order of their first pixel and a union hangs the larger
root under the smaller, so a component's root is the run that holds its first pixel in row-major order.  tests/test_sam_small_regions_host
checks the partition against scipy.ndimage.label (structure = ones((3, 3))) and a stored fixture.

The two rules that are the package's own: among largest islands of equal area the one whose first pixel comes
first in row-major order stays; the NMS sorts by score descending, stable by index.

The input generators of the tests are here too (integer hashes: the same masks on every machine)."""
import math

import numpy as np

NEIGHBOURS_8 = np.ones((3, 3), dtype=np.int32)  # scipy.ndimage.label's structure for 8-connectivity


# ------------------------------------------------------------------------------------------------- labelling
def row_runs(mask):
    """(H, W) bool -> (y, x0, x1) of every row run [x0, x1), in row-major order."""
    H, W = mask.shape
    pad = np.zeros((H, W + 2), dtype=np.int8)
    pad[:, 1:-1] = mask
    d = np.diff(pad, axis=1)
    y, x0 = np.nonzero(d == 1)
    _, x1 = np.nonzero(d == -1)
    return y, x0, x1


def _find(parent, i):
    r = i
    while parent[r] != r:
        r = parent[r]
    while parent[i] != r:
        parent[i], i = r, parent[i]
    return r


def run_roots(mask):
    """-> (y, x0, x1, root): the runs and, per run, the index of the first run of its 8-connected component."""
    H, W = mask.shape
    y, x0, x1 = row_runs(mask)
    n = len(y)
    parent = list(range(n))
    first = np.searchsorted(y, np.arange(H + 1))  # runs of row r are first[r] .. first[r + 1] - 1
    a0, a1 = x0.tolist(), x1.tolist()
    for r in range(1, H):
        i, i_end = int(first[r - 1]), int(first[r])
        j, j_end = i_end, int(first[r + 1])
        while i < i_end and j < j_end:
            if a0[i] <= a1[j] and a1[i] >= a0[j]:
                ri, rj = _find(parent, i), _find(parent, j)
                if ri < rj:
                    parent[rj] = ri
                elif rj < ri:
                    parent[ri] = rj
            if a1[i] < a1[j]:  # the run that ends first cannot touch anything further right
                i += 1
            else:
                j += 1
    root = np.array([_find(parent, i) for i in range(n)], dtype=np.int64).reshape(-1)
    return y, x0, x1, root


def _paint(values, y, x0, x1, shape):
    """An (H, W) int64 image with values[i] on run i and 0 elsewhere."""
    H, W = shape
    d = np.zeros(H * W + 1, dtype=np.int64)
    np.add.at(d, y * W + x0, values)
    np.add.at(d, y * W + x1, -values)
    return np.cumsum(d)[:-1].reshape(H, W)


def components(mask):
    """(H, W) bool -> (labels, areas, first, size): labels (H, W) int32 = 0 off the mask, else 1 + the smallest row-major pixel index of
    the pixel's 8-connected component; areas (H, W) int32 = the component's pixel count, 0 off the mask; first, size: per component, in
    row-major order of the first pixel, that pixel's index and the pixel count."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    y, x0, x1, root = run_roots(mask)
    if len(y) == 0:
        z = np.zeros((H, W), dtype=np.int32)
        return z, z.copy(), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    start = y * W + x0
    area_of_root = np.bincount(root, weights=(x1 - x0), minlength=len(y)).astype(np.int64)
    labels = _paint(start[root] + 1, y, x0, x1, (H, W))
    areas = _paint(area_of_root[root], y, x0, x1, (H, W))
    roots = np.unique(root)
    return labels.astype(np.int32), areas.astype(np.int32), start[roots], area_of_root[roots]


def components_batch(masks, invert=False):
    """(K, H, W) -> labels, areas (K, H, W) int32 of masks != 0, or of masks == 0 with `invert`."""
    fg = (np.asarray(masks) != 0) != bool(invert)
    out = [components(m)[:2] for m in fg]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------------------------------------- the two passes
def remove_small(mask, min_area, holes):
    """One remove_small_regions call: (mask, changed).  holes: components of ~mask smaller than min_area are filled; islands:
    components of mask smaller than min_area are dropped, the largest (first in row-major order among equals) stays if all are."""
    work = ~mask if holes else mask
    labels, areas, first, size = components(work)
    small = size < min_area
    if not small.any():
        return mask, False
    if holes:
        return mask | (work & (areas < min_area)), True
    if small.all():
        return labels == int(first[int(np.argmax(size))]) + 1, True  # argmax: the first of equal maxima
    return work & (areas >= min_area), True


def clean(mask, min_area):
    """Both passes in the reference's order -> (cleaned (H, W) bool, changed)."""
    mask = np.asarray(mask) != 0
    mask, c1 = remove_small(mask, min_area, True)
    mask, c2 = remove_small(mask, min_area, False)
    return mask, bool(c1 or c2)


def mask_box(m):
    """batched_mask_to_box for one mask: xyxy inclusive, [0, 0, 0, 0] when empty."""
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def clean_batch(masks, min_area):
    """(K, H, W) -> cleaned (K, H, W) bool, changed (K) bool, boxes (K, 4) int64."""
    res = [clean(m, min_area) for m in masks]
    cleaned = np.stack([r[0] for r in res]) if len(res) else np.zeros(np.shape(masks), dtype=bool)
    return cleaned, np.array([r[1] for r in res], dtype=bool), np.array([mask_box(m) for m in cleaned], dtype=np.int64).reshape(-1, 4)


def nms_stable(boxes, scores, thresh):
    """torchvision.ops.nms in fp32 with a stable sort: kept indices, score descending, equal scores in index order."""
    b = np.asarray(boxes, dtype=np.float32)
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept, removed = [], np.zeros(len(b), dtype=bool)
    for n, i in enumerate(order):
        if removed[i]:
            continue
        kept.append(int(i))
        for j in order[n + 1:]:
            if removed[j]:
                continue
            w = max(np.float32(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            h = max(np.float32(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = np.float32(w * h)
            with np.errstate(invalid="ignore", divide="ignore"):
                if inter / np.float32(area[i] + area[j] - inter) > np.float32(thresh):
                    removed[j] = True
    return np.array(kept, dtype=np.int64)


def postprocess(masks, boxes_in, min_area, nms_thresh):
    """postprocess_small_regions: masks (K, H, W), boxes_in (K, 4) -> (masks, boxes) of the survivors in NMS order."""
    cleaned, changed, boxes = clean_batch(masks, min_area)
    keep = nms_stable(boxes, (~changed).astype(np.float32), nms_thresh)
    out = np.where(changed[:, None], boxes, np.asarray(boxes_in))
    return cleaned[keep], out[keep], keep


def threshold(min_area):
    """`size < min_area` for integer sizes is `size < ceil(min_area)`."""
    return int(math.ceil(min_area))


# ------------------------------------------------------------------------------------------------- inputs
def hash01(H, W, seed):
    """(H, W) float64 in [0, 1) from an integer hash of (y, x, seed)."""
    y, x = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    h = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (np.uint64(seed) * np.uint64(83492791) + np.uint64(0x9E3779B9))
    for _ in range(2):
        h = (h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
        h = (h ^ (h >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(15))
    return (h & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)


def blobs(H, W, seed, k=7):
    """Box-filtered hash noise thresholded at its median: smooth regions with small islands and holes along their borders."""
    v = hash01(H, W, seed)
    pad = np.pad(v, ((k // 2, k - 1 - k // 2), (k // 2, k - 1 - k // 2)), mode="wrap")
    c = np.cumsum(np.cumsum(np.pad(pad, ((1, 0), (1, 0))), axis=0), axis=1)
    box = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    return box > np.median(box)


def coin(H, W, seed):
    return hash01(H, W, seed) < 0.5


def serpentine(H, W):
    """A one-pixel path over the whole image: every other row is full, the rows between hold one pixel at alternating ends."""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def comb(H, W):
    """Teeth in every other column, joined only along the last row."""
    m = np.zeros((H, W), dtype=bool)
    m[:, 0::2] = True
    m[H - 1] = True
    return m


def checkerboard(H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (y + x) % 2 == 0


def diagonal(H, W):
    """A one-pixel staircase from corner to corner (8-connected, not 4-connected)."""
    m = np.zeros((H, W), dtype=bool)
    n = max(H, W)
    t = np.arange(n)
    m[(t * (H - 1)) // max(n - 1, 1), (t * (W - 1)) // max(n - 1, 1)] = True
    return m


def lattice(H, W):
    """Isolated pixels on the stride-2 lattice: the largest possible component count."""
    m = np.zeros((H, W), dtype=bool)
    m[0::2, 0::2] = True
    return m


def patterns(H, W, seed=0):
    """name -> (H, W) bool: the labelling cases of the GPU tests."""
    s, d = serpentine(H, W), diagonal(H, W)
    return {"blobs": blobs(H, W, seed), "coin": coin(H, W, seed + 1), "serpentine": s, "serpentine_complement": ~s, "comb": comb(H, W),
            "checkerboard": checkerboard(H, W), "diagonal": d, "diagonal_complement": ~d, "lattice": lattice(H, W),
            "zeros": np.zeros((H, W), dtype=bool), "ones": np.ones((H, W), dtype=bool)}
