"""Regenerates tests/golden/sam_small_regions.npz with scipy.

Run by hand where scipy is installed; never imported by a test.  The inputs are the patterns of tests/small_regions_ref.py (stored as
packed bits, so the fixture does not depend on the generators staying as they are); everything expected is computed here with
scipy.ndimage.label (structure = ones((3, 3)): 8-connectivity) and plain numpy, not with the restatement: the cleaned masks of
remove_small_regions' two passes (ISM/segment_anything/utils/amg.py:267-291, holes first), `changed`, the boxes of the cleaned masks and
the component counts of every input and of its complement.  scipy numbers its labels in row-major order of their first pixel, so
np.argmax over the sizes picks, among equal largest islands, the one the package's rule picks.

    python tests/gen_sam_small_regions_golden.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import small_regions_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
EIGHT = np.ones((3, 3), dtype=np.int32)

# (H, W), seed, min_areas ("HW+1": one more than the image has pixels), patterns (None: all of R.patterns)
SETS = [
    ((70, 130), 200, (1, 2, 20, 100, "HW+1"), None),
    ((129, 191), 320, (1, 2, 20, 100, "HW+1"), None),
    ((480, 640), 11, (100,), ("blobs", "coin")),
]


def remove_small(mask, min_area, holes):
    work = ~mask if holes else mask
    lab, n = ndimage.label(work, structure=EIGHT)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    small = np.nonzero(sizes < min_area)[0] + 1
    if len(small) == 0:
        return mask, False
    if holes:
        return mask | np.isin(lab, small), True
    keep = np.setdiff1d(np.arange(1, n + 1), small)
    if len(keep) == 0:
        keep = [int(np.argmax(sizes)) + 1]
    return np.isin(lab, keep), True


def box(m):
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if len(ys) else [0, 0, 0, 0]


def main():
    out = {"n_sets": np.int64(len(SETS))}
    for j, ((H, W), seed, min_areas, names) in enumerate(SETS):
        pats = R.patterns(H, W, seed)
        names = tuple(pats) if names is None else names
        masks = np.stack([pats[n] for n in names])
        p = "s%d." % j
        out[p + "shape"] = np.array([H, W], dtype=np.int64)
        out[p + "names"] = np.array(names)
        out[p + "bits"] = np.packbits(masks.reshape(len(names), -1), axis=1)
        out[p + "n_fg"] = np.array([ndimage.label(m, structure=EIGHT)[1] for m in masks], dtype=np.int64)
        out[p + "n_bg"] = np.array([ndimage.label(~m, structure=EIGHT)[1] for m in masks], dtype=np.int64)
        ts = [H * W + 1 if t == "HW+1" else int(t) for t in min_areas]
        out[p + "min_areas"] = np.array(ts, dtype=np.int64)
        for t in ts:
            cleaned, changed = [], []
            for m in masks:
                m1, c1 = remove_small(m, t, True)
                m2, c2 = remove_small(m1, t, False)
                cleaned.append(m2)
                changed.append(c1 or c2)
            cleaned = np.stack(cleaned)
            q = p + "t%d." % t
            out[q + "cleaned"] = np.packbits(cleaned.reshape(len(names), -1), axis=1)
            out[q + "changed"] = np.array(changed, dtype=bool)
            out[q + "boxes"] = np.array([box(m) for m in cleaned], dtype=np.int64)
            print("%dx%d min_area %d: changed %s" % (H, W, t, np.array(changed).astype(int)))
    path = os.path.join(GOLD, "sam_small_regions.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
