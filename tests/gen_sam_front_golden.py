"""Writes tests/golden/sam_front.npz: what Pillow's bilinear resize makes of seeded images at the sizes ResizeLongestSide asks for
(ISM/segment_anything/utils/transforms.py:26-31, 91-102).  Run where Pillow is installed: python -m tests.gen_sam_front_golden

Per small case NAME: in_NAME (H, W, 3) uint8, out_NAME = np.asarray(PIL.Image.fromarray(in).resize((ow, oh), BILINEAR)), side_NAME.
Per large case (side 1024, the input rebuilt from its seed by `noise`): sha_HxW = the sha256 of Pillow's output bytes, seed_HxW."""
import hashlib
import os

import numpy as np

from tests.pil_bilinear import preprocess_shape

# name: (H, W, side, fill)  fill: None = seeded noise, else the constant byte
SMALL = {
    "enlarge_landscape": (33, 47, 64, None),   # -> 45 x 64: the output height is no multiple of 16
    "enlarge_portrait": (50, 35, 96, None),    # -> 96 x 67
    "shrink_1p9": (122, 304, 160, None),       # 4 taps
    "shrink_3p3": (100, 159, 48, None),        # 7 taps
    "shrink_3p6": (120, 230, 64, None),        # 8 taps
    "shrink_4": (195, 260, 64, None),          # 9 taps (scale 4.0625)
    "shrink_4_exact": (64, 256, 64, None),     # 8 taps
    "shrink_portrait": (151, 87, 48, None),
    "width_unchanged": (100, 3, 96, None),     # -> 96 x 3: the horizontal pass is skipped
    "height_unchanged": (3, 160, 160, None),   # identity on both axes
    "identity": (48, 64, 64, None),
    "one_pixel": (1, 1, 64, None),             # -> 64 x 64
    "one_row": (1, 50, 64, None),              # -> 1 x 64
    "one_column": (50, 1, 64, None),           # -> 64 x 1
    "all_0": (20, 30, 64, 0),
    "all_255": (20, 30, 64, 255),
    "all_255_shrink": (130, 200, 64, 255),
    "tall": (1100, 10, 64, None),              # -> 64 x 1, over 100 times as tall as wide: Image.resize runs the vertical pass first
}
LARGE = ((480, 640), (1080, 1920), (1500, 700))
SEED = 20250340


def noise(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def small_input(i, name):
    h, w, side, fill = SMALL[name]
    return noise(SEED + i, h, w) if fill is None else np.full((h, w, 3), fill, dtype=np.uint8)


def pil_resize(img, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, name in enumerate(SMALL):
        h, w, side, _ = SMALL[name]
        img = small_input(i, name)
        out["in_" + name], out["side_" + name] = img, np.int64(side)
        out["out_" + name] = pil_resize(img, *preprocess_shape(h, w, side))
    for i, (h, w) in enumerate(LARGE):
        seed = SEED + 100 + i
        got = pil_resize(noise(seed, h, w), *preprocess_shape(h, w, 1024))
        out["sha_%dx%d" % (h, w)] = np.array(hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest())
        out["seed_%dx%d" % (h, w)] = np.int64(seed)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_front.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
