"""CPU checks of the numpy restatement of cv2.resize(INTER_LINEAR) that pins the device rgb crop (tests/cv2_linear.py): against a
float64 bilinear with OpenCV's coordinate map, the identity and 2x special cases, and cv2 itself where it imports."""
import numpy as np
import pytest

from tests import cv2_linear as CV

SIDES = [448, 480, 300, 130, 34, 2, 225, 447]


def _img(g, h, w):
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("side", SIDES)
def test_restatement_within_one_level_of_float64_bilinear(side):
    g = np.random.default_rng(side)
    src = _img(g, side, side)
    got = CV.resize_linear(src, 224).astype(np.float64)  # at 448 the INTER_AREA fast path: the same bilinear at exactly 1/2
    want = CV.bilinear_f64(src, 224)
    assert got.shape == (224, 224, 3)
    assert np.abs(got - want).max() <= 1.0


def test_restatement_rectangular_and_smooth_images():
    g = np.random.default_rng(7)
    yy, xx = np.mgrid[0:97, 0:203]
    src = np.stack([(xx + yy) % 256, (2 * xx) % 256, (yy * 3) % 256], -1).astype(np.uint8)
    assert np.abs(CV.resize_linear(src, 224).astype(np.float64) - CV.bilinear_f64(src, 224)).max() <= 1.0
    src = _img(g, 61, 17)
    assert np.abs(CV.resize_linear(src, 224).astype(np.float64) - CV.bilinear_f64(src, 224)).max() <= 1.0


def test_identity_at_side_S():
    g = np.random.default_rng(1)
    src = _img(g, 224, 224)
    assert np.array_equal(CV.resize_linear(src, 224), src)


def test_fixed_point_path_is_identity_at_unit_scale():
    """The bilinear fixed-point arithmetic itself (not the copy short-cut) reproduces the source at scale 1."""
    g = np.random.default_rng(2)
    src = _img(g, 40, 40).astype(np.int64)
    sx, a0, a1 = CV.taps(40, 40, True)
    assert np.array_equal(sx, np.arange(40)) and (a0 == 2048).all() and (a1 == 0).all()


def test_side_2S_is_rounded_2x2_mean():
    g = np.random.default_rng(3)
    src = _img(g, 448, 448)
    s = src.astype(np.int64)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) // 4
    assert np.array_equal(CV.resize_linear(src, 224), want.astype(np.uint8))


def test_vertical_pass_is_the_vectorised_form():
    """t_k = (sat16(H_k >> 4) * b_k) >> 16, (t0 + t1 + 2) >> 2 -- within one level of the scalar (H0 b0 + H1 b1 + 2^21) >> 22."""
    g = np.random.default_rng(4)
    src = _img(g, 300, 300)
    h, w = 300, 300
    sx, a0, a1 = CV.taps(w, 224, True)
    s = src.astype(np.int64)
    nxt = np.minimum(sx + 1, w - 1)
    hx = s[:, sx] * a0[None, :, None] + s[:, nxt] * a1[None, :, None]
    sy, b0, b1 = CV.taps(h, 224, False)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    scalar = (hx[y0] * b0[:, None, None] + hx[y1] * b1[:, None, None] + (1 << 21)) >> 22
    got = CV.resize_linear(src, 224).astype(np.int64)
    assert np.abs(got - scalar).max() <= 1


def test_normalise_recipe():
    g = np.random.default_rng(5)
    u8 = _img(g, 8, 8)
    t = CV.to_tensor_normalize(u8).numpy()
    for c in range(3):
        want = ((u8[:, :, c].astype(np.float32) / np.float32(255)) - np.float32(CV.MEAN[c])) / np.float32(CV.STD[c])
        assert np.array_equal(t[c], want.astype(np.float32))


@pytest.mark.parametrize("side", SIDES)
def test_restatement_matches_cv2(side):
    cv2 = pytest.importorskip("cv2")
    g = np.random.default_rng(100 + side)
    src = _img(g, side, side)
    got = CV.resize_linear(src, 224).astype(np.int64)
    want = cv2.resize(src, (224, 224), interpolation=cv2.INTER_LINEAR).astype(np.int64)
    d = np.abs(got - want)
    assert d.max() <= 1 and (d == 0).mean() >= 0.99
