"""The device draw of the point choices (sam6d_hip.inputs.draw_choice over csrc/choice.hip, and `rng=DeviceChoice(seed)` of
inputs.test_data / inputs.templates) against the numpy restatement of its definition (tests/choice_ref.py): bit for bit."""
import numpy as np
import pytest
import torch

from tests import choice_ref as R
from sam6d_hip import _lib, inputs

pytestmark = pytest.mark.gpu

H, W = 480, 640
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def _counts(ns):
    """every path of the kernel in one launch: an empty row, one candidate, the with-replacement side of the threshold (ns - 1, ns),
    the first row that sorts (ns + 1), 2 ns, and rows of many passes per thread up to a 1080 x 1080 crop"""
    return [0, 1, ns - 1, ns, ns + 1, 2 * ns, 70001, 230400, 1166400]


@pytest.mark.parametrize("seed", [3, 0xDEADBEEF])
@pytest.mark.parametrize("ns", [1, 3, 100, 2048, 5000, 8192])
def test_draw_choice_equals_the_restatement(dev, ns, seed):
    counts = _counts(ns)
    n = torch.tensor(counts, dtype=torch.int32, device=dev)
    got = inputs.draw_choice(n, ns, seed)
    assert got.shape == (9, ns) and got.dtype == torch.int32 and got.device == n.device
    whole = got.cpu().numpy()
    want = R.draw(counts, ns, seed)
    for i, c in enumerate(counts):
        assert np.array_equal(whole[i], want[i]), ("row", i, c, int((whole[i] != want[i]).sum()))
        if c > ns:  # ns distinct values below n
            assert whole[i].min() >= 0 and whole[i].max() < c and np.unique(whole[i]).size == ns, ("row", i, c)
    assert torch.equal(inputs.draw_choice(n, ns, seed), got)  # two calls are bitwise equal
    assert torch.equal(inputs.draw_choice(n[4:], ns, seed, row0=4), got[4:])  # rows 4 .. 8 on their own


def test_rows_wrap_and_large_counts_are_clamped(dev):
    n = torch.tensor([500, 9, (1 << 24) + 5, 1 << 24], dtype=torch.int32, device=dev)
    got = inputs.draw_choice(n, 16, 5, row0=0xFFFFFFFF).cpu().numpy()  # rows 2^32 - 1, 0, 1, 2
    assert np.array_equal(got[0], R.draw_row(5, 0xFFFFFFFF, 500, 16))
    assert np.array_equal(got[1], R.draw_row(5, 0, 9, 16))
    over, cap = (inputs.draw_choice(torch.tensor([c], dtype=torch.int32, device=dev), 16, 5, row0=7).cpu().numpy()[0] for c in
                 ((1 << 24) + 5, 1 << 24))  # the same row of the stream, once with a count above 2^24
    assert np.array_equal(over, cap) and np.unique(cap).size == 16 and cap.max() < 1 << 24
    assert np.array_equal(got[3], inputs.draw_choice(n[3:], 16, 5, row0=2).cpu().numpy()[0])
    h = R.keys(5, 7, np.arange(1 << 24))
    low = np.argpartition(h, 16)[:16]
    assert np.array_equal(cap, low[np.argsort(h[low])])  # the 16 smallest keys of 2^24, without sorting them all


def test_guard_values_and_refusals(dev):
    ns, counts, G = 100, [0, 7, 100, 101, 5000], 64
    n = torch.tensor(counts, dtype=torch.int32, device=dev)
    buf = torch.full((2 * G + len(counts) * ns,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("sam6d_draw_choice", n.data_ptr(), len(counts), ns, 11, 2, buf.data_ptr() + 4 * G, stream)
    out = buf.cpu().numpy()
    assert (out[:G] == -7).all() and (out[-G:] == -7).all()
    assert np.array_equal(out[G:-G].reshape(len(counts), ns), R.draw(counts, ns, 11, row0=2))
    before = buf.clone()
    for bad in (0, 8193):
        with pytest.raises(RuntimeError):
            _lib.call("sam6d_draw_choice", n.data_ptr(), len(counts), bad, 11, 2, buf.data_ptr() + 4 * G, stream)
        with pytest.raises(ValueError):
            inputs.draw_choice(n, bad, 11)
    with pytest.raises(RuntimeError):
        _lib.call("sam6d_draw_choice", n.data_ptr(), -1, ns, 11, 2, buf.data_ptr() + 4 * G, stream)
    with pytest.raises(RuntimeError):
        _lib.call("sam6d_draw_choice", None, 2, ns, 11, 2, buf.data_ptr() + 4 * G, stream)
    with pytest.raises(RuntimeError):
        inputs.draw_choice(n.cpu(), ns, 11)
    with pytest.raises(RuntimeError):
        inputs.draw_choice(n.float(), ns, 11)
    assert torch.equal(buf, before)  # a refused call writes nothing
    assert inputs.draw_choice(n[:0], ns, 11).shape == (0, ns)


# ------------------------------------------------------------------------------------------------------- assembled inputs
CFG = dict(img_size=224, n_sample_observed_point=64, n_sample_template_point=5000, rgb_mask_flag=True)
N_DET = 12


def _scene(seed):
    """seeded discs with holes and zero-depth pixels; detection 3 has 30 pixels (skipped), detection 5 a 7 x 7 mask (<= 64 points: the
    draw with replacement)"""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (0.6 + 0.0004 * xx + 0.05 * g.random((H, W))).astype(np.float32)
    depth[g.random((H, W)) < 0.05] = 0
    masks = np.zeros((N_DET, H, W), np.uint8)
    for i in range(N_DET):
        cy, cx, r = g.integers(0, H), g.integers(0, W), g.integers(30, 160)
        m = ((xx - cx) ** 2 + (yy - cy) ** 2) < r * r
        m &= g.random((H, W)) > 0.15
        masks[i] = m * g.integers(1, 256)
    masks[3] = 0
    masks[3, 100:105, 100:106] = 1
    masks[5] = 0
    masks[5, 200:207, 300:307] = 1
    depth[200:207, 300:307] = 0.7
    scores = g.random(N_DET)
    model = ((g.random((1024, 3)) - 0.5) * 0.12).astype(np.float32)
    return img, depth, masks, scores, model


def test_test_data_with_device_choice(dev):
    img, depth, masks, scores, model = _scene(31)
    args = (torch.from_numpy(img).to(dev), torch.from_numpy(depth).to(dev), K, torch.from_numpy(masks).to(dev), scores, model, CFG)
    rng = inputs.DeviceChoice(7)
    got, kept = inputs.test_data(*args, rng=rng)
    assert rng.row == N_DET
    np.random.seed(2)
    base, bkept = inputs.test_data(*args)
    assert kept == bkept and 3 not in kept and 5 in kept and len(kept) >= 8
    for k in ("rgb", "score", "model", "K"):
        assert torch.equal(got[k], base[k]), k
    geom = inputs.proposal_geometry(args[3], args[1], K, np.max(np.linalg.norm(model, axis=1)))
    n_keep = geom["n_keep"].cpu().numpy()
    assert 4 <= n_keep[5] <= 64 < n_keep[kept[0]]
    idx = torch.tensor(kept, device=dev)
    for row0, data in ((0, got), (N_DET, inputs.test_data(*args, rng=rng)[0])):  # the second call with the same object: rows N .. 2 N - 1
        sel = torch.from_numpy(R.draw(n_keep, 64, 7, row0=row0)).to(dev)
        pts, rc = inputs.proposal_choose(geom, sel, 224)
        assert data["pts"].shape == (len(kept), 64, 3) and data["rgb_choose"].dtype == torch.int64
        assert torch.equal(data["pts"], pts[idx]) and torch.equal(data["rgb_choose"], rc[idx]), row0
    assert rng.row == 2 * N_DET
    assert not torch.equal(got["pts"], base["pts"])  # not numpy's stream


def test_templates_with_device_choice(dev):
    g = np.random.default_rng(9)
    T, h, w = 3, 120, 160
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = g.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    masks = np.zeros((T, h, w), np.uint8)
    for t in range(T):
        r = 20 if t == 1 else g.integers(45, 60)  # template 1: fewer than 5000 mask pixels
        cy, cx = g.integers(40, h - 40), g.integers(50, w - 50)
        masks[t] = np.where(((xx - cx) ** 2 + (yy - cy) ** 2) < r * r, 255, np.where(g.random((h, w)) < 0.02, 128, 0))
    xyz = ((g.random((T, h, w, 3)) - 0.5) * 200.0).astype(np.float32)
    d = [torch.from_numpy(a).to(dev) for a in (imgs, masks, xyz)]
    rng = inputs.DeviceChoice(7)
    rng.row = 40
    got = inputs.templates(*d, CFG, rng=rng)
    assert rng.row == 43
    geom = inputs.template_geometry(d[1], d[2])
    n_valid = geom["n_valid"].cpu().numpy()
    assert n_valid[1] < 5000 < n_valid[0]
    sel = torch.from_numpy(R.draw(n_valid, 5000, 7, row0=40)).to(dev)
    want = inputs.template_inputs(*d, sel, 224, True)  # rgb, rgb_choose, xyz
    for a, b, what in zip(got, (want[0], want[2], want[1]), ("rgb", "pts", "choose")):
        assert len(a) == T
        for t in range(T):
            assert a[t].dtype == b.dtype and torch.equal(a[t], b[t:t + 1]), (what, t)
    d[1][2] = 0  # a template without a mask pixel is refused before anything is drawn
    with pytest.raises(RuntimeError):
        inputs.templates(*d, CFG, rng=rng)
    assert rng.row == 43
