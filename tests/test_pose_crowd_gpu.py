"""The pose check and the refinement on the device (csrc/verify.hip, csrc/refine.hip, csrc/verify_raster.h through sam6d_hip.verify,
sam6d_hip.refine and the C entries) on the scenes of tests/pose_crowd_ref.py: N = 1024 poses with windows of a few words (many poses
to a wave, the LDS exit and the direct-atomic exit of the per-pose loop in one wave, runs of empty windows under the bisection, every
pose-indexed kernel past its first block), seventy poses that tie, all five status codes of the solve in one call, and one window at
the 2048 x 2048 limit.  Every comparison is bit for bit against tests/verify_ref.py and tests/refine_ref.py;
tests/test_pose_crowd_host.py asserts that the scenes hold what is said here."""
import math

import numpy as np
import pytest
import torch

from tests import pose_crowd_ref as PC
from tests import refine_ref as RF
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from tests.test_refine_gpu import Step, _same_step, _same_whole
from tests.test_verify_gpu import _mesh, _run, _same, _t
from sam6d_hip import _lib, refine, verify
from sam6d_hip import visualize as V

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _check(dev, s, masks, wave_area=0):
    return _run(dev, s.v, s.f, s.view, s.obs, masks, tau=PC.TAU, intr=s.intr, near=PC.NEAR, wave_area=wave_area)


def _same_check(dev, got, want, with_masks):
    _same(dev, got, want)
    if with_masks:
        assert torch.equal(got.mask_iou, _t(VR.mask_iou(want[1]), dev))
    else:
        assert got.mask_iou is None


# ------------------------------------------------------------------------------------------------------------ 1. the check on a crowd
@pytest.mark.parametrize("with_masks", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("name", ["tiny", "mid", "mixed"])
def test_crowd_verify(dev, name, with_masks):
    s = PC.scene(name)
    masks = s.masks if with_masks else None
    want = PC.verify_want(name, with_masks)
    got = _check(dev, s, masks)
    _same_check(dev, got, want, with_masks)
    if name == "tiny":  # every face by the wave; every face by its lane
        for wave_area in (1, 2 ** 31 - 1):
            _same_check(dev, _check(dev, s, masks, wave_area), want, with_masks)
    # a pose alone: its counts and its box do not depend on the company
    has = np.nonzero(VR.areas(want[0], s.size) > 0)[0]
    some = np.random.default_rng(6).choice(has[1:-1], 6, replace=False)
    for n in [has[0], has[-1]] + sorted(some.tolist()):
        alone = _run(dev, s.v, s.f, s.view[n:n + 1], s.obs, None if masks is None else masks[n:n + 1], tau=PC.TAU, intr=s.intr, near=PC.NEAR)
        assert torch.equal(alone.counts[0], got.counts[n]) and torch.equal(alone.boxes[0], got.boxes[n]), n


# ------------------------------------------------------------------------------------------------------------ 2. the C entry, guarded
def test_crowd_verify_entry_guards(dev):
    """sam6d_pose_windows and sam6d_pose_verify on `tiny` with 64 guard elements round the workspace and every output"""
    s = PC.scene("tiny")
    H, W = s.size
    N, G = len(s.view), 64
    wbox, wcounts, wids, wdepth = PC.verify_want("tiny", True)
    d = dict(v=_t(s.v, dev), f=_t(s.f, dev), view=_t(s.view, dev), obs=_t(s.obs, dev), masks=_t(s.masks, dev))
    sizes = dict(box=(N * 4, torch.int32), dropped=(N, torch.int32), counts=(N * 8, torch.int32), ids=(H * W, torch.int32),
                 depth=(H * W, torch.float32))
    bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
    offset = np.concatenate([[0], np.cumsum(VR.areas(wbox, s.size))]).astype(np.int64)
    assert offset.shape == (N + 1,)
    total = int(offset[-1])
    d_offset = _t(offset, dev)
    need = int(_lib.load().sam6d_pose_verify_workspace_bytes(total, H, W))
    assert need == 8 * (total + H * W)
    ws = torch.full((need // 8 + 2 * G,), 77, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("sam6d_pose_windows", d["v"].data_ptr(), len(s.v), d["f"].data_ptr(), len(s.f), d["view"].data_ptr(), N, *s.intr, H, W, PC.NEAR,
              ptr["box"], ptr["dropped"], stream)
    _lib.call("sam6d_pose_verify", d["v"].data_ptr(), len(s.v), d["f"].data_ptr(), len(s.f), d["view"].data_ptr(), N, *s.intr, H, W, PC.NEAR, 0,
              ptr["box"], d_offset.data_ptr(), total, d["obs"].data_ptr(), d["masks"].data_ptr(), PC.TAU, ptr["counts"], ptr["ids"], ptr["depth"],
              ws.data_ptr() + 8 * G, need, stream)
    want = dict(box=wbox, dropped=wcounts[:, 7], counts=wcounts, ids=wids, depth=wdepth)
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 77).all() and (h[-G:] == 77).all(), k
        assert np.array_equal(h[G:-G].view(np.uint32), np.ascontiguousarray(want[k]).reshape(-1).view(np.uint32)), k
    hw = ws.cpu().numpy()
    assert (hw[:G] == 77).all() and (hw[-G:] == 77).all()


# ------------------------------------------------------------------------------------------------------------ 3. seventy poses that tie
@pytest.mark.parametrize("with_masks", [False, True], ids=["plain", "masks"])
def test_duplicates(dev, with_masks):
    s = PC.duplicates()
    want = PC.verify_want("duplicates", with_masks)
    got = _check(dev, s, s.masks if with_masks else None)
    _same_check(dev, got, want, with_masks)
    ids, counts = got.ids.cpu().numpy(), got.counts.cpu().numpy()
    assert not ((ids >= 1) & (ids <= 69)).any() and (ids == 0).any() and (ids == 70).any()
    cols = [0, 1, 2, 3, 4, 7]  # n_mask and n_inter are each mask's own
    assert (counts[:70][:, cols] == counts[0, cols]).all()


# ------------------------------------------------------------------------------------------------------------ 4. one step of a crowd
def _unstepped_keep_their_bits(s, what):
    """for every pose whose status is not 0, the state holds the bits it held before the call"""
    state, stats = s.host("state")[0].view(np.uint64).reshape(-1, 12), s.host("stats")[0].reshape(-1, 4)
    kept = (state == s.state0.view(np.uint64)).all(axis=1)
    assert kept[stats[:, 1] != 0].all(), (what, np.nonzero(~kept & (stats[:, 1] != 0))[0])
    return stats[:, 1]


@pytest.mark.parametrize("max_step", [math.inf, 0.05], ids=["inf", "0.05"])
def test_crowd_refine_step(dev, max_step):
    c = PC.scene("tiny")
    R, t, box = PC.crowd_starts("tiny", PC.CROWD_MARGIN)
    s = Step(dev, c.v, c.f, R, t, box, c.obs, c.masks, size=c.size, intr=c.intr)
    for with_masks in (False, True):
        what = "max_step %g, masks %s" % (max_step, with_masks)
        s.reset()
        s(inv_unit=RF.inv_unit_of(c.v), damping=PC.DAMPING, min_pairs=PC.CROWD_MIN_PAIRS, max_step=max_step, masks=with_masks)
        _same_step(s, PC.crowd_step_want("tiny", max_step, with_masks), what)
        codes = _unstepped_keep_their_bits(s, what)
        assert set(codes.tolist()) == ({0, 1, 4} if max_step == math.inf else {1, 3, 4}), what


# ------------------------------------------------------------------------------------------------------------ 5. singular by construction
def test_frontal_quads_are_singular(dev):
    q = PC.frontal_quads()
    s = Step(dev, q.v, q.f, q.R, q.t, q.box, q.obs, None, size=q.size, intr=q.intr)
    for damping in (0.0, PC.DAMPING):
        what = "damping %g" % damping
        s.reset()
        s(gate=PC.QUADS_GATE, inv_unit=RF.inv_unit_of(q.v), damping=damping, min_pairs=PC.QUADS_MIN_PAIRS)
        _same_step(s, PC.quads_step_want(damping), what)
        codes = _unstepped_keep_their_bits(s, what)
        assert set(codes.tolist()) == {1, 2, 4}, what  # in one call
        assert np.array_equal(s.host("state")[0].view(np.uint64), s.state0.view(np.uint64).reshape(-1)), what
        assert not s.host("acc")[0].reshape(-1, 32)[:, RF.WORDS.index((2, 2))].any(), what


# ------------------------------------------------------------------------------------------------------------ 6. the whole call
def test_crowd_refine_poses(dev):
    c = PC.scene("mid")
    R, t, _ = PC.crowd_starts("mid", PC.MID_MARGIN)
    got = refine.refine_poses((_t(c.v, dev), _t(c.f, dev)), _t(R, dev), _t(t, dev), c.intr, _t(c.obs, dev), iters=PC.MID_ITERS, gate=RF.GATE,
                              margin=PC.MID_MARGIN, min_pairs=PC.CROWD_MIN_PAIRS)
    _same_whole(dev, got, PC.mid_refine_want())


# ------------------------------------------------------------------------------------------------------------ 7. the size limit
def test_limit_size(dev):
    """one window of 2^22 words: 4096 workgroups at one pose's counters and sums; 32 MiB of z-buffer and 32 MiB of composite"""
    m = PC.limit()
    assert all(np.array_equal(a, b) for a, b in zip(PC.QUAD, _mesh("quad")))
    got = _check(dev, m, None)
    _same_check(dev, got, PC.verify_want("limit", False), False)
    del got
    s = Step(dev, m.v, m.f, m.view[:, :, :3], m.view[:, :, 3], m.box, m.obs, None, size=m.size, intr=m.intr)
    assert s.total == 2 ** 22
    s(inv_unit=RF.inv_unit_of(m.v), damping=PC.DAMPING, min_pairs=PC.LIMIT_MIN_PAIRS)
    _same_step(s, PC.limit_step_want(), "limit")
    assert s.host("stats")[0].tolist()[:2] == [2 ** 22, 0]
    del s
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ 8. the picture
def test_overlay_1024_colours(dev):
    g = np.random.default_rng(9)
    H, W = PC.TINY_SIZE
    ids = PC.verify_want("tiny", True)[2].copy()
    assert np.unique(ids[ids >= 0]).size >= 100
    ids[3, 5], ids[20, 30], ids[44, 60], ids[10, 11] = -1, 1024, 2 ** 31 - 1, 1023
    colors = g.integers(0, 256, (1024, 3), dtype=np.uint8)
    rgb = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    got = V.overlay_instances(_t(rgb, dev), _t(ids, dev), colors, alpha=128)
    want = VR.overlay_instances(rgb, ids, colors, 128)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, 2 * W, 3) and torch.equal(got, _t(want, dev))
    assert np.array_equal(want[20, W + 30], rgb[20, 30]) and np.array_equal(want[44, W + 60], rgb[44, 60]) and np.array_equal(want[10, W + 11], colors[1023])


# ------------------------------------------------------------------------------------------------------------ 9. one pose too many
def test_wrappers_refuse_1025_poses(dev, monkeypatch):
    """ValueError from the wrappers' own check: no entry of the library is called"""
    c = PC.scene("tiny")
    view = np.concatenate([c.view, c.view[:1]])
    mesh, R, t, obs = (_t(c.v, dev), _t(c.f, dev)), _t(view[:, :, :3], dev), _t(view[:, :, 3], dev), _t(c.obs, dev)

    def called(name, *args):
        raise AssertionError("%s was called" % name)

    monkeypatch.setattr(_lib, "call", called)
    with pytest.raises(ValueError, match="N = 1025"):
        verify.render_compare(mesh, R, t, c.intr, obs)
    with pytest.raises(ValueError, match="N = 1025"):
        refine.refine_poses(mesh, R, t, c.intr, obs)
