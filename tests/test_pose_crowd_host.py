"""The scenes of tests/pose_crowd_ref.py are what they are built to be.  No GPU: every condition here is computed from the numpy
restatements' own output (tests/verify_ref.py, tests/refine_ref.py) and is a condition on the scene, not a measurement -- a seed that
misses one is changed, never the condition.  This is what keeps tests/test_pose_crowd_gpu.py from comparing the kernels where their
control flow is the one the older scenes already walk: many poses to a wave, many windows to a workgroup, runs of empty windows, every
status code in every block of the solve kernel, and the sums of a whole 2048 x 2048 window."""
import math

import numpy as np

from tests import pose_crowd_ref as PC
from tests import refine_ref as RF
from tests import verify_ref as VR

F64 = np.float64


def _layout(box, size):
    """offset (N+1), area (N) and the first words of the windows that are not empty"""
    area = VR.areas(box, size)
    offset = np.concatenate([[0], np.cumsum(area)]).astype(np.int64)
    return offset, area, offset[:-1][area > 0]


def _most_in_span(start, span):
    """the largest number of windows that start inside one aligned span of `span` words"""
    return int(np.bincount(start // span).max())


def _longest_empty_run(area):
    best = run = 0
    for a in area:
        run = run + 1 if a == 0 else 0
        best = max(best, run)
    return best


def _status_counts(stats):
    return [int((stats[:, 1] == k).sum()) for k in range(5)]


# ------------------------------------------------------------------------------------------------------------ tiny: the pose check
def test_tiny_windows_crowd_the_waves():
    s = PC.scene("tiny")
    box, counts, ids, depth = PC.verify_want("tiny", True)
    offset, area, start = _layout(box, s.size)
    in_wave, in_group, empty_run, total = _most_in_span(start, 64), _most_in_span(start, 1024), _longest_empty_run(area), int(offset[-1])
    distinct = int(np.unique(ids[ids >= 0]).size)
    cover = np.zeros(s.size, np.int64)
    for n, setup in enumerate(VR._setups(s.v, s.f, s.view, s.intr, s.size, PC.NEAR)):
        x0, y0, bw, bh = VR.clamp_box(box[n], s.size)
        cover[y0:y0 + bh, x0:x0 + bw] += VR.window_zbuffer(setup, (x0, y0, bw, bh)) != VR.EMPTY
    print("tiny: %d windows start in one 64-word span, %d in one 1024-word span, %d empty windows in a row, total %d words, %d ids in the "
          "composite, a pixel under %d poses" % (in_wave, in_group, empty_run, total, distinct, cover.max()))
    assert len(s.view) == 1024 and s.size == (45, 61)
    assert in_wave >= 8 and in_group >= 64 and empty_run >= 3
    assert total > 2 * 1024  # at least three workgroups
    assert distinct >= 100 and cover.max() >= 3
    assert cover.sum() == counts[:, 0].sum() and ((cover > 0) == (ids >= 0)).all()
    # every class is counted, somewhere behind the first workgroup too, and the masks meet the renders
    assert (counts[:, 1:5].sum(axis=0) > 0).all() and (counts[:, 1:5].sum(axis=1) == counts[:, 0]).all()
    assert counts[offset[:-1] >= 1024, 0].sum() > 0 and counts[:, 6].sum() > 0 and (counts[:, 5] > 0).all()
    assert not PC.verify_want("tiny", False)[1][:, 5:7].any()


def test_mid_and_mixed_windows():
    for name, N in (("mid", 300), ("mixed", 64)):
        s = PC.scene(name)
        box, counts, ids, _ = PC.verify_want(name, True)
        offset, area, start = _layout(box, s.size)
        some = area[area > 0]
        print("%s: windows of %d .. %d words, total %d, %d without a window, %d ids in the composite"
              % (name, some.min(), some.max(), offset[-1], (area == 0).sum(), np.unique(ids[ids >= 0]).size))
        assert len(s.view) == N and s.size == RF.BIG and (counts[:, 1:5].sum(axis=0) > 0).all()
        if name == "mid":
            assert (area == 0).any() and _most_in_span(start, 1024) >= 4 and _most_in_span(start, 64) >= 2
        else:  # both sides of a workgroup's 1024 words, and of a wave's 64
            assert some.min() < 100 and some.max() > 1024 and (some < 1024).sum() >= 10 and (some > 1024).sum() >= 3


# ------------------------------------------------------------------------------------------------------------ tiny: the refinement
def test_tiny_steps_end_in_every_way():
    s = PC.scene("tiny")
    R, t, box = PC.crowd_starts("tiny", PC.CROWD_MARGIN)
    offset, area, start = _layout(box, s.size)
    state0 = PC.state_of(R, t)
    free = _status_counts(PC.crowd_step_want("tiny", math.inf, False)[2])
    bound = _status_counts(PC.crowd_step_want("tiny", 0.05, False)[2])
    print("tiny refine: statuses 0 .. 4 without a step bound %s, with max_step 0.05 %s; %d windows start in one 64-word span, total %d"
          % (free, bound, _most_in_span(start, 64), offset[-1]))
    assert free[0] >= 10 and free[1] >= 10 and free[4] >= 10 and free[2] == free[3] == 0
    assert bound[3] >= 10 and bound[1] == free[1] and bound[4] == free[4]
    assert _most_in_span(start, 64) >= 4 and offset[-1] > 2 * 1024
    for max_step in (math.inf, 0.05):
        for with_masks in (False, True):
            state, acc, stats = PC.crowd_step_want("tiny", max_step, with_masks)
            codes = stats[:, 1]
            assert all(np.unique(codes[b:b + 64]).size >= 2 for b in range(0, 1024, 64)), (max_step, with_masks)
            kept = state.view(np.uint64) == state0.view(np.uint64)
            assert kept[codes != 0].all() and not kept[codes == 0].all(axis=1).any()
            assert (acc[:, 28] == stats[:, 0]).all() and (acc[:, 29:] == 0).all()
    masked = PC.crowd_step_want("tiny", math.inf, True)[2]
    assert 0 < masked[:, 0].sum() < PC.crowd_step_want("tiny", math.inf, False)[2][:, 0].sum()


def test_mid_refinement_ends_in_several_ways():
    want = PC.mid_refine_want()
    codes = [int((want["status"] == k).sum()) for k in range(5)]
    print("mid refine_poses: statuses 0 .. 4 after the last iteration %s" % codes)
    assert codes[0] >= 10 and codes[1] >= 10 and codes[4] >= 1
    assert all(np.unique(want["status"][b:b + 64]).size >= 2 for b in range(0, 300, 64))  # five blocks of the solve kernel


# ------------------------------------------------------------------------------------------------------------ duplicates
def test_duplicates_tie():
    s = PC.duplicates()
    box, counts, ids, _ = PC.verify_want("duplicates", True)
    offset, area, _ = _layout(box, s.size)
    assert len(s.view) == 71 and (area[:70] == area[0]).all() and 64 < area[0] < 1024
    assert (ids == 0).sum() > 100 and not ((ids >= 1) & (ids <= 69)).any() and (ids == 70).sum() > 100
    assert (counts[:70, [0, 1, 2, 3, 4, 7]] == counts[0, [0, 1, 2, 3, 4, 7]]).all() and counts[0, 0] > (ids == 0).sum()
    assert (PC.verify_want("duplicates", False)[1][:70] == PC.verify_want("duplicates", False)[1][0]).all()


# ------------------------------------------------------------------------------------------------------------ frontal quads
def test_frontal_quads_are_singular_by_construction():
    s = PC.frontal_quads()
    assert len(s.R) == 130 and (s.R == np.eye(3, dtype=np.float32)).all() and (s.t[:, 2] >= 1.2).all() and (s.obs > 0).all()
    state0 = PC.state_of(s.R, s.t)
    word = RF.WORDS.index((2, 2))
    for damping in (0.0, PC.DAMPING):
        state, acc, stats = PC.quads_step_want(damping)
        codes = _status_counts(stats)
        print("frontal quads, damping %g: statuses 0 .. 4 %s" % (damping, codes))
        assert codes[2] >= 10 and codes[4] >= 1 and codes[1] >= 1 and codes[0] == codes[3] == 0
        assert (acc[:, word] == 0).all() and (acc[:, [RF.WORDS.index(ij) for ij in ((0, 2), (1, 2), (2, 3), (2, 4), (2, 5), (2, 6))]] == 0).all()
        assert (state.view(np.uint64) == state0.view(np.uint64)).all()
        assert (acc[stats[:, 1] == 2, 0] > 0).all() and (acc[stats[:, 1] == 2, 7] > 0).all()  # the first two pivots are positive
        assert ((stats[:, 1] == 1) & (stats[:, 0] > 0)).any()  # clipped by the border, not merely unseen


# ------------------------------------------------------------------------------------------------------------ the size limit
def test_limit_fills_the_largest_window():
    s = PC.limit()
    box, counts, ids, depth = PC.verify_want("limit", False)
    assert box.tolist() == [[0, 0, 2047, 2047]] == s.box.tolist() and counts[0, 0] == 2 ** 22 and (ids == 0).all()
    assert counts[0, 1:5].sum() == counts[0, 0] and (counts[0, 1:4] > 2 ** 20).all() and counts[0, 4] == 0
    state, acc, stats = PC.limit_step_want()
    bits = int(np.abs(acc).max()).bit_length()
    print("limit: n_render %d, counts %s, pairs %d, status %d, the largest sum has %d bits" % (counts[0, 0], counts[0].tolist(), stats[0, 0],
                                                                                              stats[0, 1], bits))
    assert stats[0, 0] == 2 ** 22 == acc[0, 28] and stats[0, 1] == 0 and np.abs(acc).max() >= 2 ** 50
    assert not (state.view(np.uint64) == PC.state_of(s.view[:, :, :3], s.view[:, :, 3]).view(np.uint64)).all()
