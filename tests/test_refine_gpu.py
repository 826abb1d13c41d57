"""The pose refinement on the device (sam6d_hip.refine over csrc/refine.hip) against its numpy restatement (tests/refine_ref.py).
Every comparison is bit for bit: the integer sums, the statistics, and the float64 state after the solve."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import refine_ref as RF
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, refine, verify

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MESHES = {"a": RF.mesh_a, "b": RF.mesh_b}
DAMPING, MIN_PAIRS = 1e-6, 32


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _five(mesh):
    """the mesh at VR.five_poses, each perturbed; the observed depth is the render of the true poses 0, 1 and 2, the earlier pose
    where two cover a pixel; masks of about 60 % ones.  -> v, f, R, t, box (margin 4), depth, masks, inv_unit"""
    v, f = MESHES[mesh]()
    depth = np.zeros(VR.SIZE, F32)
    for M in VR.five_poses()[:3]:
        d = VR.render_depth(v, f, M, VR.INTR, VR.SIZE)[1]
        depth = np.where(depth > 0, depth, d)
    R, t = RF.five_starts()
    view = np.concatenate([R, t[:, :, None]], axis=2)
    box = RF.grow(VR.windows(v, f, view, VR.INTR, VR.SIZE)[0], 4, VR.SIZE)
    masks = (np.random.default_rng(5).random((5,) + VR.SIZE) < 0.6).astype(np.uint8) * 3
    return v, f, R, t, box, depth, masks, RF.inv_unit_of(v)


@functools.lru_cache(maxsize=None)
def _five_want(mesh, with_masks):
    v, f, R, t, box, depth, masks, iu = _five(mesh)
    state = np.concatenate([R.reshape(5, 9), t], axis=1).astype(F64)
    return RF.step(v, f, state, 1.0, VR.INTR, VR.SIZE, 1e-3, box, depth, masks if with_masks else None, RF.GATE, iu, DAMPING, MIN_PAIRS, math.inf)


class Step:
    """sam6d_pose_refine_step on buffers with G guard elements of 77 on either side of the workspace and of every output"""
    G = 64

    def __init__(self, dev, v, f, R, t, box, depth, masks, size=VR.SIZE, intr=VR.INTR):
        self.dev, self.size, self.intr = dev, size, intr
        self.N = N = len(R)
        self.d = dict(v=_t(v, dev), f=_t(f, dev), box=_t(np.asarray(box, np.int32), dev), depth=_t(depth, dev), masks=_t(masks, dev))
        offset = np.concatenate([[0], np.cumsum(VR.areas(box, size))]).astype(np.int64)
        self.total = int(offset[-1])
        self.d["offset"] = _t(offset, dev)
        self.need = int(_lib.load().sam6d_pose_refine_workspace_bytes(self.total, N))
        assert self.need == 8 * self.total + 80 * N
        G = self.G
        sizes = dict(state=(N * 12, torch.float64), acc=(N * 32, torch.int64), stats=(N * 4, torch.int32), ws=(self.need // 8, torch.int64))
        self.bufs = {k: torch.full((n + 2 * G,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
        self.ptr = {k: b.data_ptr() + G * b.element_size() for k, b in self.bufs.items()}
        self.state0 = np.concatenate([np.asarray(R, F32).reshape(N, 9), np.asarray(t, F32)], axis=1).astype(F64)
        self.reset()

    def reset(self):
        self.bufs["state"][self.G:-self.G] = _t(self.state0.reshape(-1), self.dev)

    def __call__(self, wave_area=0, gate=RF.GATE, inv_unit=1.0, damping=DAMPING, min_pairs=MIN_PAIRS, max_step=math.inf, masks=True, **kw):
        d, p = self.d, self.ptr
        a = dict(vert=d["v"].data_ptr(), V=int(d["v"].shape[0]), faces=d["f"].data_ptr(), F=int(d["f"].shape[0]), scale=1.0, N=self.N,
                 H=self.size[0], W=self.size[1], near=1e-3, box=d["box"].data_ptr(), offset=d["offset"].data_ptr(), total=self.total,
                 depth=d["depth"].data_ptr(), masks=d["masks"].data_ptr() if masks and d["masks"] is not None else None, state=p["state"],
                 acc=p["acc"], stats=p["stats"], ws=p["ws"], ws_bytes=self.need)
        a.update(kw)
        _lib.call("sam6d_pose_refine_step", a["vert"], a["V"], a["faces"], a["F"], a["scale"], a["N"], *self.intr, a["H"], a["W"], a["near"], wave_area,
                  a["box"], a["offset"], a["total"], a["depth"], a["masks"], gate, float(inv_unit), damping, min_pairs, max_step, a["state"], a["acc"],
                  a["stats"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)

    def host(self, k):
        """(the buffer without its guards, the guards are whole)"""
        h = self.bufs[k].cpu().numpy()
        return h[self.G:-self.G], bool((h[:self.G] == 77).all() and (h[-self.G:] == 77).all())


def _same_step(s, want, what):
    state, acc, stats = want
    for k, w in (("acc", acc), ("stats", stats)):
        h, whole = s.host(k)
        assert whole, (what, k)
        assert np.array_equal(h, np.asarray(w).reshape(-1)), (what, k, h.reshape(np.asarray(w).shape), w)
    h, whole = s.host("state")
    assert whole and s.host("ws")[1], what
    same = h.view(np.uint64) == _bits(state).reshape(-1)
    assert same.all(), (what, "state", float(np.abs(h - state.reshape(-1)).max()), int((~same).sum()))


# ------------------------------------------------------------------------------------------------------------ the step entry
@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_step_entry(dev, mesh, with_masks):
    """five poses at once (inside; straddling the right and bottom borders; through the camera plane; off-screen; behind the camera),
    every face by the wave, every face by its lane and the default: sums, statistics and the float64 state, bit for bit"""
    v, f, R, t, box, depth, masks, iu = _five(mesh)
    want = _five_want(mesh, with_masks)
    stats = want[2]
    assert stats[:, 1].tolist()[3:] == [4, 4] and stats[0, 1] == 0 and stats[0, 0] > 100 and (stats[:3, 0] > 0).all(), stats
    assert box[1, 2:].tolist() == [63, 47] and len(f) == (8 if mesh == "a" else 320)
    s = Step(dev, v, f, R, t, box, depth, masks)
    for wave_area in (1, 2 ** 31 - 1, 0):
        s.reset()
        s(wave_area=wave_area, inv_unit=iu, masks=with_masks)
        _same_step(s, want, "wave_area %d" % wave_area)


# ------------------------------------------------------------------------------------------------------------ the whole call
@functools.lru_cache(maxsize=None)
def _whole_scene():
    v, f = RF.mesh_a()
    depth = VR.render_depth(v, f, RF.TRUE, VR.INTR, VR.SIZE)[1]
    off = VR.pose((10.0, 0.0, 4.0))
    Rs, ts = zip(RF.start("near"), RF.start("far"), (off[:, :3], off[:, 3]))
    return v, f, np.stack(Rs), np.stack(ts), depth


def _same_whole(dev, got, want):
    for k, dt in (("R", torch.float32), ("t", torch.float32), ("n_pairs", torch.int32), ("status", torch.int32), ("history", torch.float32),
                  ("rms", torch.float32), ("boxes", torch.int32)):
        g = getattr(got, k)
        assert g.dtype == dt and g.is_cuda, k
        assert np.array_equal(g.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), (k, g.cpu().numpy(), want[k])


@pytest.mark.parametrize("margin", [0, 8, 100])
def test_refine_poses(dev, margin):
    """five iterations, three poses (the two starts and one off-screen), window margins 0, 8 and the whole image: R, t, n_pairs,
    status, history and boxes equal the restatement's; the refined poses are the true pose to 1e-3"""
    v, f, R, t, depth = _whole_scene()
    want = RF.refine(v, f, R, t, VR.INTR, VR.SIZE, depth, iters=5, gate=RF.GATE, margin=margin)
    got = refine.refine_poses((_t(v, dev), _t(f, dev)), _t(R, dev), _t(t, dev), VR.INTR, _t(depth, dev), iters=5, gate=RF.GATE, margin=margin)
    _same_whole(dev, got, want)
    assert want["status"].tolist() == [0, 0, 4] and want["boxes"][2].tolist() == [0, 0, -1, -1]
    if margin == 100:
        assert want["boxes"][:2].tolist() == [[0, 0, 63, 47]] * 2
    for n in range(2):
        assert np.abs(want["t"][n] - RF.TRUE[:, 3]).max() <= 1e-3 and np.linalg.norm(want["R"][n] - RF.TRUE[:, :3]) <= 1e-3, n
    assert np.array_equal(want["R"][2], R[2]) and np.array_equal(want["t"][2], t[2])


def test_refine_poses_takes_render_compares_forms(dev):
    """a mesh dict of numpy arrays, K as a matrix, bool masks, a millimetre model under scale 0.001"""
    v, f, R, t, depth = _whole_scene()
    mm = (v * F32(1000.0)).astype(F32)
    K = np.array([[VR.INTR[0], 0, VR.INTR[2]], [0, VR.INTR[1], VR.INTR[3]], [0, 0, 1]])
    masks = np.zeros((3,) + VR.SIZE, bool)
    masks[:, :, 8:] = True
    want = RF.refine(mm, f, R, t, VR.INTR, VR.SIZE, depth, masks=masks, iters=3, gate=RF.GATE, scale=0.001, max_step=0.5, min_pairs=50)
    got = refine.refine_poses(dict(vertices=mm, faces=f), _t(R, dev), _t(t, dev), K, _t(depth, dev), masks=_t(masks, dev), iters=3, gate=RF.GATE,
                              scale=0.001, max_step=0.5, min_pairs=50)
    _same_whole(dev, got, want)
    assert want["status"].tolist() == [0, 0, 4] and (want["n_pairs"][:2] > 100).all()


# ------------------------------------------------------------------------------------------------------------ windows and guards
@pytest.mark.parametrize("margin", [0, 100])
def test_step_stays_inside_its_windows(dev, margin):
    """the tight windows and the whole image as every window: the step equals the restatement, and the guard words round the
    workspace (whose z-buffer is the windows, laid end to end) and round every output are untouched"""
    v, f, R, t, _, depth, masks, iu = _five("a")
    box = RF.grow(VR.windows(v, f, np.concatenate([R, t[:, :, None]], axis=2), VR.INTR, VR.SIZE)[0], margin, VR.SIZE)
    assert box[3].tolist() == [0, 0, -1, -1] and (margin == 0 or box[:3].tolist() == [[0, 0, 63, 47]] * 3)
    state = np.concatenate([R.reshape(5, 9), t], axis=1).astype(F64)
    want = RF.step(v, f, state, 1.0, VR.INTR, VR.SIZE, 1e-3, box, depth, masks, RF.GATE, iu, DAMPING, MIN_PAIRS, math.inf)
    s = Step(dev, v, f, R, t, box, depth, masks)
    s(inv_unit=iu)
    _same_step(s, want, "margin %d" % margin)


def test_wild_boxes_and_offsets_stay_inside(dev):
    """boxes and offsets the host never sees: nothing outside the buffers is touched, whatever they hold"""
    v, f, R, t, box, depth, masks, iu = _five("b")
    s = Step(dev, v, f, R, t, box, depth, masks)
    wild = _t(np.array([[-5, -7, 5000, 4000], [60, 40, 70, 50], [10, 10, 5, 5], [0, 0, -1, -1], [0, 0, 63, 47]], np.int32), dev)
    s(inv_unit=iu, box=wild.data_ptr())
    s(inv_unit=iu, offset=_t(np.array([0, s.total, -40, 1 << 40, 7, s.total], np.int64), dev).data_ptr())
    for k in s.bufs:
        assert s.host(k)[1], k


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    v, f, R, t, box, depth, masks, iu = _five("a")
    s = Step(dev, v, f, R, t, box, depth, masks)
    before = {k: b.clone() for k, b in s.bufs.items()}
    cases = [(dict(vert=None), "null"), (dict(faces=None), "null"), (dict(box=None), "null"), (dict(offset=None), "null"), (dict(depth=None), "null"),
             (dict(state=None), "null"), (dict(acc=None), "null"), (dict(stats=None), "null"), (dict(ws=None), "null"), (dict(N=1025), "N = 1025"),
             (dict(N=0), "N = 0"), (dict(H=2049), "H x W"), (dict(F=0), "F = 0"), (dict(near=0.0), "near"), (dict(gate=-1.0), "gate"),
             (dict(gate=float("nan")), "gate"), (dict(gate=float("inf")), "gate"), (dict(inv_unit=0.0), "inv_unit"),
             (dict(inv_unit=float("inf")), "inv_unit"), (dict(damping=-1.0), "damping"), (dict(damping=float("nan")), "damping"),
             (dict(min_pairs=0), "min_pairs"), (dict(max_step=0.0), "max_step"), (dict(max_step=float("nan")), "max_step"), (dict(scale=0.0), "scale"),
             (dict(wave_area=-1), "wave_area"), (dict(total=-1), "total"), (dict(total=5 * 48 * 64 + 1), "total"),
             (dict(ws_bytes=s.need - 1), "workspace"), (dict(ws=s.ptr["ws"] + 4), "aligned")]
    for kw, name in cases:
        with pytest.raises(RuntimeError, match=name):
            s(**dict(dict(inv_unit=iu), **kw))
    torch.cuda.synchronize()
    assert all(torch.equal(s.bufs[k], before[k]) for k in s.bufs)  # a refused call launches nothing


# ------------------------------------------------------------------------------------------------------------ verify is what it was
def test_render_compare_of_the_refined_poses(dev):
    """verify.render_compare on the refined poses equals its restatement, as before the raster pass moved into the shared header"""
    v, f, R, t, depth = _whole_scene()
    got = refine.refine_poses((_t(v, dev), _t(f, dev)), _t(R, dev), _t(t, dev), VR.INTR, _t(depth, dev), iters=5, gate=RF.GATE)
    check = verify.render_compare((_t(v, dev), _t(f, dev)), got.R, got.t, VR.INTR, _t(depth, dev), tol=0.01)
    Rn, tn = got.R.cpu().numpy(), got.t.cpu().numpy()
    view = np.concatenate([Rn, tn[:, :, None]], axis=2)
    box, dropped = VR.windows(v, f, view, VR.INTR, VR.SIZE)
    counts, ids, out = VR.pose_verify(v, f, view, VR.INTR, VR.SIZE, 1e-3, box, depth, None, 0.01)
    counts[:, 7] = dropped
    assert torch.equal(check.boxes, _t(box, dev)) and torch.equal(check.counts, _t(counts, dev))
    assert torch.equal(check.ids, _t(ids, dev)) and torch.equal(check.depth, _t(out, dev))
    start = verify.render_compare((_t(v, dev), _t(f, dev)), _t(R, dev), _t(t, dev), VR.INTR, _t(depth, dev), tol=0.01)
    assert float(check.inlier_ratio[0]) > 0.9 > float(start.inlier_ratio[0]) and float(check.inlier_ratio[1]) > 0.9
