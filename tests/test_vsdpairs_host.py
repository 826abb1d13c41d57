"""All-pairs VSD without a device: the restatement tests/vsdpairs_ref.py (one render per view, the pairs by the overlap of their
windows) against tests/poseerr_ref.py's vsd_counts on the expanded pairs (union windows, two renders per pair) bit for bit, the
generalised vsd_from_counts, the workspace formula, and the refusals of posematch.pair_vsd and vsd_matches that need no launch."""
import numpy as np
import pytest
import torch

from tests import poseerr_ref as PR
from tests import verify_ref as VR
from tests import vsdpairs_ref as VP
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, poseerr, posematch

F32 = np.float32


def test_the_split_gives_the_pair_restatements_integers():
    """9 x 8 poses: every one of the 72 x (4 + 4) counts equals what the pair restatement counts in the pair's union window"""
    s = VP.mixed()
    counts, view_counts, box, X = VP.mixed_want()
    A, B = len(s.a), len(s.b)
    old = PR.vsd_counts(s.mesh[0], s.mesh[1], VP.expand(s.a, s.b), s.intr, s.size, VP.NEAR, s.obs, s.delta, s.taus, s.inv_norm)
    assert counts.dtype == np.int32 and counts.shape == (A, B, 8) and np.array_equal(counts.reshape(A * B, 8), old)
    assert np.array_equal(VP.vsd_of(counts).reshape(A * B, 4), PR.vsd_of(old))
    # the scene has pairs of each kind, or the comparison would prove nothing
    E, G = view_counts[:A, 1], view_counts[A:, 1]
    areas = VR.areas(box, s.size)
    assert (counts[:, :, 1] > 0).sum() >= 20                                   # the renders meet
    assert (counts[:, :, 2] > E[:, None]).sum() >= 5                           # the estimate gains pixels through `|| visib_gt`
    assert (counts[:, :, 4] > counts[:, :, 7]).any() and (counts[:, :, 7] > 0).any()
    assert ((X[:, :, 2] == 0) & (areas[:A, None] > 0) & (areas[None, A:] > 0)).any()   # two windows that do not meet
    assert (areas[:A, None] + areas[None, A:] == 0).any()                      # both windows empty
    assert np.array_equal(counts[:, :, 3], np.broadcast_to(G[None, :], (A, B)))
    assert (view_counts[:, 1] < view_counts[:, 0]).any() and (view_counts[:, 1] <= view_counts[:, 0]).all()
    assert (counts[:, :, 0] + counts[:, :, 1] == counts[:, :, 2] + counts[:, :, 3]).all()


def test_the_restatement_of_a_scene_without_windows_is_all_zero():
    five = VR.five_poses()
    s = VP._scene(VP.RR.icosphere(2), five[[VP.OFF, VP.BEHIND]], five[[VP.BEHIND, VP.OFF, VP.OFF]], np.ones(VR.SIZE, F32))
    counts, view_counts, _, _ = VP.want(s)
    assert counts.shape == (2, 3, 5) and not counts.any() and not view_counts.any() and (VP.vsd_of(counts) == 1).all()


def test_vsd_from_counts_takes_leading_dimensions():
    counts = torch.from_numpy(VP.mixed_want()[0])
    A, B, C = counts.shape
    flat, cube = poseerr.vsd_from_counts(counts.reshape(A * B, C)), poseerr.vsd_from_counts(counts)
    assert flat.dtype == cube.dtype == torch.float32 and tuple(flat.shape) == (A * B, C - 4) and tuple(cube.shape) == (A, B, C - 4)
    assert torch.equal(flat.reshape(A, B, C - 4), cube) and torch.equal(flat, torch.from_numpy(PR.vsd_of(counts.reshape(A * B, C).numpy())))
    assert (cube == 1).any() and ((cube > 0) & (cube < 1)).any()


def test_the_entries_are_bound_and_the_workspace_formula():
    assert len(_lib.SIGNATURES["sam6d_pose_pair_vsd"]) == 28 and len(_lib.SIGNATURES["sam6d_pose_pair_vsd_workspace_bytes"]) == 3
    lib = _lib.load()
    f = lib.sam6d_pose_pair_vsd_workspace_bytes
    assert f(0, 1, 1) == 64 and f(1001, 7, 3) == 8 * 1001 + 8 * 501 + 32 * 10 and f(1 << 28, 1024, 1024) == 12 * (1 << 28) + 32 * 2048
    bad = ((-1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 1025, 1), (0, 1, 1025), (2 * 2048 * 2048 + 1, 1, 1))
    assert [f(*a) for a in bad] == [0] * len(bad)
    assert posematch.MAX_VSD_WORDS == 1 << 28


def _args(A=2, B=3, size=(12, 16)):
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    eye = torch.eye(3)
    return dict(mesh=(v, f), R_a=eye.repeat(A, 1, 1), t_a=torch.zeros(A, 3), R_b=eye.repeat(B, 1, 1), t_b=torch.zeros(B, 3), K=VR.INTR,
                depth=torch.zeros(size), delta=0.1, taus=[0.05])


@pytest.mark.parametrize("change, kind, match", [
    (dict(R_a=torch.zeros(2, 3, 4)), ValueError, "R_a"), (dict(R_a=torch.zeros(2, 3, 3, dtype=torch.float64)), ValueError, "R_a"),
    (dict(t_a=torch.zeros(3, 3)), ValueError, "t_a"), (dict(R_b=torch.zeros(3, 3)), ValueError, "R_b"),
    (dict(t_b=torch.zeros(3, 3, dtype=torch.float16)), ValueError, "t_b"), (dict(t_b=np.zeros((3, 3), F32)), ValueError, "t_b"),
    (dict(R_a=torch.zeros(0, 3, 3), t_a=torch.zeros(0, 3)), ValueError, "A = 0"),
    (dict(R_a=torch.zeros(1025, 3, 3), t_a=torch.zeros(1025, 3)), ValueError, "A = 1025"),
    (dict(R_b=torch.zeros(0, 3, 3), t_b=torch.zeros(0, 3)), ValueError, "B = 0"),
    (dict(R_b=torch.zeros(1025, 3, 3), t_b=torch.zeros(1025, 3)), ValueError, "B = 1025"),
    (dict(depth=torch.zeros(12, 16, dtype=torch.float64)), ValueError, "depth"), (dict(depth=torch.zeros(16)), ValueError, "depth"),
    (dict(depth=torch.zeros(12, 2049)), ValueError, "H x W"), (dict(mesh=torch.zeros(3, 3)), ValueError, "mesh"),
    (dict(mesh=(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64))), ValueError, "faces"), (dict(K=np.zeros(5)), ValueError, "K"),
    (dict(near=0.0), ValueError, "near"),
    (dict(taus=[]), ValueError, "T = 0"), (dict(taus=[0.1] * 17), ValueError, "T = 17"), (dict(taus=[0.1, -0.1]), ValueError, "taus"),
    (dict(taus=[float("nan")]), ValueError, "taus"), (dict(delta=-1.0), ValueError, "delta"), (dict(delta=float("nan")), ValueError, "delta"),
    (dict(diameter=0.0), ValueError, "diameter"), (dict(diameter=-2.0), ValueError, "diameter"), (dict(diameter=float("inf")), ValueError, "diameter"),
    (dict(), RuntimeError, "HIP device")])
def test_pair_vsd_refusals(change, kind, match):
    """the error kinds are poseerr.vsd's: a wrong shape or dtype is a ValueError naming the argument, CPU tensors a RuntimeError"""
    with pytest.raises(kind, match=match):
        posematch.pair_vsd(**{**_args(), **change})


def test_pair_vsd_and_vsd_refuse_alike():
    """the same bad tolerances through the same helper: the messages differ in the function's name alone"""
    a = _args(A=2, B=2)
    for change in (dict(delta=-1.0), dict(taus=[0.1] * 17), dict(taus=[-0.5]), dict(diameter=0.0)):
        kw = {**a, **change}
        with pytest.raises(ValueError) as new:
            posematch.pair_vsd(**kw)
        with pytest.raises(ValueError) as old:
            poseerr.vsd(kw["mesh"], kw["R_a"], kw["t_a"], kw["R_b"], kw["t_b"], kw["K"], kw["depth"], kw["delta"], kw["taus"],
                        diameter=kw.get("diameter"))
        assert str(new.value).replace("pair_vsd", "vsd") == str(old.value)


@pytest.mark.parametrize("vsd, scores, kind, match", [
    (torch.zeros(3, 4), torch.zeros(3), ValueError, "vsd"), (torch.zeros(3, 4, 2, dtype=torch.float64), torch.zeros(3), ValueError, "vsd"),
    (np.zeros((3, 4, 2), F32), torch.zeros(3), ValueError, "vsd"), (torch.zeros(3, 4, 0), torch.zeros(3), ValueError, "T = 0"),
    (torch.zeros(3, 4, 17), torch.zeros(3), ValueError, "T = 17"), (torch.zeros(3, 4, 2), torch.zeros(4), ValueError, "scores"),
    (torch.zeros(3, 4, 2), torch.zeros(3), RuntimeError, "HIP device")])
def test_vsd_matches_refusals(vsd, scores, kind, match):
    with pytest.raises(kind, match=match):
        posematch.vsd_matches(vsd, scores, [0.3])


def test_vsd_matches_refuses_what_match_poses_refuses():
    with pytest.raises(ValueError, match="thresholds"):
        posematch.vsd_matches(torch.zeros(3, 4, 2), torch.zeros(3), [])
    with pytest.raises(ValueError, match="max_ests"):
        posematch.vsd_matches(torch.zeros(3, 4, 2), torch.zeros(3), [0.3], max_ests=-1)
    with pytest.raises(ValueError, match="valid"):
        posematch.vsd_matches(torch.zeros(3, 4, 2), torch.zeros(3), [0.3], valid=torch.zeros(3, dtype=torch.bool))
