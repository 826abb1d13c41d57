"""The pose check (sam6d_hip.verify, csrc/verify.hip): the host side and the numpy restatement of the recipe (tests/verify_ref.py).
No GPU: the restatement against raster_ref's whole-image render, the class boundaries, the picture, pose_views, the binding, the
refusals and the kernels' resources from the code object's metadata."""
import numpy as np
import pytest
import torch

from tests import raster_ref as RR
from tests import verify_ref as VR
from tests._util import ROOT  # noqa: F401  (puts the package on sys.path)
from sam6d_hip import _lib, verify
from sam6d_hip import visualize as V

F32 = np.float32
MESHES = {"octahedron": RR.octahedron, "icosphere2": lambda: RR.icosphere(2)}


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_windows_hold_the_whole_image_render(mesh):
    """every pixel of raster_ref.render_view's mask lies in the restatement's window, the windowed depth is the crop of that render,
    and columns 1 .. 4 of counts sum to column 0"""
    v, f = MESHES[mesh]()
    view = VR.five_poses()
    box, dropped = VR.windows(v, f, view, VR.INTR, VR.SIZE)
    assert box[3].tolist() == [0, 0, -1, -1] and box[4].tolist() == [0, 0, -1, -1]
    assert dropped[2] > 0 and box[2, 2] >= box[2, 0] and dropped[4] == len(f) and dropped[0] == dropped[1] == dropped[3] == 0
    assert box[1, 2] == VR.SIZE[1] - 1 and box[1, 3] == VR.SIZE[0] - 1 and box[0, 2] < VR.SIZE[1] - 1  # clamped at the right and bottom
    setups = VR._setups(v, f, view, VR.INTR, VR.SIZE, 1e-3)
    renders = []
    for n in range(5):
        mask, depth = VR.render_depth(v, f, view[n], VR.INTR, VR.SIZE)
        renders.append((mask, depth))
        x0, y0, bw, bh = VR.clamp_box(box[n], VR.SIZE)
        inside = np.zeros(VR.SIZE, bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert not (mask & ~inside).any(), n
        zb = VR.window_zbuffer(setups[n], (x0, y0, bw, bh))
        assert np.array_equal(VR.window_depth(zb), depth[y0:y0 + bh, x0:x0 + bw]), n
        if bw:  # the window is tight: its first and last rows and columns hold a face's box (not necessarily a covered centre)
            assert mask.sum() > 0
    obs = renders[0][1].copy()
    obs[:24] += F32(0.5)
    obs[30:, :20] = 0
    masks = np.stack([m.astype(np.uint8) for m, _ in renders])
    for mk in (None, masks):
        counts, ids, depth_out = VR.pose_verify(v, f, view, VR.INTR, VR.SIZE, 1e-3, box, obs, mk, 0.01)
        assert np.array_equal(counts[:, 1:5].sum(axis=1), counts[:, 0])
        assert counts[:, 0].tolist() == [int(m.sum()) for m, _ in renders] and counts[:, 7].tolist() == dropped.tolist()
        if mk is None:
            assert not counts[:, 5:7].any()
        else:
            assert np.array_equal(counts[:, 5], counts[:, 0]) and np.array_equal(counts[:, 6], counts[:, 0])  # the renders' own masks
        assert np.array_equal(ids >= 0, np.any([m for m, _ in renders], axis=0))
        near = np.min([np.where(m, d, np.inf) for m, d in renders], axis=0)
        assert np.array_equal(depth_out, np.where(np.isfinite(near), near, 0).astype(F32))


def test_class_boundaries():
    """o = r + tau and o = r - tau with exactly representable values are inliers; the next float beyond is not; 0, a negative
    value and NaN are unknown whatever r is"""
    r, tau = F32(1.5), F32(0.25)
    up, down = np.nextafter(F32(1.75), F32(9)), np.nextafter(F32(1.25), F32(0))
    o = np.array([1.5, 1.75, 1.25, up, down, 0.0, -0.0, -1.0, np.nan, np.inf, 1e-30], F32)
    got = VR.classify(np.full_like(o, r), o, tau)
    assert got.tolist() == [VR.INLIER, VR.INLIER, VR.INLIER, VR.BEHIND, VR.OCCLUDED, VR.UNKNOWN, VR.UNKNOWN, VR.UNKNOWN, VR.UNKNOWN,
                            VR.BEHIND, VR.OCCLUDED]
    assert VR.classify(np.array([2.0], F32), np.array([2.0], F32), 0.0).tolist() == [VR.INLIER]  # tau = 0: equality alone


def test_overlay_restatement():
    g = np.random.default_rng(2)
    rgb = g.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    ids = np.full((6, 9), -1, np.int32)
    ids[1:5, 2:7] = 1
    colors = np.array([[9, 8, 7], [250, 100, 10]], np.uint8)
    inner = np.zeros((6, 9), bool)
    inner[2:4, 3:6] = True
    out0 = VR.overlay_instances(rgb, ids, colors, 0)
    assert out0.shape == (6, 18, 3) and np.array_equal(out0[:, :9], rgb)
    assert np.array_equal(out0[:, 9:][inner], rgb[inner]) and np.array_equal(out0[:, 9:][ids < 0], rgb[ids < 0])  # alpha = 0: rgb off the edges
    ring = (ids == 1) & ~inner
    assert (out0[:, 9:][ring] == colors[1]).all()  # the silhouette, unblended
    out256 = VR.overlay_instances(rgb, ids, colors, 256)
    assert (out256[:, 9:][ids == 1] == colors[1]).all() and np.array_equal(out256[:, 9:][ids < 0], rgb[ids < 0])
    half = VR.overlay_instances(rgb, ids, colors, 128)[:, 9:][inner]
    assert np.array_equal(half, ((rgb[inner].astype(int) * 128 + colors[1].astype(int) * 128 + 128) >> 8).astype(np.uint8))
    # an instance that fills the image has no edge: the border is none; an id out of range is background
    assert np.array_equal(VR.overlay_instances(rgb, np.zeros((6, 9), np.int32), colors, 256)[:, 9:], np.broadcast_to(colors[0], (6, 9, 3)))
    assert np.array_equal(VR.overlay_instances(rgb, np.full((6, 9), 2, np.int32), colors, 256)[:, 9:], rgb)


def test_pose_views_against_float64():
    g = np.random.default_rng(5)
    R = np.stack([VR.rotation(g.normal(size=3), a) for a in (0.3, 2.0, -1.1)]).astype(F32)
    t = g.normal(size=(3, 3)).astype(F32)
    M = verify.pose_views(torch.from_numpy(R), torch.from_numpy(t), 0.001)
    assert M.dtype == torch.float32 and tuple(M.shape) == (3, 3, 4) and M.is_contiguous()
    want = np.concatenate([R.astype(np.float64) * 0.001, t.astype(np.float64)[:, :, None]], axis=2)
    assert np.abs(M.numpy() - want).max() <= 2.0 ** -23 * 0.001  # scale rounded once, the product once
    assert np.array_equal(M.numpy()[:, :, :3], R * F32(0.001)) and np.array_equal(M.numpy()[:, :, 3], t)
    assert np.array_equal(verify.pose_views(torch.from_numpy(R), torch.from_numpy(t)).numpy()[:, :, :3], R)
    with pytest.raises(ValueError, match="R must"):
        verify.pose_views(torch.zeros(3, 3), torch.zeros(3))
    with pytest.raises(ValueError, match="t must"):
        verify.pose_views(torch.zeros(2, 3, 3), torch.zeros(3, 3))


def test_binding_lists_the_new_entries():
    for name in ("sam6d_pose_windows", "sam6d_pose_verify", "sam6d_pose_verify_workspace_bytes", "sam6d_overlay_instances"):
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["sam6d_pose_verify"]) == 26 and len(_lib.SIGNATURES["sam6d_pose_windows"]) == 16
    lib = _lib.load()
    assert lib.sam6d_pose_verify_workspace_bytes(0, 48, 64) == 8 * 48 * 64
    assert lib.sam6d_pose_verify_workspace_bytes(1000, 48, 64) == 8 * (1000 + 48 * 64)
    assert lib.sam6d_pose_verify_workspace_bytes(-1, 48, 64) == 0 and lib.sam6d_pose_verify_workspace_bytes(5, 2049, 64) == 0
    assert lib.sam6d_pose_verify_workspace_bytes(1024 * 48 * 64 + 1, 48, 64) == 0


def test_render_compare_refusals():
    v, f = RR.octahedron()
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.tensor([[0.0, 0.0, 4.0]] * 2)
    K = np.array([[60.0, 0, 32], [0, 60, 24], [0, 0, 1]])
    depth = torch.ones(48, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        verify.render_compare((v, f), R, t, K, depth)
    with pytest.raises(RuntimeError, match="HIP device"):
        verify.render_compare(dict(vertices=v.numpy(), faces=f.numpy()), R, t, K, depth)
    with pytest.raises(RuntimeError, match="HIP device"):
        verify.pose_windows(v, f, verify.pose_views(R, t), (60.0, 60.0, 32.0, 24.0), (48, 64))
    for kw, name in ((dict(R=R[:, :2]), "R"), (dict(t=t[:1]), "t"), (dict(depth=depth.double()), "depth"), (dict(depth=depth[None]), "depth"),
                     (dict(masks=torch.zeros(2, 48, 63, dtype=torch.uint8)), "masks"), (dict(masks=torch.zeros(2, 48, 64)), "masks"),
                     (dict(K=np.eye(4)), "K"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(mesh=(v.double(), f)), "vertices"),
                     (dict(mesh=(v, f.long())), "faces"), (dict(mesh=v), "mesh"), (dict(wave_area=-1), "wave_area"), (dict(near=0.0), "near"),
                     (dict(depth=torch.ones(48, 2049)), "2048"), (dict(R=torch.eye(3).repeat(1025, 1, 1), t=torch.zeros(1025, 3)), "N = 1025")):
        args = dict(mesh=(v, f), R=R, t=t, K=K, depth=depth)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            verify.render_compare(**args)
    rgb = torch.zeros(4, 5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ids"):
        V.overlay_instances(rgb, torch.zeros(4, 5), [[1, 2, 3]])
    with pytest.raises(ValueError, match="alpha"):
        V.overlay_instances(rgb, torch.zeros(4, 5, dtype=torch.int32), [[1, 2, 3]], alpha=300)
    with pytest.raises(ValueError, match="CPU"):
        V.overlay_instances(rgb, torch.zeros(4, 5, dtype=torch.int32), [[1, 2, 3]])
    with pytest.raises(ValueError, match="ids"):
        V.vis_pem_render(rgb, np.zeros((4, 5), np.int32))


def test_kernel_resources():
    """no kernel of verify.hip uses scratch or spills, and each keeps within its built VGPR count rounded
    up to the next step of 8 (built: windows_faces 80, windows_finish 6, verify_faces 63, verify_classify 22, verify_mask_area 12,
    verify_resolve 6, overlay_instances 14).  Read from the code object's metadata: the compiler's figures, not a GPU's."""
    from tests._util import kernel_resources
    limits = dict(windows_faces_kernel=80, windows_finish_kernel=8, verify_faces_kernel=64, verify_classify_kernel=24,
                  verify_mask_area_kernel=16, verify_resolve_kernel=8, overlay_instances_kernel=16)
    found = kernel_resources(b"verify_classify_kernel")
    print("\n[verify] (VGPRs, scratch bytes, spilled): %s" % found)
    assert set(found) == set(limits), found
    for name, cap in limits.items():
        assert found[name][0] <= cap and found[name][1:] == (0, 0), (name, found[name])
