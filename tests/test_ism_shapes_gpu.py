"""The ISM template-scoring kernels (csrc/ism.hip) off their one golden shape: every entry point against a float64 evaluation of the
same operation (tests/ism_shapes_ref.py) at boundary shapes, several objects, tile counts other than 2 x 2, image sizes with a
partial last chunk, depth scales other than 1, exact ties and empty inputs.  The inputs are seeded and built so that every index /
count output is decided by a margin the kernels' rounding cannot cross (tests/test_ism_shapes_host.py proves those conditions and that
the fp32 oracle alone meets each tolerance); integer outputs are then compared exactly."""
import pytest
import torch

from tests import ism_shapes_ref as R
from tests.test_ism_gpu import ism_model  # noqa: F401  (the drop-in Instance_Segmentation_Model fixture)

pytestmark = pytest.mark.gpu


def _err(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) if got.numel() else 0.0


def _within(got, want, tol, what):
    e = _err(got, want)
    print("%s: max abs diff %.3e (bound %.1e)" % (what, e, tol))
    assert e <= tol, "%s: max abs diff %.3e > %.1e" % (what, e, tol)


# ------------------------------------------------------------------------------------------------------------- cosine
@pytest.mark.parametrize("shape", R.COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_shapes(dev, shape):
    from sam6d_hip import ism
    q, ref = R.cosine_inputs(*shape)
    got = ism.pairwise_similarity(q.to(dev), ref.to(dev))
    assert got.shape == (shape[0], shape[1], shape[2])
    _within(got, R.cosine64(q, ref), R.TOL["sim"], "cosine %s" % (shape,))


@pytest.mark.parametrize("D", [4, 36, 260, 1024])
def test_cosine_edge_rows(dev, D):
    from sam6d_hip import ism
    q, ref = R.cosine_edge_inputs(D)
    got = ism.pairwise_similarity(q.to(dev), ref.to(dev)).cpu()
    assert float(got[0].abs().max()) == 0.0 and float(got[:, 0, 0].abs().max()) == 0.0, "all-zero rows score 0"
    assert float(got[2, 0, 2]) == 0.0 and float(got.max()) <= 1.0 and float(got.min()) >= 0.0, "clamped to [0,1]"
    _within(got, R.cosine64(q, ref), R.TOL["sim"], "cosine edge rows D=%d" % D)


# ------------------------------------------------------------------------------------------------------------- semantic
def _semantic_both(dev, s, mode, thresh):
    """sam6d_ism_semantic_compact (through ism.semantic_select) and sam6d_ism_semantic (called directly) on the same scores"""
    from sam6d_hip import ism, _lib
    Nq, No, Nt = s.shape
    sd = s.to(dev)
    sel, obj, sem, best = ism.semantic_select(sd, mode, thresh)
    n = max(Nq, 1)
    r_sem = torch.empty(n, dtype=torch.float32, device=dev)
    r_int = torch.full((3 * n + 1,), -1, dtype=torch.int32, device=dev)  # obj | best | sel | count
    with torch.cuda.device(dev):
        _lib.call("sam6d_ism_semantic", sd.data_ptr(), Nq, No, Nt, R.MODES.index(mode), float(thresh), r_sem.data_ptr(), r_int.data_ptr(),
                  r_int.data_ptr() + 4 * n, r_int.data_ptr() + 8 * n, r_int.data_ptr() + 12 * n, torch.cuda.current_stream().cuda_stream)
    r_int = r_int.cpu()
    k = int(r_int[3 * n])
    raw = dict(sem=r_sem.cpu()[:Nq], obj=r_int[:Nq].long(), best=r_int[n:n + Nq].long(), sel=r_int[2 * n:2 * n + k].long())
    return dict(sel=sel.cpu(), obj=obj.cpu(), sem=sem.cpu(), best=best.cpu()), raw


def _check_semantic(dev, s, mode, thresh=0.2, dup_obj=None):
    d_thr, gap = R.semantic_conditions(s, mode, thresh, dup_obj=dup_obj)
    assert d_thr >= R.MARGIN and gap >= R.MARGIN, "input margins: threshold %.2e, object gap %.2e" % (d_thr, gap)
    want = R.semantic64(s, mode, thresh)
    cmp, raw = _semantic_both(dev, s, mode, thresh)
    ws = want["sel"]
    assert cmp["sel"].dtype == torch.int64 and cmp["obj"].dtype == torch.int64 and cmp["best"].dtype == torch.int64
    assert torch.equal(cmp["sel"], ws), "selected proposals (ascending)"
    assert torch.equal(cmp["obj"], want["obj"][ws]) and torch.equal(cmp["best"], want["best"][ws])
    assert _err(cmp["sem"], want["sem"][ws]) <= R.TOL["sem"]
    # the plain entry reports every query, selected or not
    assert torch.equal(raw["sel"], ws) and torch.equal(raw["obj"], want["obj"]) and torch.equal(raw["best"], want["best"])
    assert _err(raw["sem"], want["sem"]) <= R.TOL["sem"]
    assert torch.equal(raw["sem"][ws], cmp["sem"]), "the two entries run one kernel: same bits"
    return want


@pytest.mark.parametrize("Nq,No,Nt,mode", R.sem_cases())
def test_semantic_shapes(dev, Nq, No, Nt, mode):
    _check_semantic(dev, R.semantic_scores(Nq, No, Nt, mode), mode)


@pytest.mark.parametrize("mode", R.MODES)
def test_semantic_all_below_threshold(dev, mode):
    want = _check_semantic(dev, R.semantic_scores(65, 3, 65, mode, low=True), mode)
    assert want["sel"].numel() == 0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dup", sorted(R.TIE_TEMPLATES))
def test_semantic_template_ties(dev, mode, dup):
    """duplicated templates at the top of every row: the first maximum is the best template, and avg_5 takes the duplicates one
    occurrence per round (also when one lane holds several of them: templates 5, 69, 133)"""
    _check_semantic(dev, R.semantic_scores(65, 3, 162, mode, dup_templates=R.TIE_TEMPLATES[dup]), mode)


@pytest.mark.parametrize("mode", R.MODES)
def test_semantic_object_ties(dev, mode):
    """object 6 is an exact copy of object 2: the first of the two wins"""
    _check_semantic(dev, R.semantic_scores(65, 8, 65, mode, dup_obj=(2, 6)), mode, dup_obj=(2, 6))


def test_semantic_rejects_more_than_65535(dev):
    from sam6d_hip import ism
    with pytest.raises(RuntimeError):
        ism.semantic_select(torch.zeros(65536, 1, 1, device=dev), "max", 0.2)


def test_compute_semantic_score_3072_proposals(dev, ism_model):
    """the drop-in compute_semantic_score on the raw proposals of SAM's 32 x 32 point grid (three masks per point)"""
    m, loss = ism_model
    q, ref = R.descriptors_3072()
    assert R.descriptor_margins(q, ref, "avg_5", 0.2) >= R.MARGIN, "input margins: threshold, object gap, template gap"
    want = R.semantic64(R.cosine64(q, ref), "avg_5", 0.2)
    m.ref_data = {"descriptors": ref.to(dev)}
    sel, obj, sem, best = m.compute_semantic_score(q.to(dev))
    ws = want["sel"]
    assert torch.equal(sel.cpu(), ws) and torch.equal(obj.cpu(), want["obj"][ws]) and torch.equal(best.cpu(), want["best"][ws])
    _within(sem, want["sem"][ws], R.TOL["sem"], "semantic score of 3072 proposals")
    sel0 = m.compute_semantic_score(q[:0].to(dev))
    assert all(t.numel() == 0 for t in sel0), "no proposals in, none out"


# ------------------------------------------------------------------------------------------------------------- patch scores
@pytest.mark.parametrize("shape", R.PATCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_patch_scores_fused_shapes(dev, shape):
    """q_index absent (the gathered queries) and present (the queries read in place through a permutation with repeats), against
    float64 and against the materialised path (gather + GEMM + sam6d_ism_patch_scores) at three thresholds"""
    from sam6d_hip import ism
    d = R.patch_case(shape)
    margins = R.patch_conditions(d["red"])
    assert min(margins) >= R.MARGIN, "input margins: column maximum from a threshold %.2e, from 0 %.2e, patch sum from 0 %.2e" % margins
    q, ref, obj, best, qi = (d[k].to(dev) for k in ("q", "ref", "obj", "best", "qi"))
    q_sel = q[qi].contiguous()
    ps_plain = ism.patch_scores_fused(q_sel, ref, obj, best)
    ps_index = ism.patch_scores_fused(q, ref, obj, best, q_index=qi)
    ref_sel = ref[obj, best].contiguous()
    sim = ism.patch_similarity(q_sel, ref_sel)
    for thr in R.PATCH_THREDS:
        a64, v64 = R.patch_scores64(d["red"], thr)
        a1, v1 = ps_plain.scores(thr)
        a2, v2 = ps_index.scores(thr)
        assert torch.equal(a1, a2) and torch.equal(v1, v2), "q_index path differs from the gathered-query path"
        _within(a1, a64, R.TOL["appe"], "appearance %s" % (shape,))
        _within(v1, v64, R.TOL["vis"], "visible ratio %s at %g" % (shape, thr))
        a3, v3 = ism.patch_scores(sim, q_sel, thr)
        _within(a3, a64, R.TOL["appe"], "appearance, materialised %s" % (shape,))
        _within(v3, v64, R.TOL["vis"], "visible ratio, materialised %s at %g" % (shape, thr))
        _within(a1, a3.cpu(), 2e-6, "appearance: fused vs materialised")
        _within(v1, v3.cpu(), 1e-6, "visible ratio: fused vs materialised")
        for k in ("ng", "zq", "zt"):
            if d[k] is not None:
                assert float(a1[d[k]]) == 0.0 and float(v1[d[k]]) == 0.0, "proposal %s: appearance and visible ratio are exactly 0" % k


@pytest.mark.parametrize("P,D", [(100, 32), (128, 48)])
def test_patch_fused_rejects_other_tilings(dev, P, D):
    from sam6d_hip import _lib
    q = torch.zeros(1, P, D, device=dev)
    ref = torch.zeros(1, 1, P, D, device=dev)
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        _lib.call("sam6d_ism_patch_fused", q.data_ptr(), None, ref.data_ptr(), idx.data_ptr(), idx.data_ptr(), 1, 1, P, D, ws.data_ptr(),
                  ws.numel(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("P", [1, 100, 256, 300])
def test_patch_scores_alone(dev, P):
    from sam6d_hip import ism
    q, sim = R.sim_inputs(P)
    red = R.sim_reduce64(q, sim)
    assert min(R.patch_conditions(red)) >= R.MARGIN, "input margins"
    for thr in R.PATCH_THREDS:
        a64, v64 = R.patch_scores64(red, thr)
        a, v = ism.patch_scores(sim.to(dev), q.to(dev), thr)
        _within(a, a64, R.TOL["appe"], "appearance P=%d" % P)
        _within(v, v64, R.TOL["vis"], "visible ratio P=%d at %g" % (P, thr))


# ------------------------------------------------------------------------------------------------------------- projection
def _check_projection(d, got, what):
    vu, xyxy, tr = (t.cpu() for t in got)
    want_vu, keep, want_xyxy, share = R.projection_expect(d)
    assert share <= R.PX_SHARE, "share of projections within %g px of an integer: %.2e" % (R.PX_MARGIN, share)
    live, H, W = d["live"], d["H"], d["W"]
    ulp = int(R.ulp_distance(tr, d["translate"]).max())
    print("%s: translation %d ulp from float64 rounded once" % (what, ulp))
    assert ulp <= (0 if d["depth_scale"] == 1.0 else 1), "%s: translation %d ulp from the float64 reference" % (what, ulp)
    assert (tr[~live] == 0).all(), "an empty mask translates to 0"
    k = keep & live[:, None, None]
    nbad = int((vu[k] != want_vu[k]).sum())
    assert nbad == 0, "%s: %d of %d compared coordinates differ" % (what, nbad, int(k.sum()))
    whole = live & keep.all(-1).all(-1)
    assert torch.equal(xyxy[whole], want_xyxy[whole]), "%s: bounding boxes" % what
    for t in (vu, xyxy.reshape(-1, 2, 2)):
        assert (t[..., 0] >= 0).all() and (t[..., 0] < W).all() and (t[..., 1] >= 0).all() and (t[..., 1] < H).all()
    assert torch.equal(xyxy, torch.cat((vu.min(1).values, vu.max(1).values), -1)), "the box is the extent of the kernel's own pixels"
    return vu, xyxy, tr, k


@pytest.mark.parametrize("case", R.proj_cases(), ids=lambda c: "-".join(map(str, c)))
def test_projection_shapes(dev, case):
    from sam6d_hip import ism, _lib
    H, W, Npc, Ns, kind, with_index, ds = case
    d = R.proj_inputs(*case)
    best, obj, poses, pc, depth, K = (d[k].to(dev) for k in ("best", "obj", "poses", "pc", "depth", "K"))
    mi = d["mi"].to(dev) if with_index else None
    got = ism.project_template_to_image(best, obj, poses, pc, d["masks"].to(dev), depth, K, ds, mask_index=mi)
    vu, xyxy, tr, k = _check_projection(d, got, "project2" if W % 16 == 0 else "project")
    if W % 16:
        return
    # the general entry on the gathered float32 masks
    m32 = d["sel_masks"].float().to(dev)
    b32, o32 = best.to(torch.int32), obj.to(torch.int32)
    vu2 = torch.empty(Ns, Npc, 2, dtype=torch.int32, device=dev)
    xy2 = torch.empty(Ns, 4, dtype=torch.int32, device=dev)
    tr2 = torch.empty(Ns, 3, dtype=torch.float32, device=dev)
    part = torch.empty(Ns * 64 * 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("sam6d_ism_project", m32.data_ptr(), depth.data_ptr(), K.data_ptr(), float(ds), poses.data_ptr(), pc.data_ptr(),
                  b32.data_ptr(), o32.data_ptr(), Ns, H, W, Npc, part.data_ptr(), vu2.data_ptr(), xy2.data_ptr(), tr2.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    vu2, xy2, tr2, _ = _check_projection(d, (vu2, xy2, tr2), "project")
    assert torch.equal(vu2[k], vu[k]), "the two entries disagree on a compared coordinate"
    if ds == 1.0:
        assert torch.equal(tr2, tr)


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("shape", R.MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_translate_maps_shapes(dev, shape, N):
    from sam6d_hip import ism
    H, W = shape
    md = R.map_inputs(N, H, W)
    K = R.camera(480, 640)
    got = ism.translate_masked_depth_maps(md.to(dev), K.to(dev), 1.0)
    assert torch.equal(got.cpu(), R.translate_maps64(md, K, 1.0)), "float64 sums rounded once: bit-exact"


# ------------------------------------------------------------------------------------------------------------- IoU / final score
@pytest.mark.parametrize("Ns", R.IOU_NS)
def test_iou_and_final_score_shapes(dev, Ns):
    from sam6d_hip import ism, _lib
    sem_all, sel, appe, geo, vis = R.final_inputs(Ns)
    sem = sem_all[sel.long()]
    for spoil in (None, "touch", "disjoint"):
        if spoil and not Ns:
            continue
        a, b = R.iou_inputs(Ns, spoil)
        want, pos = R.iou64(a, b)
        iou, flag = ism.compute_iou(a.to(dev), b.to(dev), return_flag=True)
        assert int(flag.item()) == (1 if pos.all() else 0), "the flag clears exactly when a pair has a non-positive overlap"
        _within(iou.cpu()[pos], want[pos], R.TOL["iou"], "IoU Ns=%d %s" % (Ns, spoil))
        res = ism.compute_iou(a.to(dev), b.to(dev))
        assert (torch.is_tensor(res) and torch.equal(res, iou)) if pos.all() else (res == 0.0)
        # the quirk decided on the device: the geometric term counts only while the flag is set
        fin = ism.final_score(sem.to(dev), appe.to(dev), iou, vis.to(dev), all_positive=flag)
        _within(fin, R.final64(sem, appe, want if pos.all() else 0.0, vis), R.TOL["final"], "final score with the device flag")
    fin = ism.final_score(sem.to(dev), appe.to(dev), geo.to(dev), vis.to(dev))
    _within(fin, R.final64(sem, appe, geo, vis), R.TOL["final"], "final score")
    fin0 = ism.final_score(sem.to(dev), appe.to(dev), 0.0, vis.to(dev))  # geo = NULL
    _within(fin0, R.final64(sem, appe, 0.0, vis), R.TOL["final"], "final score without a geometric term")
    # a selection into the per-query scores (sel != NULL), with and without geo
    n = max(Ns, 1)
    out = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    sa, sl, ap, ge, vi = (t.to(dev) for t in (sem_all, sel, appe, geo, vis))
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream
        _lib.call("sam6d_ism_final_score", sa.data_ptr(), ap.data_ptr(), ge.data_ptr(), vi.data_ptr(), sl.data_ptr(), Ns, out.data_ptr(), s)
        _lib.call("sam6d_ism_final_score", sa.data_ptr(), ap.data_ptr(), None, vi.data_ptr(), sl.data_ptr(), Ns, out.data_ptr() + 4 * n, s)
    _within(out[:Ns], R.final64(sem, appe, geo, vis), R.TOL["final"], "final score through a selection")
    _within(out[n:n + Ns], R.final64(sem, appe, 0.0, vis), R.TOL["final"], "final score through a selection, no geometric term")
    if Ns:
        assert torch.equal(out[:Ns], fin) and torch.equal(out[n:n + Ns], fin0)
