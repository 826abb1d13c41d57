"""The inputs and bounds of tests/test_ism_shapes_gpu.py, proved on the CPU: every input condition the exact comparisons rest on
holds for the seeded builders of tests/ism_shapes_ref.py (decision margins, the share of near-integer projections), and the fp32
oracle (oracle/ism_oracle.py) alone meets every tolerance against the float64 restatements -- so the GPU file encodes no bound the
reference itself would miss."""
import pytest
import torch

from tests import ism_shapes_ref as R
from oracle import ism_oracle as IO


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) if got.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------- cosine
@pytest.mark.parametrize("shape", R.COSINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cosine_oracle_meets_the_bound(shape):
    q, ref = R.cosine_inputs(*shape)
    e = _err(IO.pairwise_similarity(q, ref), R.cosine64(q, ref))
    print("cosine %s: fp32 oracle vs float64 %.3e" % (shape, e))
    assert e <= R.TOL["sim"]


@pytest.mark.parametrize("D", [4, 36, 260, 1024])
def test_cosine_edge_rows(D):
    q, ref = R.cosine_edge_inputs(D)
    want = R.cosine64(q, ref)
    assert float(want[0].abs().max()) == 0.0 and float(want[:, 0, 0].abs().max()) == 0.0, "all-zero rows score 0"
    assert abs(float(want[1, 0, 1]) - 1.0) <= 1e-12 and float(want[2, 0, 2]) == 0.0, "identical pair 1, opposite pair 0"
    assert torch.isfinite(want).all()
    e = _err(IO.pairwise_similarity(q, ref), want)
    print("cosine edge rows D=%d: fp32 oracle vs float64 %.3e" % (D, e))
    assert e <= R.TOL["sim"]


# ------------------------------------------------------------------------------------------------------------- semantic
def _oracle_semantic(monkeypatch, scores, mode, thresh):
    monkeypatch.setattr(IO, "pairwise_similarity", lambda q, r: scores)
    return IO.semantic_score(None, None, mode, thresh)


def _check_semantic_oracle(monkeypatch, s, mode, thresh, want):
    sel, obj, sem, best = _oracle_semantic(monkeypatch, s, mode, thresh)
    assert torch.equal(sel, want["sel"]) and torch.equal(obj, want["obj"][sel]) and torch.equal(best, want["best"][sel])
    assert _err(sem, want["sem"][sel]) <= R.TOL["sem"]


@pytest.mark.parametrize("Nq,No,Nt,mode", R.sem_cases())
def test_semantic_inputs_and_oracle(monkeypatch, Nq, No, Nt, mode):
    s = R.semantic_scores(Nq, No, Nt, mode)
    d_thr, gap = R.semantic_conditions(s, mode, 0.2)
    assert d_thr >= R.MARGIN and gap >= R.MARGIN, "margins: threshold %.2e, object gap %.2e" % (d_thr, gap)
    want = R.semantic64(s, mode, 0.2)
    if Nq:
        assert int(want["obj"][0]) == No - 1 and int(want["best"][0]) == Nt - 1, "the last object / template must be reached"
    if Nq >= 63:
        assert 0 < want["sel"].numel() < Nq, "both sides of the threshold"
    if mode == "avg_5" and Nt < 5:
        return  # torch.topk(k=5) raises here: the mean of the Nt largest is this library's contract, stated by aggregate64 alone
    _check_semantic_oracle(monkeypatch, s, mode, 0.2, want)


@pytest.mark.parametrize("mode", R.MODES)
def test_semantic_all_below_threshold(monkeypatch, mode):
    s = R.semantic_scores(65, 3, 65, mode, low=True)
    assert R.semantic_conditions(s, mode, 0.2)[0] >= R.MARGIN
    assert R.semantic64(s, mode, 0.2)["sel"].numel() == 0
    assert _oracle_semantic(monkeypatch, s, mode, 0.2)[0].numel() == 0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dup", sorted(R.TIE_TEMPLATES))
def test_semantic_template_ties(monkeypatch, mode, dup):
    s = R.semantic_scores(65, 3, 162, mode, dup_templates=R.TIE_TEMPLATES[dup])
    d_thr, gap = R.semantic_conditions(s, mode, 0.2)
    assert d_thr >= R.MARGIN and gap >= R.MARGIN
    want = R.semantic64(s, mode, 0.2)
    first = R.TIE_TEMPLATES[dup][0]  # (an earlier template that holds the maximum by itself comes first)
    assert (want["best"] <= first).all() and int((want["best"] == first).sum()) > 32, "first maximum wins"
    _check_semantic_oracle(monkeypatch, s, mode, 0.2, want)


@pytest.mark.parametrize("mode", R.MODES)
def test_semantic_object_ties(monkeypatch, mode):
    s = R.semantic_scores(65, 8, 65, mode, dup_obj=(2, 6))
    d_thr, gap = R.semantic_conditions(s, mode, 0.2, dup_obj=(2, 6))
    assert d_thr >= R.MARGIN and gap >= R.MARGIN
    want = R.semantic64(s, mode, 0.2)
    assert (want["obj"][1::2] == 2).all() and not (want["obj"] == 6).any(), "first object wins"
    _check_semantic_oracle(monkeypatch, s, mode, 0.2, want)


def test_compute_semantic_score_inputs_3072():
    q, ref = R.descriptors_3072()
    assert R.descriptor_margins(q, ref, "avg_5", 0.2) >= R.MARGIN
    want = R.semantic64(R.cosine64(q, ref), "avg_5", 0.2)
    assert 1024 < want["sel"].numel() < 3072 and int(want["sel"][-1]) > 2048
    sel, obj, sem, best = IO.semantic_score(q, ref, "avg_5", 0.2)
    assert torch.equal(sel, want["sel"]) and torch.equal(obj, want["obj"][sel]) and torch.equal(best, want["best"][sel])
    assert _err(sem, want["sem"][sel]) <= R.TOL["sem"]


# ------------------------------------------------------------------------------------------------------------- patch scores
@pytest.mark.parametrize("shape", R.PATCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_patch_inputs_and_oracle(shape):
    d = R.patch_case(shape)
    No, Nt = shape[0], shape[1]
    d_thr, d_zero, d_row = R.patch_conditions(d["red"])
    assert min(d_thr, d_zero, d_row) >= R.MARGIN, "margins: threshold %.2e, zero %.2e, patch sum %.2e" % (d_thr, d_zero, d_row)
    assert (int(d["obj"].max()), int(d["best"][d["obj"] == No - 1].max())) == (No - 1, Nt - 1)
    assert len(set(d["qi"].tolist())) < len(d["qi"]), "q_index repeats a query"
    q_sel = d["q"][d["qi"]]
    appe, ref_sel = IO.appearance_score(d["best"], d["obj"], q_sel, d["ref"])
    a64, _ = R.patch_scores64(d["red"], 0.5)
    assert all(float(a64[d[k]]) == 0.0 for k in ("ng", "zq", "zt") if d[k] is not None)
    assert (d["zq"] is not None and d["zt"] is not None) or shape[4] < 5
    ng_cm = d["red"]["colmax"][d["ng"]]
    assert (ng_cm < 0).all(), "negated template: every column maximum non-zero and below the thresholds"
    assert 0.0 < float(a64.max()) < 1.0
    e = _err(appe, a64)
    print("appearance %s: fp32 oracle vs float64 %.3e" % (shape, e))
    assert e <= R.TOL["appe"]
    seen = []
    for thr in R.PATCH_THREDS:
        v64 = R.patch_scores64(d["red"], thr)[1]
        seen.append(v64)
        e = _err(IO.visible_ratio(q_sel, ref_sel, thr), v64)
        print("visible ratio %s at %g: fp32 oracle vs float64 %.3e" % (shape, thr, e))
        assert e <= R.TOL["vis"]
    assert not torch.equal(seen[1], seen[2]), "the thresholds must separate column maxima"


@pytest.mark.parametrize("P", [1, 100, 256, 300])
def test_sim_inputs(P):
    q, sim = R.sim_inputs(P)
    red = R.sim_reduce64(q, sim)
    d_thr, d_zero, d_row = R.patch_conditions(red)
    assert min(d_thr, d_zero, d_row) >= R.MARGIN
    for thr in R.PATCH_THREDS:  # the same reductions in fp32
        a64, v64 = R.patch_scores64(red, thr)
        a32 = (sim.max(2).values.sum(-1) / (torch.count_nonzero(q.sum(-1), dim=-1) + 1e-6)).clamp(0, 1)
        cm = sim.max(1).values
        v32 = torch.count_nonzero(cm * (cm > thr), dim=-1) / (torch.count_nonzero(cm, dim=-1) + 1e-6)
        assert _err(a32, a64) <= R.TOL["appe"] and _err(v32, v64) <= R.TOL["vis"]


# ------------------------------------------------------------------------------------------------------------- projection
@pytest.mark.parametrize("case", R.proj_cases(), ids=lambda c: "-".join(map(str, c)))
def test_projection_inputs_and_oracle(case):
    H, W, Npc, Ns, kind, with_index, ds = case
    d = R.proj_inputs(*case)
    vu, keep, xyxy, share = R.projection_expect(d)
    assert share <= R.PX_SHARE, "share of projections within %g px of an integer: %.2e" % (R.PX_MARGIN, share)
    assert (int(d["best"][0]), int(d["obj"][0])) == (5, 2)
    live = d["live"]
    assert (d["translate"][~live] == 0).all() and (d["translate"][live][:, 2] > 0).all()
    if with_index:
        assert len(set(d["mi"].tolist())) < Ns or Ns < 3, "mask_index repeats a mask"
    ds_t = torch.tensor([ds], dtype=torch.float64)
    m32 = d["sel_masks"].float()
    tr = IO.query_translation(m32, d["depth"], d["K"], ds_t)
    ulp = int(R.ulp_distance(tr, d["translate"]).max())
    assert ulp <= (0 if ds == 1.0 else 1), "translation: %d ulp" % ulp
    got = IO.project_template_to_image(d["best"], d["obj"], d["poses"], d["pc"], m32, d["depth"], d["K"], ds_t)
    k = keep & live[:, None, None]
    assert torch.equal(got[k], vu[k])
    assert (got[..., 0] >= 0).all() and (got[..., 0] < W).all() and (got[..., 1] >= 0).all() and (got[..., 1] < H).all()


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("shape", R.MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_translate_maps_oracle(shape, N):
    H, W = shape
    md = R.map_inputs(N, H, W)
    K = R.camera(480, 640)
    assert H * W < 4 or ((md < 0).any() and (md == 0).any() and (md > 0).any())
    want = R.translate_maps64(md, K, 1.0)
    ds_t = torch.tensor([1.0], dtype=torch.float64)
    got = torch.cat([IO.query_translation(torch.ones(1, H, W), md[i], K, ds_t) for i in range(N)])
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------- IoU / final score
@pytest.mark.parametrize("Ns", R.IOU_NS)
def test_iou_final_oracle(Ns):
    a, b = R.iou_inputs(Ns)
    want, pos = R.iou64(a, b)
    assert pos.all()
    if Ns >= 3:
        assert int(a.max()) > 2 ** 19
    got = IO.compute_iou(a.long(), b)
    assert torch.is_tensor(got) and _err(got, want) <= R.TOL["iou"]
    for spoil in ("touch", "disjoint"):
        if Ns:
            a2, b2 = R.iou_inputs(Ns, spoil)
            p2 = R.iou64(a2, b2)[1]
            assert int((~p2).sum()) == 1
            assert IO.compute_iou(a2.long(), b2) == 0.0
    sem_all, sel, appe, geo, vis = R.final_inputs(Ns)
    sem = sem_all[sel.long()]
    assert _err(IO.final_score(sem, appe, geo, vis), R.final64(sem, appe, geo, vis)) <= R.TOL["final"]
    assert _err(IO.final_score(sem, appe, 0.0, vis), R.final64(sem, appe, 0.0, vis)) <= R.TOL["final"]
