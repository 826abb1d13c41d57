"""The inputs and bounds of tests/test_pose_shapes_gpu.py, proved on the CPU: every condition the exact comparisons rest on holds for
the seeded builders of tests/pose_shapes_ref.py (label margins and the share of labels left out, bitwise duplicates, conditioning,
minimum distances, score gaps, cut shares), and the fp32 oracle (oracle/pem_oracle.py) alone meets every bound of the TOL table
against the float64 restatements -- so the GPU file encodes no bound the reference arithmetic itself would miss."""
import pytest
import torch

from tests import pose_shapes_ref as R
from tests._util import golden
from oracle import pem_oracle as O


def _err(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) if got.numel() else 0.0


def _rel(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) if got.numel() else 0.0


def _oracle_stats(att):
    """the statistics the kernels export, as fp32 torch computes them"""
    rmax, cmax = att.max(2).values, att.max(1).values
    return rmax, torch.exp(att - rmax[:, :, None]).sum(2), cmax, torch.exp(att - cmax[:, None, :]).sum(1)


# ------------------------------------------------------------------------------------------------------- soft assignment
@pytest.mark.parametrize("shape", R.SA_SHAPES, ids=R.sa_id)
def test_soft_assign_inputs_and_oracle(shape):
    Rn, C = shape
    att, want = R.sa_case(Rn, C)
    # the raised entries sit where the builder says: the last column and the last row hold a raised entry
    assert float(att[:, :, C - 1].max()) > 6.0 and float(att[:, Rn - 1, :].max()) > 6.0
    s1, s2 = float(want["near1"].float().mean()), float(want["near2"].float().mean())
    print("%s: labels left out: %.4f of the rows, %.4f of the columns" % (shape, s1, s2))
    assert s1 <= R.LABEL_SHARE and s2 <= R.LABEL_SHARE
    rmax, rsum, cmax, csum = _oracle_stats(att)
    assert torch.equal(rmax, want["rmax"]) and torch.equal(cmax, want["cmax"])
    er, ec = _rel(rsum, want["rsum"]), _rel(csum, want["csum"])
    print("%s: fp32 sums vs float64: rows %.2e (bound %.2e), columns %.2e (bound %.2e)" % (shape, er, R.sum_tol(C), ec, R.sum_tol(Rn)))
    assert er <= R.sum_tol(C) and ec <= R.sum_tol(Rn)
    _, l1, l2 = O.soft_assignment(att)
    k1, k2 = ~want["near1"], ~want["near2"]
    assert torch.equal(l1[k1], want["l1"][k1]) and torch.equal(l2[k2], want["l2"][k2])


@pytest.mark.parametrize("case", R.TIE_CASES, ids=R.tie_id)
def test_tie_inputs_are_bitwise_duplicates(case):
    Rn, C, kind = case
    att, tie = R.tie_inputs(Rn, C, kind)
    a, b, where = tie["first"], tie["second"], tie["where"]
    assert 1 <= a < b
    bits = att.view(torch.int32)
    want = R.soft_assign64(att)
    if tie["axis"] == "col":
        assert torch.equal(bits[:, :, a], bits[:, :, b])
        assert (b - a) % 64 == 0 if kind == "col_same_lane" else (b % 64 != a % 64)
        lab, S = want["l1"][:, where - 1], want["S"][:, where, :]
        assert _rel(S[:, :, b], S[:, :, a]) <= 1e-12, "float64: the duplicates tie (to the order of its vectorised sums)"
        rest = S.clone()
        rest[:, :, [a, b]] = 0
        margin = (S[:, :, a] - rest.max(2).values) / S[:, :, a]
    else:
        assert torch.equal(bits[:, a, :], bits[:, b, :])
        per = (Rn + R.SA_SLICES - 1) // R.SA_SLICES
        assert (a // per == b // per) == (kind == "row_in_slice") or Rn <= 256
        lab, S = want["l2"][:, where - 1], want["S"][:, :, where]
        assert _rel(S[:, b, :], S[:, a, :]) <= 1e-12, "float64: the duplicates tie (to the order of its vectorised sums)"
        rest = S.clone()
        rest[:, [a, b], :] = 0
        margin = (S[:, a, :] - rest.max(1).values) / S[:, a, :]
    assert ((lab == a) | (lab == b)).all(), "float64 picks the duplicate class"
    assert float(margin.min()) > R.LABEL_REL, "the tied pair leads every other entry by more than the label margin"
    _, l1, l2 = O.soft_assignment(att)
    lo = l1[:, where - 1] if tie["axis"] == "col" else l2[:, where - 1]
    assert ((lo == a) | (lo == b)).all(), "the fp32 oracle picks the duplicate class"


@pytest.mark.parametrize("shape", [(197, 197), (257, 300)], ids=R.sa_id)
def test_bg_inputs_give_both_kinds_of_label(shape):
    att = R.bg_inputs(*shape)
    want = R.soft_assign64(att)
    for l, near in ((want["l1"], want["near1"]), (want["l2"], want["near2"])):
        assert float(near.float().mean()) <= R.LABEL_SHARE
        assert int((l[~near] == 0).sum()) > l.numel() // 4 and int((l[~near] > 0).sum()) > l.numel() // 4
    _, l1, l2 = O.soft_assignment(att)
    assert torch.equal(l1[~want["near1"]], want["l1"][~want["near1"]]) and torch.equal(l2[~want["near2"]], want["l2"][~want["near2"]])


@pytest.mark.parametrize("shape", R.ASSIGN_SHAPES, ids=R.sa_id)
def test_assign_inputs_and_oracle(shape):
    att, pts2 = R.assign_inputs(*shape)
    assert float(pts2.abs().max()) <= 0.5
    S, l1, l2 = O.soft_assignment(att)
    assert (l1[:, R.BG_ROW - 1] == 0).all(), "the bg row's label is the bg column"
    assert (R.soft_assign64(att)["l1"][:, R.BG_ROW - 1] == 0).all()
    want = R.assign64(att, l1, l2, pts2)
    weights, w1 = O.coarse_sampling_weights(att)
    A = S[:, 1:, 1:] * (l1 > 0).float().unsqueeze(2) * (l2 > 0).float().unsqueeze(1)
    pred = (A / (A.sum(2, keepdim=True) + 1e-6)) @ pts2  # (oracle/pem_oracle.py compute_fine_Rt, the lines before the solve)
    errs = dict(weights=_err(weights, want["weights"]), w1=_err(w1, want["w1"]), weight=_err(A.sum(2), want["weight"]), pred=_err(pred, want["pred"]))
    print("%s: fp32 oracle vs float64 %s" % (shape, errs))
    assert max(errs.values()) <= R.TOL["assign"]
    assert float(want["weight"][:, R.BG_ROW - 1].abs().max()) == 0.0 and float(want["pred"][:, R.BG_ROW - 1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- one-launch coarse path (LDS bound)
def test_one_launch_shapes_sit_at_the_lds_bound():
    assert R.cas_lds_bytes(199, 199) <= R.CAS_LIMIT < R.cas_lds_bytes(*R.CAS_OVER), "199 x 199 is the largest square"
    for _, Rn, C in R.CAS_SHAPES:
        assert R.cas_lds_bytes(Rn, C) <= R.CAS_LIMIT
    assert R.cas_lds_bytes(50, 770) == R.CAS_LIMIT and R.cas_lds_bytes(50, 771) > R.CAS_LIMIT, "the wide shape is exactly at the bound"
    assert R.cas_lds_bytes(256, 155) <= R.CAS_LIMIT < R.cas_lds_bytes(256, 156), "the tall shape is the last that fits"
    assert any(C < 64 for _, _, C in R.CAS_SHAPES)


def test_coarse_scene_200_oracle_recovers_the_pose():
    g = golden("coarse_rt")
    att, p1, p2, model, u = R.coarse_scene(g)
    assert att.shape[1:] == R.CAS_OVER and R.cas_lds_bytes(*att.shape[1:]) > R.CAS_LIMIT
    assert torch.equal(p1[:, :196], torch.from_numpy(g["p1"])) and torch.equal(p2[:, :196], torch.from_numpy(g["p2"]))
    Ro, to = O.compute_coarse_Rt(att, p1, p2, model, u)[:2]
    assert _err(Ro, g["R_gt"]) <= R.TOL["coarse_Rt"] and _err(to, g["t_gt"]) <= R.TOL["coarse_Rt"]


# ------------------------------------------------------------------------------------------------------- 3-point hypotheses
def test_hypothesis_inputs_and_oracle():
    pts1, pts2, idx, deg = R.hyp_inputs()
    B, N1, N2, nh = (R.HYP[k] for k in ("B", "N1", "N2", "nh"))
    assert N1 != N2 and (B * nh) % 256 != 0 and int(idx.max()) >= (N1 - 1) * N2 and int(idx.min()) < N2
    Rs, ts, dis, well = R.hypotheses64(idx, pts1, pts2, nh)
    share = 1.0 - float(well.float().mean())
    print("ill-posed share of the random triples: %.3f" % share)
    assert share <= 0.5
    Ro, to, do = O.coarse_hypotheses(idx.long(), pts1, pts2, nh)
    eR, et, ed = _err(Ro[well], Rs[well]), _err(to[:, :, 0][well], ts[well]), _err(do[well], dis[well])
    print("fp32 oracle vs float64 on %d well-posed triples: R %.2e, t %.2e, dis %.2e" % (int(well.sum()), eR, et, ed))
    assert eR <= R.TOL["hyp_Rt"] and et <= R.TOL["hyp_Rt"] and ed <= R.TOL["hyp_dis"]
    # the degenerate block: none of the four is well-posed, for the reason its name gives
    p1, p2, i1, i2 = R.hyp_triples(deg, pts1, pts2, 4)
    wd = R.hypotheses64(deg, pts1, pts2, 4)[3]
    assert not wd.any()
    assert (i1[:, 0, 0] == i1[:, 0, 1]).all() and (i2[:, 0, 0] == i2[:, 0, 1]).all() and (i1[:, 0, 0] != i1[:, 0, 2]).all()
    assert (i1[:, 1] == N1 - 1).all() and (i2[:, 1] == N2 - 1).all()
    coll = lambda p: torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=-1)
    assert float(coll(p1[:, 2]).max()) < 1e-6 and float(coll(p2[:, 2]).min()) > 1e-3, "collinear scene triple, general template triple"
    assert float(coll(p1[:, 3]).max()) < 1e-6 and float(coll(p2[:, 3]).max()) < 1e-6, "collinear on both sides"


# ------------------------------------------------------------------------------------------------------- hypothesis scoring
def _oracle_select(d):
    """O.coarse_select with `dis` built so that its top-k picks d['sel'] in order; one batch element at a time"""
    scores, best = [], []
    for b in range(d["B"]):
        dis = torch.full((1, d["nh"]), 1e9)
        dis[0, d["sel"][b].long()] = torch.arange(d["k"], dtype=torch.float32)
        m = d["model"][b:b + 1] / (d["radius"][b:b + 1].reshape(-1, 1, 1) + 1e-6)
        Rb, tb, top, sc = O.coarse_select(d["Rs"][b:b + 1].reshape(1, -1, 3, 3), d["ts"][b:b + 1].reshape(1, -1, 1, 3), dis, d["w1"][b:b + 1],
                                          d["pts1"][b:b + 1], m, d["k"])
        assert torch.equal(top[0].to(torch.int32), d["sel"][b])
        scores.append(sc[0])
        best.append(int(top[0, sc[0].argmax()]))
    return torch.stack(scores), torch.tensor(best)


@pytest.mark.parametrize("case", R.SCORE_CASES + R.SCORE_VECTOR_ONLY, ids=R.sa_id)
def test_score_inputs_and_oracle(case):
    N1, k, P = case
    d = R.score_case(N1, k, P)
    want = d["want"]
    assert len(set(d["sel"][0].tolist())) == k and int(d["sel"].max()) < d["nh"]
    assert want["dmin"] >= R.MIN_DIST, "nearest distance %.3f" % want["dmin"]
    for x in (d["pts1"], d["model"] / (d["radius"].reshape(-1, 1, 1) + 1e-6)):
        assert float(x.norm(dim=-1).max()) <= 1.0
    posed = (d["pts1"][:, None] - d["ts"][:, :, None]) @ d["Rs"].reshape(d["B"], -1, 3, 3)
    assert float(posed.norm(dim=-1).max()) <= 1.0, "posed scene points stay inside the unit ball"
    assert (want["gap"] > R.SCORE_GAP).all(), "float64 top two scores: relative gap %s" % want["gap"].tolist()
    assert bool((d["w1"] == 0).any()) or N1 == 1
    sc, best = _oracle_select(d)
    e = _rel(sc, want["scores"])
    print("%s: fp32 oracle scores vs float64, relative %.2e; top-two gap %s" % (case, e, want["gap"].tolist()))
    assert e <= R.TOL["score_rel"] and torch.equal(best, want["best"])


def test_score_edge_inputs():
    N1, k, P = R.SCORE_TIE
    z = R.score_case(N1, k, P, w1_kind="zero")
    assert float(z["w1"].abs().max()) == 0.0 and float(z["want"]["scores"].abs().max()) == 0.0
    assert torch.equal(z["want"]["best"], z["sel"][:, 0].long()), "all scores 0: the first"
    assert float(_oracle_select(z)[0].abs().max()) == 0.0
    t = R.score_case(N1, k, P, tie=True)
    sc = t["want"]["scores"]
    for b in range(t["B"]):
        at = torch.nonzero(sc[b] == sc[b].max())[:, 0].tolist()
        assert len(at) == 2 and at[0] % 4 != at[1] % 4, "two slots hold the maximum, in different positions of their groups of four"
        h0, h1 = int(t["sel"][b, at[0]]), int(t["sel"][b, at[1]])
        assert h0 != h1 and torch.equal(t["Rs"][b, h0].view(torch.int32), t["Rs"][b, h1].view(torch.int32))
        assert torch.equal(t["ts"][b, h0].view(torch.int32), t["ts"][b, h1].view(torch.int32))
        assert int(t["want"]["best"][b]) == h0
    assert (R.score_second_gap(sc) > R.SCORE_GAP).all()
    o_sc, o_best = _oracle_select(t)
    assert torch.equal(o_best, t["want"]["best"]) and _rel(o_sc, sc) <= R.TOL["score_rel"]


# ------------------------------------------------------------------------------------------------------- N-point Procrustes
@pytest.mark.parametrize("mode", R.PROC_MODES)
@pytest.mark.parametrize("N", R.PROC_N)
def test_procrustes_inputs_and_oracle(N, mode):
    d = R.proc_case(N, mode)
    w, thr = d["w"], d["thresh"]
    if mode == "cut":
        cut32 = w < thr                      # as the fp32 implementations decide it (0.3 rounded to fp32)
        cut64 = w.double() < thr
        share = float(cut64.float().mean())
        assert 0.2 <= share <= 0.4, "cut share %.3f" % share
        assert torch.equal(cut32, cut64) and torch.equal(w < torch.tensor(thr, dtype=torch.float32), cut64)
        assert float((w.double() - thr).abs().min()) > R.W_CLEAR
    if N >= 4:
        assert (d["cond"] > R.SIGMA_RATIO).all(), "conditioning %s" % d["cond"].tolist()
    Ro, to = O.weighted_procrustes(d["src"], d["ref"], w, thr)
    ok = d["cond"] > R.SIGMA_RATIO
    assert R.proper_error(d["R"]) <= 1e-12
    if N >= 3 and ok.any():
        eR, et = _err(Ro[ok], d["R"][ok]), _err(to[ok], d["t"][ok])
        print("N %d %s: fp32 oracle vs float64 R %.2e, t %.2e" % (N, mode, eR, et))
        assert eR <= R.TOL["proc_R"] and et <= R.TOL["proc_t"]
    if N == 2:
        both = torch.ones(d["src"].shape[0], dtype=torch.bool) if d["kept"] is None else d["kept"].all(1)
        if both.any():
            assert float(R.direction_error(d["R"], d["src"], d["ref"], w)[both].max()) <= 1e-6, "float64 maps the direction"
            # (not to 1e-16: eps = 1e-5 shrinks the centroids, which adds ~1e-10 / (|a| |b|) of a second direction to H)


@pytest.mark.parametrize("N", [3, 2049])
def test_procrustes_all_weights_cut(N):
    d = R.proc_case(N, "rand")
    w = d["w"] * 0.25
    assert float(w.max()) < R.W_THRESH - R.W_CLEAR
    Rr, t, H = R.procrustes64(d["src"], d["ref"], w, R.W_THRESH)
    assert float(H.abs().max()) == 0.0 and float(t.abs().max()) == 0.0, "no weight survives: H = 0 and both centroids are 0"


# ------------------------------------------------------------------------------------------------------- fine pose score
@pytest.mark.parametrize("case", R.FINE_SCORE_CASES, ids=R.sa_id)
def test_fine_score_inputs_clear_the_threshold(case):
    """what the exact count comparison of the GPU test rests on: no float64 nearest distance within FINE_SCORE_GAP of the threshold, and
    in every proposal some masked points are near and some are not"""
    N, P, thr = case
    d = R.fine_score_case(N, P, thr)
    w = d["want"]
    print("%s: smallest |distance - thr| %.2e; near %s of mask %s" % (case, w["gap"], w["near"].tolist(), w["mask"].tolist()))
    assert w["gap"] >= R.FINE_SCORE_GAP
    assert ((w["near"] > 0) & (w["near"] < w["mask"])).all()
    assert len(R.FINE_SCORE_RADIUS) == d["B"] and d["p1"].shape == (d["B"], N, 3) and d["model"].shape == (d["B"], P, 3)
    Rm = d["R"].double()
    assert float((Rm @ Rm.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-5, "R is orthogonal: distances are kept"


def test_fine_score_route_switch_shape():
    """Ppad * 20 bytes of planes within 64 KB - 64 B: P = 3264 is the last matrix-core cloud, one more point the first vector one"""
    pad = lambda P: (P + 31) & ~31
    assert R.FINE_SCORE_SWITCH[1] == 3264 and pad(3264) * 20 <= 65536 - 64 < pad(3265) * 20
