"""The pose solvers (csrc/pose.hip) off the workload's own shapes: every entry point against a float64 evaluation of the same operation
(tests/pose_shapes_ref.py) on both sides of each boundary the code has -- R = 256 (one row slice / 16, expf / hardware exp), C = 2304
(register-resident row / loop), four rows a workgroup, 256-column blocks, the 160 KB LDS bound of the one-launch coarse path, N1 != N2 in
the hypothesis indices, the 32-point padding / groups of four / 64-lane arg-max of the two scoring routes, 2048 points in registers of
the N-point solve -- with exact ties and degenerate inputs.  The inputs are seeded and built so that every index output is decided by a
margin the kernels' rounding cannot cross; tests/test_pose_shapes_host.py proves those conditions and that the fp32 oracle alone meets
each bound of R.TOL.  Every device tensor is named, so that no temporary dies before its launch."""
import pytest
import torch

from tests import pose_shapes_ref as R
from tests._util import golden

pytestmark = pytest.mark.gpu


def _abs(got, want, tol, what):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    e = float((got - want).abs().max()) if got.numel() else 0.0
    print("%s: max abs diff %.3e (bound %.1e)" % (what, e, tol))
    assert e <= tol, "%s: max abs diff %.3e > %.1e" % (what, e, tol)


def _rel(got, want, tol, what):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    e = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) if got.numel() else 0.0
    print("%s: max rel diff %.3e (bound %.2e)" % (what, e, tol))
    assert e <= tol, "%s: max rel diff %.3e > %.2e" % (what, e, tol)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------- 1. statistics and labels
def _check_soft_assign(st, att, want, what):
    """statistics: maxima bit-equal, sums within the derived bound; labels exact outside the float64 near-ties"""
    Rn, C = att.shape[1:]
    assert torch.equal(st["rmax"].cpu(), want["rmax"]) and torch.equal(st["cmax"].cpu(), want["cmax"]), what + ": a max rounds nothing"
    _rel(st["rsum"], want["rsum"], R.sum_tol(C), what + " rsum")
    _rel(st["csum"], want["csum"], R.sum_tol(Rn), what + " csum")
    l1, l2 = st["l1"].cpu().long(), st["l2"].cpu().long()
    k1, k2 = ~want["near1"], ~want["near2"]
    n1, n2 = int((l1[k1] != want["l1"][k1]).sum()), int((l2[k2] != want["l2"][k2]).sum())
    print("%s: %d of %d row labels, %d of %d column labels compared" % (what, int(k1.sum()), k1.numel(), int(k2.sum()), k2.numel()))
    assert n1 == 0 and n2 == 0, "%s: %d row labels and %d column labels differ from float64" % (what, n1, n2)
    assert int(l1.min()) >= 0 and int(l1.max()) < C and int(l2.min()) >= 0 and int(l2.max()) < Rn
    return l1, l2


@pytest.mark.parametrize("shape", R.SA_SHAPES, ids=R.sa_id)
def test_soft_assign_shapes_vs_float64(dev, shape):
    """sam6d_soft_assign on both sides of R = 256 (256 / 257 / 258: one slice / 16 slices, the last of 2 rows at 257; expf / hardware
    exp) and of C = 2304 (2304 / 2305: register-resident row / loop), C < 64 (2, 64 columns and below), (R-1) % 4 != 0, C % 256 != 0,
    wide and tall; a raised entry in every row's and column's tail."""
    from sam6d_hip import pem
    att, want = R.sa_case(*shape)
    att_d = att.to(dev)
    st = pem.soft_assign(att_d)
    _check_soft_assign(st, att, want, "soft_assign %s" % (shape,))


@pytest.mark.parametrize("case", R.TIE_CASES, ids=R.tie_id)
def test_soft_assign_exact_ties(dev, case):
    """a column copied bitwise 64 columns on (one lane of the row pass holds both) and to the last column (another lane), a row copied
    inside a row slice and into the last slice: the duplicates' statistics are bit-equal and every tied label is the lower index"""
    from sam6d_hip import pem
    Rn, C, kind = case
    att, tie = R.tie_inputs(Rn, C, kind)
    a, b, where = tie["first"], tie["second"], tie["where"]
    att_d = att.to(dev)
    st = {k: v.cpu() for k, v in pem.soft_assign(att_d).items()}
    if tie["axis"] == "col":
        assert torch.equal(_bits(st["cmax"][:, a]), _bits(st["cmax"][:, b])) and torch.equal(_bits(st["csum"][:, a]), _bits(st["csum"][:, b]))
        got = st["l1"][:, where - 1]
    else:
        assert torch.equal(_bits(st["rmax"][:, a]), _bits(st["rmax"][:, b])) and torch.equal(_bits(st["rsum"][:, a]), _bits(st["rsum"][:, b]))
        got = st["l2"][:, where - 1]
    assert (got == a).all(), "tied labels must be the lower index %d (the copy is %d): %s" % (a, b, got.tolist())
    # everything else as in the untied cases; the float64 reference decides the tied labels by the order of its own sums, so they are left out
    want = R.soft_assign64(att)
    _check_soft_assign(st, att, want, "tie %s" % (case,))


@pytest.mark.parametrize("shape", [(197, 197), (257, 300)], ids=R.sa_id)
def test_soft_assign_bg_labels(dev, shape):
    """the bg column wins every second row and the bg row every second column: labels of 0 and above 0 both occur, exact vs float64"""
    from sam6d_hip import pem
    att = R.bg_inputs(*shape)
    att_d = att.to(dev)
    st = pem.soft_assign(att_d)
    l1, l2 = _check_soft_assign(st, att, R.soft_assign64(att), "bg labels %s" % (shape,))
    for l in (l1, l2):
        assert int((l == 0).sum()) > l.numel() // 4 and int((l > 0).sum()) > l.numel() // 4


# ------------------------------------------------------------------------------------------------------- 3. weights and assignment
@pytest.mark.parametrize("shape", R.ASSIGN_SHAPES, ids=R.sa_id)
def test_weights_and_assignment_vs_float64(dev, shape):
    """sam6d_coarse_weights and sam6d_fine_assign on the kernel's own statistics and labels: R = 256 / 257 (exact / fast form of
    fine_assign), tails (R-1) % 4 and (C-1) % 64, a row whose label is the bg column"""
    from sam6d_hip import _lib, pem
    Rn, C = shape
    att, pts2 = R.assign_inputs(Rn, C)
    B = att.shape[0]
    att_d, pts2_d = att.to(dev), pts2.to(dev)
    st = pem.soft_assign(att_d)
    weights = torch.full((B, (Rn - 1) * (C - 1)), -1.0, device=dev)
    w1 = torch.full((B, Rn - 1), -1.0, device=dev)
    pred = torch.full((B, Rn - 1, 3), -1.0, device=dev)
    weight = torch.full((B, Rn - 1), -1.0, device=dev)
    args = [st[k].data_ptr() for k in ("rmax", "rsum", "cmax", "csum", "l1", "l2")]
    _lib.call("sam6d_coarse_weights", att_d.data_ptr(), B, Rn, C, *args, weights.data_ptr(), w1.data_ptr(), _stream())
    _lib.call("sam6d_fine_assign", att_d.data_ptr(), B, Rn, C, *args, pts2_d.data_ptr(), pred.data_ptr(), weight.data_ptr(), _stream())
    torch.cuda.synchronize()
    l1, l2 = st["l1"].cpu().long(), st["l2"].cpu().long()
    want = R.assign64(att, l1, l2, pts2)
    for got, key in ((weights, "weights"), (w1, "w1"), (weight, "weight"), (pred, "pred")):
        _abs(got, want[key], R.TOL["assign"], "%s %s" % (key, shape))
    r = R.BG_ROW - 1
    assert (l1[:, r] == 0).all(), "row %d prefers the bg column" % R.BG_ROW
    assert float(weight[:, r].abs().max()) == 0.0 and float(pred[:, r].abs().max()) == 0.0 and float(w1[:, r].abs().max()) == 0.0
    assert float(weights.reshape(B, Rn - 1, C - 1)[:, r].abs().max()) == 0.0, "a bg row gives weight 0 and pred 0 exactly"
    assert int((l1 > 0).sum()) > 0 and float(weight.max()) > 0.0


# ------------------------------------------------------------------------------------------- 4. one-launch coarse path at its bound
def _one_launch(dev, att_d):
    from sam6d_hip import _lib
    B, Rn, C = att_d.shape
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    o = dict(rmax=z(B, Rn), rsum=z(B, Rn), cmax=z(B, C), csum=z(B, C), l1=z(B, Rn - 1, dt=torch.int32), l2=z(B, C - 1, dt=torch.int32),
             weights=z(B, (Rn - 1) * (C - 1)), w1=z(B, Rn - 1))
    _lib.call("sam6d_coarse_soft_assign", att_d.data_ptr(), B, Rn, C, *[o[k].data_ptr() for k in ("rmax", "rsum", "cmax", "csum", "l1", "l2",
                                                                                                    "weights", "w1")], _stream())
    torch.cuda.synchronize()
    return o


def test_coarse_soft_assign_refuses_the_first_shape_over_the_bound(dev):
    """200 x 200 is 800 bytes over the 160 KB: refused, and the message names the two-call path"""
    att_d = torch.zeros(1, *R.CAS_OVER, device=dev)
    with pytest.raises(RuntimeError, match="sam6d_soft_assign"):
        _one_launch(dev, att_d)


def test_coarse_soft_assign_tall_matrix_vs_float64(dev):
    """R = 257 inside the LDS bound: the two-call form now cuts the rows into 16 slices and takes the hardware exp, so the one launch
    (one sequential column sum, expf) is held to float64 instead of to the two-call bits"""
    att = R.sa_inputs(257, 150)
    assert R.cas_lds_bytes(257, 150) <= R.CAS_LIMIT
    att_d = att.to(dev)
    o = _one_launch(dev, att_d)
    l1, l2 = _check_soft_assign(o, att, R.soft_assign64(att), "one launch 257 x 150")
    want = R.assign64(att, l1, l2, torch.zeros(att.shape[0], 149, 3))
    _abs(o["weights"], want["weights"], R.TOL["assign"], "one launch 257 x 150 weights")
    _abs(o["w1"], want["w1"], 0.0, "one launch 257 x 150 w1")


def test_coarse_rt_200x200_takes_the_two_call_route(dev, monkeypatch):
    """pem.compute_coarse_Rt on the first attention that does not fit the one launch: sam6d_soft_assign + sam6d_coarse_weights run, and
    the pose is the oracle's"""
    from oracle import pem_oracle as O
    from sam6d_hip import _lib, pem
    att, p1, p2, model, u = R.coarse_scene(golden("coarse_rt"))
    assert att.shape[1:] == R.CAS_OVER
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    att_d, p1_d, p2_d, model_d, u_d = (x.to(dev) for x in (att, p1, p2, model, u))
    radius = torch.ones(att.shape[0], device=dev)
    Rg, tg = pem.compute_coarse_Rt(att_d, p1_d, p2_d, model_d, radius, u_d)
    torch.cuda.synchronize()
    assert "sam6d_soft_assign" in called and "sam6d_coarse_weights" in called and "sam6d_coarse_soft_assign" not in called
    Ro, to = O.compute_coarse_Rt(att, p1, p2, model, u)[:2]
    _abs(Rg, Ro, R.TOL["coarse_Rt"], "coarse R, 200 x 200")
    _abs(tg, to, R.TOL["coarse_Rt"], "coarse t, 200 x 200")


# ------------------------------------------------------------------------------------------------------- 5. 3-point hypotheses
def _hypotheses(dev, idx, pts1, pts2, nh):
    from sam6d_hip import _lib
    B, N1, N2 = pts1.shape[0], pts1.shape[1], pts2.shape[1]
    idx_d, p1_d, p2_d = idx.to(dev), pts1.to(dev), pts2.to(dev)
    Rs = torch.full((B, nh, 9), float("nan"), device=dev)
    ts = torch.full((B, nh, 3), float("nan"), device=dev)
    dis = torch.full((B, nh), float("nan"), device=dev)
    _lib.call("sam6d_coarse_hypotheses", idx_d.data_ptr(), p1_d.data_ptr(), p2_d.data_ptr(), B, N1, N2, nh, Rs.data_ptr(), ts.data_ptr(),
              dis.data_ptr(), _stream())
    torch.cuda.synchronize()
    return Rs.cpu().reshape(B, nh, 3, 3), ts.cpu(), dis.cpu()


def test_hypotheses_n1_not_n2_vs_float64(dev):
    """N1 = 50, N2 = 119 (idx / N2 and idx % N2 with N1 != N2), B * nh = 771 (total % 256 = 3): well-posed triples against float64 Kabsch"""
    pts1, pts2, idx, _ = R.hyp_inputs()
    nh = R.HYP["nh"]
    Rs, ts, dis = _hypotheses(dev, idx, pts1, pts2, nh)
    assert torch.isfinite(Rs).all() and torch.isfinite(ts).all() and torch.isfinite(dis).all()
    R64, t64, d64, well = R.hypotheses64(idx, pts1, pts2, nh)
    assert 1.0 - float(well.float().mean()) <= 0.5
    _abs(Rs[well], R64[well], R.TOL["hyp_Rt"], "well-posed hypothesis rotations")
    _abs(ts[well], t64[well], R.TOL["hyp_Rt"], "well-posed hypothesis translations")
    _abs(dis[well], d64[well], R.TOL["hyp_dis"], "well-posed hypothesis residuals")
    assert R.proper_error(Rs) <= R.TOL["proper"], "every rotation is proper, ill-posed triples included"


def test_hypotheses_degenerate_triples(dev):
    """a pair sampled twice, three times, three collinear points, both sides collinear: finite proper rotations, and the residual is the
    residual of the pose returned"""
    pts1, pts2, _, deg = R.hyp_inputs()
    Rs, ts, dis = _hypotheses(dev, deg, pts1, pts2, len(R.HYP_DEGENERATE))
    assert torch.isfinite(Rs).all() and torch.isfinite(ts).all() and torch.isfinite(dis).all()
    e = R.proper_error(Rs)
    print("degenerate triples: orthonormality / determinant error %.2e" % e)
    assert e <= R.TOL["proper"]
    p1, p2, _, _ = R.hyp_triples(deg, pts1, pts2, len(R.HYP_DEGENERATE))
    _abs(dis, R.residual64(p1, p2, Rs, ts), R.TOL["hyp_dis"], "degenerate hypothesis residuals from the kernel's own R, t")


# ------------------------------------------------------------------------------------------------------- 6. hypothesis scoring
def _score(dev, d, route):
    """route "ws": sam6d_score_select_hypotheses_ws (matrix cores); "vec": sam6d_score_select_hypotheses (vector ALU)"""
    from sam6d_hip import _lib
    B, N1, k, P, nh = d["B"], d["N1"], d["k"], d["P"], d["nh"]
    sel, Rs, ts, pts1, w1, model, radius = (d[x].to(dev) for x in ("sel", "Rs", "ts", "pts1", "w1", "model", "radius"))
    scores = torch.full((B, k), float("nan"), device=dev)
    Rb = torch.full((B, 3, 3), float("nan"), device=dev)
    tb = torch.full((B, 3), float("nan"), device=dev)
    best = torch.full((B,), -1, dtype=torch.int32, device=dev)
    common = (sel.data_ptr(), Rs.data_ptr(), ts.data_ptr(), pts1.data_ptr(), w1.data_ptr(), model.data_ptr(), radius.data_ptr(), B, N1, P, nh, k,
              scores.data_ptr(), Rb.data_ptr(), tb.data_ptr(), best.data_ptr())
    if route == "ws":
        ws = torch.empty(max(B * N1 * k, 1), device=dev)
        _lib.call("sam6d_score_select_hypotheses_ws", *common, ws.data_ptr(), ws.numel() * 4, _stream())
    else:
        _lib.call("sam6d_score_select_hypotheses", *common, _stream())
    torch.cuda.synchronize()
    return dict(scores=scores.cpu(), R=Rb.cpu(), t=tb.cpu(), best=best.cpu().long())


def _check_score(d, out, what, expect_best=None):
    want = d["want"]
    _rel(out["scores"], want["scores"], R.TOL["score_rel"], what + " scores")
    exp = want["best"] if expect_best is None else expect_best
    decided = (want["gap"] > R.SCORE_GAP) if expect_best is None else torch.ones_like(exp, dtype=torch.bool)
    assert decided.all(), "the builder keeps the float64 top two apart"
    assert torch.equal(out["best"], exp), "%s: best %s, float64 %s" % (what, out["best"].tolist(), exp.tolist())
    for b in range(d["B"]):
        h = int(exp[b])
        assert torch.equal(out["R"][b].reshape(9), d["Rs"][b, h]) and torch.equal(out["t"][b], d["ts"][b, h]), what + ": pose of the best"


def _check_routes_agree(a, b, what):
    _rel(a["scores"], b["scores"], R.TOL["routes_rel"], what + " scores, matrix cores vs vector ALU")
    assert torch.equal(a["best"], b["best"]) and torch.equal(a["R"], b["R"]) and torch.equal(a["t"], b["t"]), what + ": the routes disagree"


@pytest.mark.parametrize("case", R.SCORE_CASES, ids=R.sa_id)
def test_score_select_both_routes_vs_float64(dev, case):
    """N1 x k x P: P = 1 / 31 / 33 / 1000 (padding to 32 with +inf, the P % 4 tail of the vector kernel), k = 1 / 5 / 63 / 300 (k % 4: the
    groups of four clamp to k - 1; k < 64 in pick_best), k * N1 % 32, N1 = 1 .. 257; w1 with zeros"""
    d = R.score_case(*case)
    ws, vec = _score(dev, d, "ws"), _score(dev, d, "vec")
    _check_score(d, ws, "matrix cores %s" % (case,))
    _check_score(d, vec, "vector ALU %s" % (case,))
    _check_routes_agree(ws, vec, str(case))


def test_score_select_all_weights_zero(dev):
    """w1 all zero: every score is exactly 0 and the first of `sel` wins"""
    d = R.score_case(*R.SCORE_TIE, w1_kind="zero")
    for route in ("ws", "vec"):
        out = _score(dev, d, route)
        assert float(out["scores"].abs().max()) == 0.0, route
        assert torch.equal(out["best"], d["sel"][:, 0].long()), route


def test_score_select_identical_hypotheses_tie_goes_to_the_first(dev):
    """the best pose sits in two slots of `sel` (bitwise copies, in different positions of their groups of four): the first wins"""
    d = R.score_case(*R.SCORE_TIE, tie=True)
    ws, vec = _score(dev, d, "ws"), _score(dev, d, "vec")
    for out, what in ((ws, "matrix cores"), (vec, "vector ALU")):
        _check_score(d, out, what + " tie", expect_best=d["want"]["best"])
    _check_routes_agree(ws, vec, "tie")


@pytest.mark.parametrize("case", R.SCORE_VECTOR_ONLY, ids=R.sa_id)
def test_score_select_vector_route_large_clouds(dev, case):
    """P = 4097 (64 KB + 16 bytes of CAD points) and P = 8192 (128 KB): the dynamic LDS the vector-ALU route reserves for its kernel"""
    d = R.score_case(*case)
    _check_score(d, _score(dev, d, "vec"), "vector ALU %s" % (case,))


def test_score_select_documented_refusals(dev):
    d = R.score_case(37, 5, 31)
    with pytest.raises(RuntimeError, match="P <= 4096"):
        _score(dev, dict(d, P=4097), "ws")
    with pytest.raises(RuntimeError, match="P <= 8192"):
        _score(dev, dict(d, P=8193), "vec")


# ------------------------------------------------------------------------------------------------------- 7. N-point Procrustes
@pytest.mark.parametrize("mode", R.PROC_MODES)
@pytest.mark.parametrize("N", R.PROC_N)
def test_weighted_procrustes_sizes_vs_float64(dev, N, mode):
    """N = 1 .. 4097: N < 256 (threads without a point), 255 / 256 / 257, 2047 / 2048 (registers) and 2049 / 4097 (the re-reading
    branch); weights absent, random, and random cut at 0.3"""
    from sam6d_hip import pem
    d = R.proc_case(N, mode)
    src_d, ref_d = d["src"].to(dev), d["ref"].to(dev)
    w_d = None if d["w"] is None else d["w"].to(dev)
    Rg, tg = pem.weighted_procrustes(src_d, ref_d, w_d, d["thresh"])
    Rg, tg = Rg.cpu(), tg.cpu()
    assert torch.isfinite(Rg).all() and torch.isfinite(tg).all()
    e = R.proper_error(Rg)
    assert e <= R.TOL["proper"], "proper rotation: %.2e" % e
    ok = d["cond"] > R.SIGMA_RATIO
    if N >= 4:
        assert ok.all()
    if N >= 3 and ok.any():
        _abs(Rg[ok], d["R"][ok], R.TOL["proc_R"], "R, N = %d, %s" % (N, mode))
        _abs(tg[ok], d["t"][ok], R.TOL["proc_t"], "t, N = %d, %s" % (N, mode))
    if N == 2:
        both = torch.ones(Rg.shape[0], dtype=torch.bool) if d["kept"] is None else d["kept"].all(1)
        if both.any():
            de = float(R.direction_error(Rg, d["src"], d["ref"], d["w"])[both].max())
            print("N = 2, %s: direction error %.2e" % (mode, de))
            assert de <= R.TOL["dir2"]


@pytest.mark.parametrize("N", [3, 2049])
def test_weighted_procrustes_all_weights_cut(dev, N):
    """no weight reaches the threshold: H = 0 and both centroids are 0 -> R = I and t = 0 exactly (registers and re-reading branch)"""
    from sam6d_hip import pem
    d = R.proc_case(N, "rand")
    src_d, ref_d, w_d = d["src"].to(dev), d["ref"].to(dev), (d["w"] * 0.25).to(dev)
    Rg, tg = pem.weighted_procrustes(src_d, ref_d, w_d, R.W_THRESH)
    assert torch.equal(Rg.cpu(), torch.eye(3).expand(Rg.shape[0], 3, 3)) and float(tg.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------- 8. fine pose score
def _fine_score(dev, d, model=None):
    """sam6d_fine_score -> cnt (B,2) = (near, mask) counts, score (B,), t (B,3) rescaled, all on the host"""
    from sam6d_hip import _lib
    model = d["model"] if model is None else model
    p1, Rm, model_d, radius, l1 = (x.to(dev).contiguous() for x in (d["p1"], d["R"], model, d["radius"], d["l1"]))
    t = d["t"].to(dev).clone()
    cnt = torch.full((d["B"], 2), float("nan"), device=dev)
    score = torch.full((d["B"],), float("nan"), device=dev)
    _lib.call("sam6d_fine_score", p1.data_ptr(), Rm.data_ptr(), t.data_ptr(), model_d.data_ptr(), radius.data_ptr(), l1.data_ptr(), d["B"], d["N"],
              model.shape[1], float(d["thr"]), cnt.data_ptr(), score.data_ptr(), _stream())
    torch.cuda.synchronize()
    return cnt.cpu(), score.cpu(), t.cpu()


@pytest.mark.parametrize("case", R.FINE_SCORE_CASES, ids=R.sa_id)
def test_fine_score_counts_vs_float64(dev, case):
    """both CAD layouts of sam6d_fine_score at their edges: P = 31 / 33 / 97 (padding to 32 rows, the vector minimum's tail), N = 63 / 65 /
    300, P = 3264 (the last cloud on the matrix cores) and 3265 (the first on the vector ALU).  Every float64 nearest distance keeps
    FINE_SCORE_GAP from the threshold (tests/test_pose_shapes_host.py), ten times the fp32 recipe's error: the counts are exact."""
    d = R.fine_score_case(*case)
    w = d["want"]
    cnt, score, t = _fine_score(dev, d)
    print("%s: near %s (float64 %s), mask %s (float64 %s)" % (case, cnt[:, 0].tolist(), w["near"].tolist(), cnt[:, 1].tolist(), w["mask"].tolist()))
    assert torch.equal(cnt[:, 0].double(), w["near"]) and torch.equal(cnt[:, 1].double(), w["mask"])
    _rel(score, w["score"], 4 * 2.0 ** -24, "fine score %s" % (case,))  # two divisions and a product of exact counts
    _abs(t, d["t"].double() * (d["radius"].double()[:, None] + 1e-6), 2.0 ** -24, "rescaled t %s" % (case,))  # |t| <= 0.05 * 1.000001: within an ulp of 0.0625


def test_fine_score_route_switch_keeps_the_bits(dev):
    """the P = 3264 cloud (matrix cores) and the same cloud plus a copy of its first point (P = 3265: vector ALU): a duplicate cannot
    change a minimum, so counts and score are bit-equal across the route switch"""
    d = R.fine_score_case(*R.FINE_SCORE_SWITCH)
    longer = torch.cat([d["model"], d["model"][:, :1]], 1).contiguous()
    assert longer.shape[1] == 3265
    a, b = _fine_score(dev, d), _fine_score(dev, d, longer)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))
    assert torch.equal(a[0][:, 0].double(), d["want"]["near"])
