"""The inputs and bounds of tests/test_fine_shapes_gpu.py, proved on the CPU: every condition the builders of tests/fine_shapes_ref.py
promise holds (the share of labels left out, bitwise ties that are the maximum with a clear third, the all-bg and no-bg label sets,
the zero rows, the antipodal cosines, the exponents of the range hole), and the float32 CPU restatement of the reference
(oracle/pem_oracle.py soft_assignment + the mask) alone meets every bound against the float64 one -- so the GPU file encodes no bound
the reference arithmetic itself would miss."""
import pytest
import torch

from tests import fine_shapes_ref as R
from oracle import pem_oracle as O


def _f32(F, B, temp, pts2):
    """compute_feature_similarity + the head of compute_fine_Rt in float32, one proposal at a time -> l1, l2, weight, pred"""
    out = []
    for b in range(B):
        f1 = torch.nn.functional.normalize(F[b][None], dim=2)
        f2 = torch.nn.functional.normalize(F[B + b][None], dim=2)
        S, l1, l2 = O.soft_assignment(f1 @ f2.transpose(1, 2) / temp)
        A = S[:, 1:, 1:] * (l1 > 0).float().unsqueeze(2) * (l2 > 0).float().unsqueeze(1)
        w = A.sum(2)
        out.append((l1[0], l2[0], w[0], ((A / (w.unsqueeze(2) + 1e-6)) @ pts2[b][None])[0]))
    return [torch.stack([o[k] for o in out]) for k in range(4)]


def _labels_ok(got, want, near, tiny, cand, what):
    """exact outside the near rows; a near label is one of the float64 candidates; rows beyond float32 (S_NORMAL) are left out"""
    got = got.long()
    keep = ~near & ~tiny
    bad = int((got[keep] != want[keep]).sum())
    assert bad == 0, "%s: %d labels differ from float64" % (what, bad)
    for b, c in enumerate(cand):
        for i, ok in c.items():
            assert bool(tiny[b, i]) or int(got[b, i]) in ok.tolist(), "%s: proposal %d, index %d: label %d is no float64 candidate" % (what, b, i, int(got[b, i]))


def _check_case(kind, temp, n=R.N, seeds=(0, 1)):
    F, pts2, want = R.case(kind, temp, n, seeds)
    B = len(seeds)
    s1, s2 = float((want["near1"] & ~want["tiny1"]).float().mean()), float(want["near2"].float().mean())
    print("%s temp %.4g n %d: labels left out: %.5f of the rows, %.5f of the columns (label_rel %.2e)" % (kind, temp, n, s1, s2, R.label_rel(temp)))
    assert s1 <= R.LABEL_SHARE and s2 <= R.LABEL_SHARE
    l1, l2, w, pred = _f32(F, B, temp, pts2)
    lo, hi = R.ANTIPODAL_ROWS
    t1 = torch.zeros_like(want["tiny1"])
    if kind == "antipodal":
        t1[:, lo - 1:hi - 1] = True
    assert torch.equal(want["tiny1"], t1) and not want["tiny2"].any(), "only the antipodal rows fall below float32's normal range"
    _labels_ok(l1, want["l1"], want["near1"], want["tiny1"], want["cand1"], "float32 l1")
    _labels_ok(l2, want["l2"], want["near2"], want["tiny2"], want["cand2"], "float32 l2")
    w64, p64 = R.assign_from(F, B, temp, l1, l2, pts2)
    ew = float(((w.double() - w64).abs() - R.weight_floor(n)).clamp_min(0).div(w64.clamp_min(1e-300)).max())
    ep = float(((pred.double() - p64).abs() - R.target_floor(n)).clamp_min(0).max()) / 0.5
    tab = R.F32_REL[min(R.F32_REL, key=lambda t: abs(t - temp))]
    print("%s temp %.4g n %d: float32 restatement vs float64, relative: weights %.2e, targets %.2e (table %.1e; bound of the GPU test %.2e)"
          % (kind, temp, n, ew, ep, tab, R.weight_rel(temp, n)))
    assert torch.isfinite(w).all() and torch.isfinite(pred).all()
    assert max(ew, ep) <= tab, "the table's entry is the float32 restatement's own error, rounded up"
    return F, pts2, want


@pytest.mark.parametrize("temp", R.TEMPS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_builders_and_float32_restatement(kind, temp):
    F, pts2, want = _check_case(kind, temp)
    assert float(pts2.abs().max()) <= 0.5
    B = pts2.shape[0]
    if kind == "all_bg":
        assert int(want["l1"].abs().max()) == 0, "every scene row prefers the bg column in float64"
        assert float(want["weight"].abs().max()) == 0.0 and float(want["pred"].abs().max()) == 0.0
    elif kind == "no_bg":
        assert int(want["l1"].min()) > 0 and int(want["l2"].min()) > 0, "no label is the bg token"
    elif kind == "matched":
        assert 0 < int((want["l1"] > 0).sum()) < want["l1"].numel() and 0 < int((want["l2"] > 0).sum())
    elif kind == "ranges":
        s, t = R.ZERO_ROWS
        assert s > 0 and t > 0
        for b in range(B):
            assert float(F[b, s].abs().max()) == 0.0 and float(F[B + b, t].abs().max()) == 0.0, "the zero rows exist"
            nrm = F[b].norm(dim=1)
            assert float(nrm[2::3].median()) > 1e9 * float(nrm[1::3].median()) and float(nrm[1::3].median()) > 1e9 * float(nrm[3::3].median())


def test_n4097_inputs():
    for kind in ("matched", "flat"):
        _check_case(kind, 0.1, 4097, (0,))


def test_smallest_temperature_inputs():
    """at MIN_TEMP the fixed shift still represents cos = -1: `antipodal` comes within 0.01 of it, and its rows and `flat` keep the
    conditions of every other case"""
    assert abs(R.MIN_TEMP - 2 * R.LOG2E / 125) < 1e-15 and -2 * R.LOG2E / R.MIN_TEMP > -126
    for kind in ("antipodal", "flat"):
        F, pts2, want = _check_case(kind, R.MIN_TEMP)
    F = R.case("antipodal", R.MIN_TEMP)[0]
    c = R.min_cos64(F, 2)
    print("antipodal: smallest cosine %.5f" % c)
    assert c < -0.99


def test_flat_at_temp_0005_underflows_the_fixed_shift():
    """the input that shows the range hole: with unrelated features the best exponent (cos_max - 1) log2e / temp of EVERY row lies below
    -126 at temp = 0.005, so every E of the row is flushed to 0 and the row sum is 0 -- while the reference softmax is exact"""
    F = R.case("flat", R.TEMPS[0])[0]
    e = R.best_exponent64(F, 2, 0.005)
    print("flat at temp 0.005: best exponent of a row between %.1f and %.1f" % (float(e.min()), float(e.max())))
    assert float(e.max()) < -126.0
    assert 0.005 < R.MIN_TEMP


@pytest.mark.parametrize("c", R.TIE_CASES, ids=R.tie_id)
def test_tie_inputs_are_bitwise_duplicates(c):
    axis, _, n, first, second, where = c
    F, pts2 = R.tie_inputs(c)
    assert 1 <= first < second < n and 1 <= where < n
    bits = F.view(torch.int32)
    cloud = 1 if axis == "tpl" else 0
    assert torch.equal(bits[cloud, first], bits[cloud, second])
    want = R.fine_match64(F, 1, R.TIE_TEMP)
    key = "1" if axis == "tpl" else "2"
    top, lab = want["top" + key][0, where - 1], int(want["l" + key][0, where - 1])
    assert lab in (first, second), "float64 picks the duplicate class"
    assert float((top[0] - top[1]) / top[0]) <= 1e-12, "float64: the duplicates tie (to the order of its vectorised sums)"
    margin = float((top[0] - top[2]) / top[0])
    print("%s: the third-best value is %.3f below the tied maximum (label_rel %.2e)" % (R.tie_id(c), margin, R.label_rel(R.TIE_TEMP)))
    assert margin > R.label_rel(R.TIE_TEMP)
    l1, l2, _, _ = _f32(F, 1, R.TIE_TEMP, pts2)
    assert int((l1 if axis == "tpl" else l2)[0, where - 1]) in (first, second), "the float32 restatement picks the duplicate class"
    s1, s2 = float(want["near1"].float().mean()), float(want["near2"].float().mean())
    assert s1 <= R.LABEL_SHARE and s2 <= R.LABEL_SHARE


def test_split_entry_inputs():
    """the projected tokens of the split-entry cases are matched pairs whose labels are decided by more than the chain's margin"""
    for B, n in ((2, R.N), (1, 4097)):
        x, W, b, pts2 = R.split_inputs(B, n, 1.0)
        F = R.chain64(x, W, b).reshape(2 * B, n, R.C)
        rel = R.label_rel(R.TIE_TEMP, R.chain_att_tol(R.TIE_TEMP))
        want = R.fine_match64(F, B, R.TIE_TEMP, rel=rel)
        s1, s2 = float(want["near1"].float().mean()), float(want["near2"].float().mean())
        print("split entry B %d n %d: labels left out %.5f / %.5f at margin %.2e" % (B, n, s1, s2, rel))
        assert s1 <= R.LABEL_SHARE and s2 <= R.LABEL_SHARE


def test_single_product_margin_leaves_few_labels_out():
    """`matched` at 0.1 with the margin of the hi . hi arithmetic (att_tol(temp, 2), 160 times the three-product one): every row label is
    still decided; of the columns, those whose scene partner became a bg copy have no match and fall inside the 4 % margin"""
    F, pts2, _ = R.case("matched", 0.1)
    rel = R.label_rel(0.1, R.att_tol(0.1, 2))
    want = R.fine_match64(F, 2, 0.1, rel=rel)
    s1, s2 = float(want["near1"].float().mean()), float(want["near2"].float().mean())
    print("matched at 0.1, margin %.2e: labels left out %.5f / %.5f" % (rel, s1, s2))
    assert s1 == 0.0 and s2 <= 0.05


def test_bounds_are_the_derived_figures():
    """the constants of the derivations, so that an edit of one shows"""
    assert abs(R.att_tol(1.0) - (2 * (2.0 ** -22 + 2.0 ** -31) + 2.0 ** -22 + 2.0 ** -18 + 13 * 2.0 ** -24 + 6 * 2.0 ** -24)) < 1e-18
    assert R.att_tol(0.1, 2) == 2.0 ** -10 / 0.1
    assert R.label_rel(0.1) == 4 * R.att_tol(0.1) + R.LABEL_REL
    assert R.weight_rel(0.1, 2049) >= 2 * R.att_tol(0.1) + 2 * R.sum_tol(2049)
