"""The fused fine-match pipeline (csrc/finematch.hip: sam6d_fine_match and sam6d_fine_match_split, the entry production takes behind
sam6d_linear_norm_split) off its two test inputs: every case against a float64 evaluation of the same operation
(tests/fine_shapes_ref.py) at three temperatures and the smallest one the fixed softmax shift serves, batches on both sides of the
groups of eight proposals, n = 4097 (chunk merges), bitwise ties in every place first-maximum-wins is decided, operand rows of extreme
magnitude and zero, all-bg and no-bg outcomes, a poisoned workspace, and the refusals.  tests/test_fine_shapes_host.py proves the
conditions the exact comparisons rest on and that the float32 restatement alone meets each bound.  Every device tensor is named, so that
no temporary dies before its launch."""
import ctypes

import pytest
import torch

from tests import fine_shapes_ref as R

pytestmark = pytest.mark.gpu

I_SENT, F_SENT = -7, -3.0  # what the outputs hold before a call


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(x):
    return x.contiguous().view(torch.int32)


def _default_arithmetic():
    from sam6d_hip import _lib
    if _lib.load().sam6d_get_matmul_mode() != 1:
        pytest.skip("bounds of the three-product arithmetic (matmul mode 1, the library default)")


def _outputs(dev, B, n):
    return (torch.full((B, n - 1), I_SENT, dtype=torch.int32, device=dev), torch.full((B, n - 1), I_SENT, dtype=torch.int32, device=dev),
            torch.full((B, n - 1, 3), F_SENT, device=dev), torch.full((B, n - 1), F_SENT, device=dev))


def _untouched(out):
    l1, l2, pred, w = out
    return bool((l1 == I_SENT).all() and (l2 == I_SENT).all() and (pred == F_SENT).all() and (w == F_SENT).all())


def _workspace(dev, B, n, fill=None):
    from sam6d_hip import _lib
    nbytes = int(_lib.load().sam6d_fine_match_workspace_bytes_n(B, n))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws, nbytes


def _raw(dev, F, B, n, temp, pts2, fill=None, halves=None):
    """sam6d_fine_match on F (2B, n, 256), or sam6d_fine_match_split on the halves (fh, fl) -> l1, l2, pred, weight on the host"""
    from sam6d_hip import _lib
    out = _outputs(dev, B, n)
    ws, nbytes = _workspace(dev, B, n, fill)
    p2 = pts2.to(dev).contiguous()
    tail = (B, n, float(temp), p2.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), nbytes, _stream())
    if halves is None:
        f = F.reshape(-1, R.C).to(dev).contiguous()
        _lib.call("sam6d_fine_match", f.data_ptr(), *tail)
    else:
        _lib.call("sam6d_fine_match_split", halves[0].data_ptr(), halves[1].data_ptr(), *tail)
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in out)


def _check(out, F, pts2, want, temp, what, tol=None):
    """labels exact where float64 decides them, a float64 candidate where it does not; weights and targets relative, from the labels
    returned; -> the labels"""
    B, n = pts2.shape[0], pts2.shape[1] + 1
    l1, l2, pred, w = out
    assert torch.isfinite(pred).all() and torch.isfinite(w).all(), what + ": non-finite values"
    assert int(l1.min()) >= 0 and int(l1.max()) < n and int(l2.min()) >= 0 and int(l2.max()) < n, what + ": a label outside 0 .. n - 1"
    for got, key in ((l1.long(), "1"), (l2.long(), "2")):
        near, tiny = want["near" + key], want["tiny" + key]
        keep = ~near & ~tiny
        bad = int((got[keep] != want["l" + key][keep]).sum())
        print("%s: l%s: %d of %d compared, %d differ" % (what, key, int(keep.sum()), keep.numel(), bad))
        assert bad == 0, "%s: %d labels l%s differ from float64" % (what, bad, key)
        for b, cand in enumerate(want["cand" + key]):
            for i, ok in cand.items():
                assert bool(tiny[b, i]) or int(got[b, i]) in ok.tolist(), "%s: proposal %d, l%s[%d] = %d is no float64 candidate" % (what, b, key, i, int(got[b, i]))
    if "weight" in want and torch.equal(l1.long(), want["l1"]) and torch.equal(l2.long(), want["l2"]):
        w64, p64 = want["weight"], want["pred"]
    else:
        w64, p64 = R.assign_from(F, B, temp, l1, l2, pts2)
    rel = R.weight_rel(temp, n, tol)
    dw, dp = (w.double() - w64).abs(), (pred.double() - p64).abs()
    ew = float((dw - R.weight_floor(n)).clamp_min(0).div(w64.clamp_min(1e-300)).max())
    ep = float((dp - R.target_floor(n)).clamp_min(0).max()) / 0.5
    print("%s: weights rel %.3e, targets rel %.3e (bound %.2e; largest weight %.3e)" % (what, ew, ep, rel, float(w64.max())))
    assert bool((dw <= rel * w64 + R.weight_floor(n)).all()), "%s: weights rel %.3e > %.2e" % (what, ew, rel)
    assert bool((dp <= rel * 0.5 + R.target_floor(n)).all()), "%s: targets rel %.3e > %.2e" % (what, ep, rel)
    return l1, l2


# ------------------------------------------------------------------------------------------------------- 1. labels against float64
@pytest.mark.parametrize("temp", R.TEMPS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_builders_vs_float64(dev, kind, temp):
    """every builder at temp 1.0 / 0.1 / 0.03, B = 2, n = 2049 through sam6d_fine_match"""
    _default_arithmetic()
    F, pts2, want = R.case(kind, temp)
    out = _raw(dev, F, 2, R.N, temp, pts2)
    l1, l2 = _check(out, F, pts2, want, temp, "%s at %g" % (kind, temp))
    if kind == "all_bg":
        assert int(l1.abs().max()) == 0 and float(out[2].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0, "all bg: weights and targets are exactly 0"
    if kind == "no_bg":
        assert int(l1.min()) > 0 and int(l2.min()) > 0
    if kind == "matched":
        assert 0 < int((l1 > 0).sum()) < l1.numel()


# ------------------------------------------------------------------------------------------------------- 2. n = 4097
@pytest.mark.parametrize("kind", ["matched", "flat"])
def test_n4097_chunk_merges_vs_float64(dev, kind):
    """two 2048-column chunks: fm_merge_rows_kernel (labels) and fm_assign_merge_kernel (the four sums)"""
    _default_arithmetic()
    F, pts2, want = R.case(kind, 0.1, 4097, (0,))
    _check(_raw(dev, F, 1, 4097, 0.1, pts2), F, pts2, want, 0.1, "%s, n = 4097" % kind)


# ------------------------------------------------------------------------------------------------------- 3. batch grouping
GROUP_SEEDS = tuple(range(10, 19))


@pytest.mark.parametrize("B", [1, 7, 8, 9])
def test_batch_groups_of_eight_vs_float64(dev, B):
    """fm_sim_kernel deals proposals to workgroups in groups of eight: a group short of eight, exactly one, and one proposal in a second
    group; proposal b is the same whatever B is"""
    _default_arithmetic()
    F, pts2, want = R.case("matched", 0.1, R.N, GROUP_SEEDS[:B])
    _check(_raw(dev, F, B, R.N, 0.1, pts2), F, pts2, want, 0.1, "matched, B = %d" % B)


def test_a_proposal_does_not_depend_on_its_batch(dev):
    """proposal 8 of a B = 9 call (alone in the second group of eight) equals, bitwise, a B = 1 call on its features; two identical
    B = 9 calls are bitwise equal"""
    F, pts2 = R.stack([R.proposal("matched", R.N, s) for s in GROUP_SEEDS])
    a = _raw(dev, F, 9, R.N, 0.1, pts2, fill=0)
    b = _raw(dev, F, 9, R.N, 0.1, pts2, fill=0xFF)
    F1, p1 = R.stack([R.proposal("matched", R.N, GROUP_SEEDS[8])])
    assert torch.equal(F1[0], F[8]) and torch.equal(F1[1], F[17])
    c = _raw(dev, F1, 1, R.N, 0.1, p1)
    for x, y, z, name in zip(a, b, c, ("label1", "label2", "pred", "weight")):
        assert torch.equal(_bits(x), _bits(y)), name + ": two identical calls differ"
        assert torch.equal(_bits(x[8:9]), _bits(z)), name + ": proposal 8 of 9 differs from the same proposal alone"


# ------------------------------------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("c", R.TIE_CASES, ids=R.tie_id)
def test_bitwise_ties_go_to_the_first_index(dev, c):
    """duplicated template rows (columns of S) inside a lane's group of four, across its groups, across lanes, with the lower column in
    the higher lane, across the GEMM tile edge and across the 2048-column chunks; duplicated scene rows inside a wave, across waves,
    with the lower row in the higher wave, across 64-row slabs and the tile edge: the label is the first index, exactly"""
    _default_arithmetic()
    axis, _, n, first, second, where = c
    F, pts2 = R.tie_inputs(c)
    want = R.fine_match64(F, 1, R.TIE_TEMP, pts2)
    out = _raw(dev, F, 1, n, R.TIE_TEMP, pts2)
    got = int((out[0] if axis == "tpl" else out[1])[0, where - 1])
    assert got == first, "%s: the tied label must be the lower index %d (the copy is %d): got %d" % (R.tie_id(c), first, second, got)
    # everything else as in the untied cases (float64 decides the tied label by the order of its own sums: it is a `near` one)
    _check(out, F, pts2, want, R.TIE_TEMP, "tie " + R.tie_id(c))


# ------------------------------------------------------------------------------------------------------- 5. the split entry
@pytest.mark.parametrize("B,n,scale", [(2, R.N, 1.0), (1, 4097, 1.0), (2, R.N, 1e4), (2, R.N, 1e-4)])
def test_linear_norm_split_then_fine_match_split_vs_float64(dev, B, n, scale):
    """the chain production runs: sam6d_linear_norm_split (out_proj + normalise + fp16 split) -> sam6d_fine_match_split, against
    chain64 -> fine_match64; tokens and bias scaled by 1e4 and 1e-4 (the normalisation removes the scale)"""
    _default_arithmetic()
    from sam6d_hip import pem
    x, W, b, pts2 = R.split_inputs(B, n, scale)
    F = R.chain64(x, W, b).reshape(2 * B, n, R.C)
    tol = R.chain_att_tol(0.1)
    want = R.fine_match64(F, B, 0.1, rel=R.label_rel(0.1, tol))
    L = pem.Linear(W.to(dev), b.to(dev))
    xd = x.to(dev).contiguous()
    fh, fl = pem.linear_norm_split(xd, L)
    out = _raw(dev, None, B, n, 0.1, pts2, halves=(fh, fl))
    _check(out, F, pts2, want, 0.1, "split entry B = %d, n = %d, scale %g" % (B, n, scale), tol=tol)
    assert int((out[0] > 0).sum()) > out[0].numel() // 2


# ------------------------------------------------------------------------------------------------------- 6. workspace
@pytest.mark.parametrize("B,n", [(2, R.N), (1, 4097)])
def test_no_kernel_reads_workspace_it_did_not_write(dev, B, n):
    """the same call on a zeroed workspace and on one filled with NaN bytes: bitwise-equal outputs"""
    F, pts2 = R.stack([R.proposal("matched", n, s) for s in range(B)])
    a = _raw(dev, F, B, n, 0.1, pts2, fill=0)
    b = _raw(dev, F, B, n, 0.1, pts2, fill=0xFF)
    for x, y, name in zip(a, b, ("label1", "label2", "pred", "weight")):
        assert torch.isfinite(y.float()).all()
        assert torch.equal(_bits(x), _bits(y)), name + " depends on what the workspace held"


def test_empty_batch_writes_nothing(dev):
    from sam6d_hip import _lib
    out = _outputs(dev, 1, R.N)
    ws, nbytes = _workspace(dev, 1, R.N)
    f = torch.zeros(2 * R.N, R.C, device=dev)
    p2 = torch.zeros(1, R.N - 1, 3, device=dev)
    _lib.call("sam6d_fine_match", f.data_ptr(), 0, R.N, 0.1, p2.data_ptr(), *[o.data_ptr() for o in out], ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(dev, match, n=R.N, temp=0.1, ws_short=0, pts2_off=0, fh_off=0, split=False):
    """one call with one argument wrong: rc < 0, the message names the argument, nothing is written"""
    from sam6d_hip import _lib
    lib = _lib.load()
    B = 1
    out = _outputs(dev, B, max(n, 2))
    ws, nbytes = _workspace(dev, B, R.N)
    f = torch.zeros(2 * B * max(n, R.N), R.C, device=dev)
    fh = torch.zeros(2 * B * max(n, R.N) * R.C + 8, dtype=torch.float16, device=dev)
    fl = torch.zeros_like(fh)
    p2 = torch.zeros(B * max(n, R.N) * 3 + 4, device=dev)
    tail = (B, n, ctypes.c_float(temp), p2.data_ptr() + pts2_off, *[o.data_ptr() for o in out], ws.data_ptr(), nbytes - ws_short, _stream())
    if split:
        rc = lib.sam6d_fine_match_split(fh.data_ptr() + fh_off, fl.data_ptr(), *tail)
    else:
        rc = lib.sam6d_fine_match(f.data_ptr(), *tail)
    msg = lib.sam6d_last_error().decode()
    torch.cuda.synchronize()
    assert rc < 0, "accepted (rc = %d)" % rc
    assert match in msg, "the message %r does not name %r" % (msg, match)
    assert _untouched(out), "a refused call wrote to its outputs"


@pytest.mark.parametrize("split", [False, True], ids=["sam6d_fine_match", "sam6d_fine_match_split"])
def test_documented_refusals(dev, split):
    from sam6d_hip import _lib
    lib = _lib.load()
    for n in (2048, 2050, 1025):
        assert int(lib.sam6d_fine_match_workspace_bytes_n(2, n)) == 0
        _refused(dev, "n = 2049 or 4097", n=n, split=split)
    assert int(lib.sam6d_fine_match_workspace_bytes_n(2, R.N)) == int(lib.sam6d_fine_match_workspace_bytes(2)) > 0
    assert int(lib.sam6d_fine_match_workspace_bytes_n(2, 4097)) > int(lib.sam6d_fine_match_workspace_bytes(2))
    _refused(dev, "ws_bytes", ws_short=1, split=split)
    _refused(dev, "pts2", pts2_off=4, split=split)
    _refused(dev, "temp", temp=0.0, split=split)
    if split:
        _refused(dev, "fh", fh_off=2, split=True)


# ------------------------------------------------------------------------------------------------------- 8. single-product arithmetic
def test_single_product_arithmetic_vs_float64(dev):
    """matmul mode 2 keeps the hi . hi product: labels of `matched` exact wherever float64 decides them by the margin of
    att_tol(temp, 2), weights to the bound from it.  (Exact on every label is more than this arithmetic can promise: the margin is 3.9e-2,
    160 columns of the case lie inside it -- tests/test_fine_shapes_host.py -- and one of them takes another of its float64 candidates;
    all 4096 row labels and the other 4095 column labels equal float64.  Measured weights 3.2e-4 relative, bound 2.0e-2.)"""
    from sam6d_hip import _lib
    lib = _lib.load()
    F, pts2, _ = R.case("matched", 0.1)
    tol = R.att_tol(0.1, 2)
    want = R.fine_match64(F, 2, 0.1, pts2, rel=R.label_rel(0.1, tol))
    before = lib.sam6d_get_thread_matmul_mode()
    assert lib.sam6d_set_thread_matmul_mode(2) == 0
    try:
        out = _raw(dev, F, 2, R.N, 0.1, pts2)
    finally:
        lib.sam6d_set_thread_matmul_mode(before)
    print("single product: %d row labels and %d column labels differ from float64 (%d / %d within the margin %.2e)" % (
        int((out[0].long() != want["l1"]).sum()), int((out[1].long() != want["l2"]).sum()), int(want["near1"].sum()), int(want["near2"].sum()),
        R.label_rel(0.1, tol)))
    _check(out, F, pts2, want, 0.1, "matched, single product", tol=tol)


# ------------------------------------------------------------------------------------------------------- 9. temperature range
@pytest.mark.parametrize("kind", ["antipodal", "flat"])
def test_smallest_temperature_vs_float64(dev, kind):
    """at sam6d_fine_match_min_temp() the fixed shift still holds cos = -1 (`antipodal`: 64 scene rows within 0.01 of it) and unrelated
    features: finite and within the bounds"""
    _default_arithmetic()
    from sam6d_hip import _lib, pem
    tmin = float(_lib.load().sam6d_fine_match_min_temp())
    assert tmin == pem.fine_match_min_temp() == float(torch.tensor(R.MIN_TEMP, dtype=torch.float32)), "one definition: 2 log2e / 125"
    F, pts2, want = R.case(kind, R.MIN_TEMP)
    _check(_raw(dev, F, 2, R.N, tmin, pts2), F, pts2, want, R.MIN_TEMP, "%s at the smallest temperature" % kind)


def test_below_the_smallest_temperature_both_entries_refuse(dev):
    from sam6d_hip import _lib, pem
    tmin = float(_lib.load().sam6d_fine_match_min_temp())
    below = float(torch.nextafter(torch.tensor(tmin, dtype=torch.float32), torch.tensor(0.0)))
    for temp in (below, 0.005):
        _refused(dev, "sam6d_fine_match_min_temp", temp=temp)
        _refused(dev, "sam6d_fine_match_min_temp", temp=temp, split=True)
    p2 = torch.zeros(1, R.N - 1, 3, device=dev)
    f = torch.zeros(2 * R.N, R.C, device=dev)
    with pytest.raises(ValueError, match="fine_match_min_temp"):
        pem.fine_match(f, 1, R.N, 0.005, p2)


def test_pem_match_routes_a_small_temperature_to_the_running_maximum(dev):
    """cfg["temp"] = 0.005 (synthetic weights, B = 2, 2048 dense points: the smallest cloud the fused route takes) goes through
    pem.fine_point_matching to feature_similarity + compute_fine_Rt: finite R, t, score, bit-equal to the fused_fine=False result,
    and resolve_routes / describe_paths report the route taken"""
    from sam6d_hip import pem, synth
    W = pem.PemWeights(synth.make_pem_weights(1), dev)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synth.config2_inputs(B=2, seed=5).items()}
    run = lambda cfg: pem.pem_match(d["dense_pm"], d["dense_fm"], d["dense_po"], d["dense_fo"], d["radius"], d["model"], W, d["rand"], cfg=cfg,
                                    return_aux=True)
    cold = dict(pem.DEFAULT_CFG, temp=0.005)
    Ra, ta, sa, aux = run(cold)
    Rb, tb, sb, _ = run(dict(cold, fused_fine=False))
    torch.cuda.synchronize()
    assert "atten" in aux["fine"], "below the smallest temperature the materialised route runs"
    for x, y in ((Ra, Rb), (ta, tb), (sa, sb)):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert "materialised" in pem.describe_paths(W, cold)["fine_match"] and "finematch.hip" in pem.describe_paths(W, pem.DEFAULT_CFG)["fine_match"]
