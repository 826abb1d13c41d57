"""The geometric structure embedding (csrc/geo.hip) and the fused RPE score kernel (csrc/rpe.hip) off the golden cloud: every stage
through the C ABI against the float64 restatements of tests/geo_shapes_ref.py -- kNN and indices on both sides of n = 64 / 128 / 192 /
256 (one to four candidates per lane, 256-pair blocks), the pair classification across its 4096-pair workgroups with an empty list and
a list of nearly every pair, the listed rows of both sinusoid kernels, the three embedding routes with indices exactly on the range ends,
the raw score term entry by entry on partial key tiles and with queries of every magnitude, the probabilities, the thin entry points and
the argument guards.  tests/test_geo_shapes_host.py proves the builders' conditions and that the fp32 oracle alone meets each bound of
R.TOL.  Every device tensor is named, so that no temporary dies before its launch; every output is pre-filled with NaN or a sentinel."""
import functools

import numpy as np
import pytest
import torch

from tests import geo_shapes_ref as R
from oracle import pem_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -777.0  # sentinel of buffers whose untouched part is compared bit for bit


@pytest.fixture(scope="module")
def sd():
    from sam6d_hip import synth
    return synth.make_pem_weights(1)


@pytest.fixture(scope="module")
def geo(sd, dev):
    """the embedding's weights on the device (pem.pack_geo), their packed images and the float64 copies of the restatements"""
    import types
    from sam6d_hip import pem
    W = pem.pack_geo(sd, dev)
    w = R.weights(sd)
    g = types.SimpleNamespace(W=W, w=w, dev=dev, packed=pem.geo_packed(W), cheb=pem.geo_cheb_packed(W),
                              dc=pem.cheb_coefficients(w.Wd, w.div), a_img={s: pem.geo_cheb_a_packed(W, s) for s in (15, 7.5)})
    assert pem.geo_images_in_range(W)
    torch.cuda.synchronize()
    return g


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from sam6d_hip import _lib
    _lib.call(name, *args)


def _maxerr(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite values"
    return float((got - want).abs().max()) if got.numel() else 0.0


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _ldp(n):
    return 4 * ((n + 3) // 4)


# ------------------------------------------------------------------------------------------------------- launches
def _indices(dev, pts, sigma_a=15):
    """sam6d_geo_indices -> (knn (B,n,3) int32, flag, idx (B,n,n,4)) on the CPU"""
    B, n, _ = pts.shape
    pts_d = pts.to(dev)
    knn_d = torch.full((B * n * 3 + 1,), -7, dtype=torch.int32, device=dev)
    idx_d = torch.full((B, n, n, 4), NAN, device=dev)
    _call("sam6d_geo_indices", pts_d.data_ptr(), B, n, R.SIGMA_D, R.factor_a(sigma_a), 3, knn_d.data_ptr(), idx_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    knn = knn_d.cpu()
    return knn[:-1].reshape(B, n, 3), int(knn[-1]), idx_d.cpu()


@functools.lru_cache(maxsize=None)
def _device_idx(kind, B, n, sigma_a=15):
    """the device's own indices of a seeded cloud (checked by test_indices_*), as the input of the later stages"""
    return _indices(torch.device("cuda:0"), R.cloud(kind, B, n), sigma_a)[2]


def _outliers(geo, idx_d, pairs, xa, flag_d, name="sam6d_geo_outliers2"):
    """classification + listed rows -> (pos, list, rows) on the device, sentinel-filled"""
    dev = geo.dev
    pos_d = torch.full((pairs,), -5, dtype=torch.int32, device=dev)
    lst_d = torch.full((pairs + 1,), -5, dtype=torch.int32, device=dev)
    rows_d = torch.full((pairs, R.C), SENT, device=dev)
    W = geo.W
    ranges = (R.XMAX, xa) if name.endswith("2") else (R.XMAX,)
    _call(name, idx_d.data_ptr(), pairs, *ranges, W.div_term.data_ptr(), geo.packed.data_ptr(), W.geo_d.w.data_ptr(),
          W.geo_a.w.data_ptr(), flag_d.data_ptr(), pos_d.data_ptr(), lst_d.data_ptr(), rows_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    return pos_d, lst_d, rows_d


def _check_lists(pos_d, lst_d, rows_d, listed, what):
    """list[0] = the reference count, list[1..count] = exactly the reference set, list[1 + pos[e]] == e, pos == -1 elsewhere; the list
    and the rows beyond the count keep their sentinel"""
    listed = listed.reshape(-1)
    pos, lst = pos_d.cpu().long(), lst_d.cpu().long()
    count = int(lst[0])
    want = listed.nonzero().reshape(-1)
    assert count == want.numel(), "%s: count %d, reference %d" % (what, count, want.numel())
    ids = lst[1:1 + count]
    assert torch.equal(ids.sort().values, want), what + ": the list is not the reference set, each pair once"
    assert bool((pos[~listed] == -1).all()), what + ": pos of an in-range pair"
    assert torch.equal(ids[pos[listed]], want), what + ": list[1 + pos[e]] != e"
    assert bool((lst[1 + count:] == -5).all()), what + ": list written beyond the count"
    assert bool((rows_d[count:] == SENT).all()), what + ": rows written beyond the count"
    return pos, count


# ------------------------------------------------------------------------------------------------------- 1. indices
INDEX_N = (4, 5, 63, 64, 65, 128, 129, 197, 255, 256)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", INDEX_N)
def test_indices_and_knn_shapes(dev, n, B):
    """sam6d_geo_indices on both sides of every 64 candidates of the wave arg-min and every 256-pair block: kNN bit for bit the stable
    (value, index) order -- bitwise duplicate points and quantised far distances tie --, d_idx the correctly rounded recipe, a_idx
    within TOL.a_idx of the oracle (its arithmetic on the neighbours of the documented tie rule: torch.topk orders the tied neighbours
    of the dup kind arbitrarily), the range flag clear, and raised by coordinates of +-2e4"""
    for kind in ("bg", "none", "dup", "mm", "flag"):
        pts = R.cloud(kind, B, n)
        knn, flag, idx = _indices(dev, pts)
        assert torch.equal(knn.long(), R.knn_stable(pts)), "%s: kNN differs from the stable (value, index) order" % kind
        assert np.array_equal(idx[..., 0].numpy(), R.d_idx_rounded(pts)), "%s: d_idx is not the correctly rounded recipe" % kind
        assert flag == (1 if kind == "flag" else 0), "%s: range flag %d" % (kind, flag)
        if kind == "flag":
            continue
        a = R.a_idx_oracle(pts, R.knn_stable(pts))
        if bool(R.knn_tie_free(pts).all()):
            assert torch.equal(a, O.geo_embedding_indices(pts)[1]), "%s: without ties this is the oracle's own a_idx" % kind
        else:
            assert kind in ("dup", "mm")
        e = _maxerr(idx[..., 1:], a)
        rec = float(np.abs(R.a_idx_recipe(pts, knn.long()).astype(np.float64) - a.numpy().astype(np.float64)).max())
        print("indices %s B %d n %d: a_idx max error %.2e / bit recipe on the CPU vs oracle %.2e / bound %.1e" % (kind, B, n, e, rec, R.TOL["a_idx"]))
        assert e <= R.TOL["a_idx"]


# ------------------------------------------------------------------------------------------------------- 2. classification, listed rows
# flag 0: the fp16x3 kernel fills the rows, flag 1: the exact kernel; the flagged cloud's indices (to 3e5) are the exact kernel's alone
LISTED_CASES = [(k, B, n, f) for k, B, n in (("bg", 2, 65), ("none", 2, 65), ("all", 2, 65), ("dup", 2, 65), ("mm", 2, 65), ("bg", 3, 17),
                                             ("all", 3, 17), ("mm", 1, 197)) for f in (0, 1)] + [("flag", 1, 40, 1)]


@pytest.mark.parametrize("kind,B,n,flag", LISTED_CASES)
def test_classification_and_listed_rows(geo, kind, B, n, flag):
    """sam6d_geo_outliers2 on the device's own indices: the list is the reference set (empty for a cloud without a bg token -- its rows
    buffer stays untouched --, every off-diagonal pair for the lattice), and rows[pos[e]] is the bias-free embedding row of the
    fp16x3 kernel (flag 0) / the exact kernel (flag 1) within TOL.rows of float64 with the fp32 argument"""
    xa = R.xmax_a(15)
    idx = _device_idx(kind, B, n)
    pairs = B * n * n
    idx_d = idx.to(geo.dev)
    flag_d = torch.full((1,), flag, dtype=torch.int32, device=geo.dev)
    pos_d, lst_d, rows_d = _outliers(geo, idx_d, pairs, xa, flag_d)
    listed = R.classify(idx, R.XMAX, xa).reshape(-1)
    what = "%s B %d n %d flag %d" % (kind, B, n, flag)
    pos, count = _check_lists(pos_d, lst_d, rows_d, listed, what)
    if kind == "none":
        assert count == 0 and bool((rows_d == SENT).all())
    if kind == "bg":
        assert count == B * (2 * n - 2)
    if kind == "all":
        assert count == B * (n * n - n)
    if count:
        sel = idx.reshape(-1, 4)[listed]
        got = rows_d.cpu()[pos[listed]]
        e, eo = _maxerr(got, R.rows64(sel, geo.w, True)), _maxerr(R.rows32(sel, geo.w), R.rows64(sel, geo.w, True))
        print("listed rows %s (%d rows): max error %.2e / fp32 oracle %.2e / bound %.1e" % (what, count, e, eo, R.TOL["rows"]))
        assert e <= R.TOL["rows"]


@pytest.mark.parametrize("pairs", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_classification_edge_indices(geo, pairs):
    """crafted indices exactly on the range ends across the 4096-pair workgroup of geo_classify_kernel: 0, -0.0, xmax and xmax_a are in
    range, the next float above either is listed; the last pair of all is listed (alone in its workgroup at 4097 and 8193)"""
    xa = R.xmax_a(15)
    idx = R.edge(1, pairs).reshape(pairs, 4)
    idx_d = idx.to(geo.dev)
    flag_d = torch.zeros(1, dtype=torch.int32, device=geo.dev)
    pos_d, lst_d, rows_d = _outliers(geo, idx_d, pairs, xa, flag_d)
    listed = R.classify(idx, R.XMAX, xa)
    assert bool(listed[-1])
    pos, count = _check_lists(pos_d, lst_d, rows_d, listed, "edge %d" % pairs)
    sel = idx[listed]
    e, eo = _maxerr(rows_d.cpu()[pos[listed]], R.rows64(sel, geo.w, True)), _maxerr(R.rows32(sel, geo.w), R.rows64(sel, geo.w, True))
    print("edge %d pairs, %d listed: rows max error %.2e / fp32 oracle %.2e / bound %.1e" % (pairs, count, e, eo, R.TOL["rows"]))
    assert e <= R.TOL["rows"]


# ------------------------------------------------------------------------------------------------------- 3. embedding routes
def _routes(geo, idx_d, pairs):
    """the three routes on one index tensor -> (exact, h3, cheb) (pairs,256) on the device, NaN-filled before"""
    dev, W = geo.dev, geo.W
    flag_d = torch.zeros(1, dtype=torch.int32, device=dev)
    ex_d, h3_d, ch_d = (torch.full((pairs, R.C), NAN, device=dev) for _ in range(3))
    pos_d = torch.full((pairs,), -5, dtype=torch.int32, device=dev)
    lst_d = torch.full((pairs + 1,), -5, dtype=torch.int32, device=dev)
    _call("sam6d_geo_embed", idx_d.data_ptr(), pairs, W.div_term.data_ptr(), W.geo_d.w.data_ptr(), W.geo_d.b.data_ptr(),
          W.geo_a.w.data_ptr(), W.geo_a.b.data_ptr(), R.C, flag_d.data_ptr(), 0, ex_d.data_ptr(), _stream())
    _call("sam6d_geo_embed_h3", idx_d.data_ptr(), pairs, W.div_term.data_ptr(), geo.packed.data_ptr(), W.geo_d.b.data_ptr(),
          W.geo_a.b.data_ptr(), R.C, flag_d.data_ptr(), h3_d.data_ptr(), _stream())
    _call("sam6d_geo_embed_cheb", idx_d.data_ptr(), pairs, geo.cheb.data_ptr(), R.XMAX, W.div_term.data_ptr(), geo.packed.data_ptr(),
          W.geo_d.b.data_ptr(), W.geo_a.b.data_ptr(), R.C, flag_d.data_ptr(), pos_d.data_ptr(), lst_d.data_ptr(), ch_d.data_ptr(),
          _stream())
    torch.cuda.synchronize()
    return ex_d, h3_d, ch_d


@pytest.mark.parametrize("kind", ["bg", "none", "all", "edge"])
@pytest.mark.parametrize("n", [4, 17, 65, 256])
def test_embedding_routes_vs_float64(geo, n, kind):
    """sam6d_geo_embed (exact fp32), sam6d_geo_embed_h3 (fp16x3 sinusoid) and sam6d_geo_embed_cheb (Chebyshev + list fix-up), each
    against float64 plus both biases -- the sinusoid kernels with the fp32 argument, the Chebyshev route with exact products on the
    pairs it serves itself --, the Chebyshev route against the exact kernel, and pem.geo_embedding against the route it documents"""
    from sam6d_hip import _lib, pem
    B = 2 if n <= 65 else 1
    idx = R.edge(B * n, n, R.XMAX, R.XMAX) if kind == "edge" else _device_idx(kind, B, n)
    pairs = B * n * n
    idx_d = idx.to(geo.dev)
    ex_d, h3_d, ch_d = _routes(geo, idx_d, pairs)
    flat = idx.reshape(pairs, 4)
    listed = R.classify(flat, R.XMAX, R.XMAX)
    r_arg32 = R.rows64(flat, geo.w, True) + geo.w.bias64
    r_served = R.rows64_served(flat, geo.w, listed) + geo.w.bias64
    eo = _maxerr(R.rows32(flat, geo.w).double() + geo.w.bias64, r_arg32)
    e_ex, e_h3, e_ch = _maxerr(ex_d, r_arg32), _maxerr(h3_d, r_arg32), _maxerr(ch_d, r_served)
    scale = float(ex_d.abs().max())
    e_ce = _maxerr(ch_d, ex_d.cpu())
    print("routes %s n %d (%d of %d pairs listed): exact %.2e, fp16x3 %.2e, Chebyshev %.2e / fp32 oracle %.2e / bound %.1e; "
          "Chebyshev vs exact %.2e / bound %.2e" % (kind, n, int(listed.sum()), pairs, e_ex, e_h3, e_ch, eo, R.TOL["rows"], e_ce,
                                                    R.TOL["cheb_vs_exact"] * max(1.0, scale)))
    assert e_ex <= R.TOL["rows"] and e_h3 <= R.TOL["rows"] and e_ch <= R.TOL["rows"]
    assert e_ce <= R.TOL["cheb_vs_exact"] * max(1.0, scale)
    if kind == "edge":
        return
    pts_d = R.cloud(kind, B, n).to(geo.dev)
    default = pem.geo_embedding(pts_d, geo.W).reshape(pairs, R.C)
    route = ex_d if _lib.load().sam6d_get_matmul_mode() == 0 else ch_d
    assert _same_bits(default, route), "pem.geo_embedding (default mode) is not its documented route"
    try:
        _call("sam6d_set_thread_matmul_mode", 0)
        mode0 = pem.geo_embedding(pts_d, geo.W).reshape(pairs, R.C)
    finally:
        _call("sam6d_set_thread_matmul_mode", -1)
    assert _same_bits(mode0, ex_d), "pem.geo_embedding (mode 0) is not the exact kernel"


def test_embedding_flagged_cloud(geo):
    """coordinates of +-2e4 raise the range flag: the default mode's result is bit-equal to mode 0's, and the exact kernel stays within
    TOL.rows of float64 with the fp32 argument at indices up to 3e5"""
    from sam6d_hip import pem
    B, n = 1, 40
    pts = R.cloud("flag", B, n)
    pts_d = pts.to(geo.dev)
    _, flag, idx = _indices(geo.dev, pts)
    assert flag == 1 and float(idx.max()) >= R.FLAG_LIMIT
    default = pem.geo_embedding(pts_d, geo.W)
    try:
        _call("sam6d_set_thread_matmul_mode", 0)
        mode0 = pem.geo_embedding(pts_d, geo.W)
    finally:
        _call("sam6d_set_thread_matmul_mode", -1)
    assert _same_bits(default, mode0)
    flat = idx.reshape(-1, 4)
    want = R.rows64(flat, geo.w, True) + geo.w.bias64
    e, eo = _maxerr(mode0.reshape(-1, R.C), want), _maxerr(R.rows32(flat, geo.w).double() + geo.w.bias64, want)
    print("flagged cloud (indices to %.3g): exact kernel %.2e / fp32 oracle %.2e / bound %.1e" % (float(idx.max()), e, eo, R.TOL["rows"]))
    assert e <= R.TOL["rows"]


# ------------------------------------------------------------------------------------------------------- 4. score term
def _score_B(n):
    return 5 if n == 4 else 2 if n <= 65 else 1


def _score_idx(kind, B, n, sigma_a):
    """(Q,n,4) indices of B clouds (Q = B n queries): the device's own, or the crafted edge tensor on this sigma_a's angular range"""
    if kind == "edge":
        return R.edge(B * n, n, R.XMAX, R.xmax_a(sigma_a))
    return _device_idx(kind, B, n, sigma_a).reshape(B * n, n, 4)


def _geo_scores(geo, idx, qp, qd, Q, n, sigma_a, products, name="sam6d_rpe_geo_scores", qk=None, xmax_first_only=False):
    """classification of the first Q queries' pairs, then the score entry point -> (out (Q,4,ldp), qk after the call or None), CPU.
    The pair list is built for exactly Q n pairs: the listed pass addresses its output by pair id."""
    dev = geo.dev
    ldp = _ldp(n)
    img, xa, _, fits = geo.a_img[sigma_a]
    assert fits
    idx_d = idx[:Q].contiguous().to(dev)
    flag_d = torch.zeros(1, dtype=torch.int32, device=dev)
    pos_d, lst_d, rows_d = _outliers(geo, idx_d, Q * n, xa, flag_d)
    qp_d, qd_d = qp[:Q].contiguous().to(dev), qd[:Q * R.H].contiguous().to(dev)
    out_d = torch.full((Q, R.H, ldp), SENT, device=dev)
    head = [idx_d.data_ptr(), pos_d.data_ptr(), lst_d.data_ptr(), rows_d.data_ptr(), img.data_ptr()]
    ranges = [R.XMAX] if xmax_first_only else [R.XMAX, xa, products]
    qk_d = None
    if qk is None:
        _call(name, *head, *ranges, qp_d.data_ptr(), qd_d.data_ptr(), out_d.data_ptr(), Q, n, ldp, _stream())
    else:
        qk_d = torch.full((Q, R.H, ldp), SENT, device=dev)
        qk_d[:, :, :n] = qk[:Q].to(dev)
        _call(name, *head, *ranges, qp_d.data_ptr(), qd_d.data_ptr(), qk_d.data_ptr(), out_d.data_ptr(), Q, n, ldp, _stream())
    torch.cuda.synchronize()
    return out_d.cpu(), (qk_d.cpu() if qk_d is not None else None)


def _check_G(G, G64, gb, n, what, oracle_ratio):
    assert bool((G[:, :, n:] == SENT).all()), what + ": padding columns written"
    g = G[:, :, :n].double()
    assert torch.isfinite(g).all(), what + ": non-finite scores"
    err = (g - G64).abs()
    ratio = float((err / gb.clamp_min(1e-300)).max()) if bool((gb > 0).any()) else 0.0
    print("%s: max |G - G64| %.3e = %.3f of g_bound / fp32 oracle %.3f of g_bound / bound 1" % (what, float(err.max()), ratio, oracle_ratio))
    bad = err > gb
    worst = np.unravel_index(int((err / gb.clamp_min(1e-300)).flatten().argmax()), tuple(err.shape))
    assert not bool(bad.any()), "%s: %d entries beyond g_bound, worst %.3f of it at (q, h, m) = %s" % (what, int(bad.sum()), ratio, worst)


SCORE_N = (4, 15, 16, 17, 64, 65, 197, 208, 209, 256)
SCORE_CASES = [(n, 15) for n in SCORE_N] + [(n, 7.5) for n in (4, 17, 65, 209)]


@pytest.mark.parametrize("kind", ["bg", "none", "all", "edge"])
@pytest.mark.parametrize("n,sigma_a", SCORE_CASES)
def test_score_term_vs_float64(geo, n, sigma_a, kind):
    """sam6d_rpe_geo_scores entry by entry: full and partial key tiles of 16 (n = 15 / 16 / 17, 208 / 209: 13 / 14 tiles, a last tile of
    one key), two and three stage-1 products on the short angular range and three on the long one, Q = 1, 17 and B n queries, lists that
    are empty (none), 2n - 2 a cloud (bg), every off-diagonal pair (all) or sit on the range ends and in the last key of a tile (edge)"""
    B = _score_B(n)
    Qfull = B * n
    idx = _score_idx(kind, B, n, sigma_a)
    listed = R.classify(idx, R.XMAX, R.xmax_a(sigma_a))
    E64 = R.rows64_served(idx, geo.w, listed)
    qp = R.queries(Qfull, seed=n)
    qd = R.fold_qd(qp, geo.dc)
    G64, gb = R.scores64(qp, E64), R.g_bound(qp, E64)
    G32 = torch.einsum("qhc,qmc->qhm", qp, R.rows32(idx, geo.w))
    oracle_ratio = float(((G32.double() - G64).abs() / gb).max())
    for products in ((2, 3) if sigma_a == 15 else (3,)):
        for Q in sorted({1, min(17, Qfull), Qfull}):
            G, _ = _geo_scores(geo, idx, qp, qd, Q, n, sigma_a, products)
            _check_G(G, G64[:Q], gb[:Q], n, "G %s n %d sigma_a %g products %d Q %d" % (kind, n, sigma_a, products, Q), oracle_ratio)


def test_score_term_many_queries(geo):
    """Q = 49 x 64 = 3136 queries at n = 64: more than 12 waves on each of 256 CUs, so every workgroup's waves take queries from its
    counter more than once"""
    B, n = 49, 64
    idx = _score_idx("bg", B, n, 15)
    listed = R.classify(idx, R.XMAX, R.xmax_a(15))
    assert int(listed.sum()) == B * (2 * n - 2)
    E64 = R.rows64_served(idx, geo.w, listed)
    qp = R.queries(B * n, seed=3)
    qd = R.fold_qd(qp, geo.dc)
    G, _ = _geo_scores(geo, idx, qp, qd, B * n, n, 15, 2)
    _check_G(G, R.scores64(qp, E64), R.g_bound(qp, E64), n, "G bg n 64 Q 3136", float("nan"))


@pytest.mark.parametrize("products", [2, 3])
@pytest.mark.parametrize("name", R.MAGNITUDES)
def test_score_term_query_magnitudes(geo, name, products):
    """the per-query power-of-two scaling of the folded query: common factors from 2^-60 to 2^40, an all-zero query (its scores are
    exactly 0, listed keys included) and a query with one channel 5e4 times the rest, n = 65"""
    B, n = 1, 65
    idx = _score_idx("bg", B, n, 15)
    listed = R.classify(idx, R.XMAX, R.xmax_a(15))
    E64 = R.rows64_served(idx, geo.w, listed)
    qp = R.magnitude_variant(R.queries(n, seed=65), name)
    qd = R.fold_qd(qp, geo.dc)
    G64, gb = R.scores64(qp, E64), R.g_bound(qp, E64)
    G32 = torch.einsum("qhc,qmc->qhm", qp, R.rows32(idx, geo.w))
    oracle_ratio = float(((G32.double() - G64).abs() / gb.clamp_min(1e-300)).max())
    G, _ = _geo_scores(geo, idx, qp, qd, n, n, 15, products)
    _check_G(G, G64, gb, n, "G magnitudes %s products %d" % (name, products), oracle_ratio)
    if name == "zero_query":
        assert float(G[1, :, :n].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------- 5. probabilities
@pytest.mark.parametrize("kind", ["bg", "edge"])
@pytest.mark.parametrize("n", [5, 16, 209, 240, 256])
def test_probabilities_vs_float64(geo, n, kind):
    """sam6d_rpe_scores2: P against the float64 softmax of (qk + G64) / 8 within p_bound, rows summing to 1, padding untouched; and the
    documented side effect on qk -- bit-unchanged at the pairs the score kernel serves, qk + G64 within g_bound at the listed ones"""
    B = 4 if n <= 16 else 1
    Q = B * n
    idx = _score_idx(kind, B, n, 15)
    listed = R.classify(idx, R.XMAX, R.xmax_a(15))
    E64 = R.rows64_served(idx, geo.w, listed)
    qp = R.queries(Q, seed=n, l1=8.0)
    qd = R.fold_qd(qp, geo.dc)
    qk = torch.randn(Q, R.H, n, generator=R.gen(40 + n)) * 4.0
    G64, gb = R.scores64(qp, E64), R.g_bound(qp, E64)
    P64, s64 = R.probs64(qk, G64)
    pb = R.p_bound(P64, gb, s64)
    P32 = torch.softmax((qk + torch.einsum("qhc,qmc->qhm", qp, R.rows32(idx, geo.w))) * 0.125, dim=2)
    oracle_ratio = float(((P32.double() - P64).abs() / pb).max())
    for products in (2, 3):
        what = "P %s n %d products %d" % (kind, n, products)
        P, qk_after = _geo_scores(geo, idx, qp, qd, Q, n, 15, products, name="sam6d_rpe_scores2", qk=qk)
        assert bool((P[:, :, n:] == SENT).all()) and bool((qk_after[:, :, n:] == SENT).all()), what + ": padding written"
        p = P[:, :, :n].double()
        assert torch.isfinite(p).all()
        err = (p - P64).abs()
        ratio, rs = float((err / pb).max()), float((p.sum(2) - 1.0).abs().max())
        print("%s: max |P - P64| %.3e = %.3f of p_bound / fp32 oracle %.3f of p_bound / bound 1; row sums off by %.2e / bound %.2e"
              % (what, float(err.max()), ratio, oracle_ratio, rs, R.rowsum_tol(n)))
        assert bool((err <= pb).all()), what + ": beyond p_bound (%.3f of it)" % ratio
        assert rs <= R.rowsum_tol(n)
        lm = listed[:, None, :].expand(Q, R.H, n)
        ka = qk_after[:, :, :n]
        assert torch.equal(_bits(ka)[~lm], _bits(qk)[~lm]), what + ": qk changed at a pair the score kernel serves"
        if bool(lm.any()):
            side = ((ka.double() - (qk.double() + G64)).abs() / gb)[lm]
            print("%s: qk side effect at the %d listed entries: %.3f of g_bound" % (what, int(lm.sum()), float(side.max())))
            assert float(side.max()) <= 1.0


# ------------------------------------------------------------------------------------------------------- 6. thin entry points
def test_thin_entry_points(geo):
    """sam6d_geo_outliers == sam6d_geo_outliers2 with xmax_a = xmax; sam6d_rpe_scores == sam6d_rpe_scores2 with xmax_a = xmax and three
    products; sam6d_geo_embed_h3 == the fp16x3 result inside sam6d_geo_embed_cheb for an all-listed input -- each bit for bit"""
    dev = geo.dev
    B, n = 2, 17  # 578 pairs: one classification workgroup, so the list order is fixed
    idx = _device_idx("bg", B, n, 7.5)
    pairs = B * n * n
    idx_d = idx.to(dev)
    flag_d = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _outliers(geo, idx_d, pairs, R.XMAX, flag_d, "sam6d_geo_outliers")
    b = _outliers(geo, idx_d, pairs, R.XMAX, flag_d, "sam6d_geo_outliers2")
    assert int(a[1][0]) == B * (2 * n - 2)
    for x, y, what in zip(a, b, ("pos", "list", "rows")):
        assert _same_bits(x, y), "sam6d_geo_outliers: %s differs from sam6d_geo_outliers2" % what

    Q = B * n
    idx3 = idx.reshape(Q, n, 4)
    qp = R.queries(Q, seed=1, l1=8.0)
    qd = R.fold_qd(qp, geo.dc)
    qk = torch.randn(Q, R.H, n, generator=R.gen(2)) * 4.0
    assert geo.a_img[7.5][1] == R.XMAX and geo.a_img[7.5][2] == 3
    P1, k1 = _geo_scores(geo, idx3, qp, qd, Q, n, 7.5, 3, name="sam6d_rpe_scores", qk=qk, xmax_first_only=True)
    P2, k2 = _geo_scores(geo, idx3, qp, qd, Q, n, 7.5, 3, name="sam6d_rpe_scores2", qk=qk)
    assert _same_bits(P1, P2) and _same_bits(k1, k2)
    assert abs(float(P1[:, :, :n].sum(2).mean()) - 1.0) < 1e-5

    pairs = 5000
    far = R.all_listed(pairs)
    far_d = far.to(dev)
    _, h3_d, ch_d = _routes(geo, far_d, pairs)
    assert _same_bits(h3_d, ch_d)
    assert _maxerr(h3_d, R.rows64(far, geo.w, True) + geo.w.bias64) <= R.TOL["rows"]


# ------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_outputs_untouched(geo):
    """arguments the SAM6D_REQUIRE guards reject before any launch: n = 3 and n = 257 (geo_indices), n = 257, ldp < n and products = 4
    (the score entry points), a misaligned idx_ws -- each raises RuntimeError and the outputs keep their sentinel"""
    dev, W = geo.dev, geo.W
    pts_d = torch.rand(1, 260, 3, generator=R.gen(1)).to(dev)
    knn_d = torch.full((260 * 3 + 1,), -7, dtype=torch.int32, device=dev)
    idx_d = torch.full((260 * 260 * 4 + 4,), SENT, device=dev)
    for n in (3, 257):
        with pytest.raises(RuntimeError):
            _call("sam6d_geo_indices", pts_d.data_ptr(), 1, n, R.SIGMA_D, R.factor_a(15), 3, knn_d.data_ptr(), idx_d.data_ptr(), _stream())
    with pytest.raises(RuntimeError):
        _call("sam6d_geo_indices", pts_d.data_ptr(), 1, 16, R.SIGMA_D, R.factor_a(15), 3, knn_d.data_ptr(), idx_d.data_ptr() + 4, _stream())
    torch.cuda.synchronize()
    assert bool((knn_d == -7).all()) and bool((idx_d == SENT).all())

    n, Q = 16, 16
    ldp = _ldp(n)
    img, xa, _, _ = geo.a_img[15]
    big = 257 * 257
    in_d = torch.rand(big * 4 + 4, generator=R.gen(2)).to(dev)  # in-range indices, room for n = 257 and for the shifted pointer
    pos_d = torch.full((big,), -1, dtype=torch.int32, device=dev)
    lst_d = torch.zeros(big + 1, dtype=torch.int32, device=dev)
    rows_d = torch.full((16, R.C), SENT, device=dev)
    qp_d = torch.randn(257, R.H, R.C, generator=R.gen(3)).to(dev)
    qd_d = torch.randn(257 * R.H, R.K, generator=R.gen(4)).to(dev)
    qk_d = torch.full((257, R.H, 260), SENT, device=dev)
    out_d = torch.full((257, R.H, 260), SENT, device=dev)
    flag_d = torch.zeros(1, dtype=torch.int32, device=dev)

    def scores(name, idx_ptr, products, Qn, nn, ld):
        extra = [qk_d.data_ptr()] if name == "sam6d_rpe_scores2" else []
        _call(name, idx_ptr, pos_d.data_ptr(), lst_d.data_ptr(), rows_d.data_ptr(), img.data_ptr(), R.XMAX, xa, products, qp_d.data_ptr(),
              qd_d.data_ptr(), *extra, out_d.data_ptr(), Qn, nn, ld, _stream())

    for name in ("sam6d_rpe_geo_scores", "sam6d_rpe_scores2"):
        for args in ((in_d.data_ptr(), 3, 257, 257, 260), (in_d.data_ptr(), 3, Q, n, n - 4), (in_d.data_ptr(), 4, Q, n, ldp),
                     (in_d.data_ptr() + 4, 3, Q, n, ldp)):
            with pytest.raises(RuntimeError):
                scores(name, *args)
    with pytest.raises(RuntimeError):
        _call("sam6d_geo_outliers2", in_d.data_ptr() + 4, 16, R.XMAX, xa, W.div_term.data_ptr(), geo.packed.data_ptr(), W.geo_d.w.data_ptr(),
              W.geo_a.w.data_ptr(), flag_d.data_ptr(), pos_d.data_ptr(), lst_d.data_ptr(), rows_d.data_ptr(), _stream())
    with pytest.raises(RuntimeError):
        _call("sam6d_geo_embed", in_d.data_ptr() + 4, 16, W.div_term.data_ptr(), W.geo_d.w.data_ptr(), W.geo_d.b.data_ptr(),
              W.geo_a.w.data_ptr(), W.geo_a.b.data_ptr(), R.C, flag_d.data_ptr(), 0, rows_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool((out_d == SENT).all()) and bool((qk_d == SENT).all()) and bool((rows_d == SENT).all())
    assert bool((pos_d == -1).all()) and bool((lst_d == 0).all())
